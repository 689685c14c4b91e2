"""CPU: the host side of the head backward (include/pose_mi355x.h: pmx_backward_head).  The NumPy twin of the documented sums and of the
Mconv1 channel map (tests/head_backward_twin.py) on examples where a wrong order or a wrong permutation changes the result; the transposed
pack in concat-buffer order from a stand-alone program (tests/conv_flip_cat_main.c + tests/conv_bwd_pack.h, host compiler), built plainly and
with -fsanitize=address,undefined; the C ABI surface."""
import os
import re
import shutil
import subprocess

import numpy as np

import conv_bwd_ref as R
import head_backward_twin as T
from conftest import pkg

ENTRIES = ['pmx_backward_enable', 'pmx_backward_head', 'pmx_get_layer_grad', 'pmx_get_trunk_grad', 'pmx_get_retained']


def test_channel_map_is_concat_maps_meaning():
    """F.concat((h1, h2, feature_map)) channel c (0..37 PAF, 38..56 heat, 57..184 feature) lives at concat-buffer channel: feature -> 0..127,
    PAF -> 128..165, heat -> 168..186; 166, 167 and 187..191 are pads.  Every channel carries its own integer, so any permutation shows."""
    src = open(os.path.join(R.CSRC, 'pmx_common.h')).read()
    for name, val in (('PMX_CAT_C', T.CAT_C), ('PMX_CAT_FEAT', T.CAT_FEAT), ('PMX_CAT_PAF', T.CAT_PAF), ('PMX_CAT_HEAT', T.CAT_HEAT)):
        assert int(re.search(r'#define %s (\d+)' % name, src).group(1)) == val
    ref = np.arange(1, 186).reshape(1, 185)          # reference channel r holds r + 1
    cat = T.to_cat(ref)
    assert cat.shape == (1, 192)
    assert np.array_equal(cat[0, 0:128], np.arange(58, 186))          # feature
    assert np.array_equal(cat[0, 128:166], np.arange(1, 39))          # PAF
    assert np.array_equal(cat[0, 168:187], np.arange(39, 58))         # heat
    assert not cat[0, 166:168].any() and not cat[0, 187:].any()
    assert np.array_equal(T.to_ref(cat), ref)                          # pads dropped, order restored
    m = T.ref_of_cat()
    assert sorted(m[m >= 0]) == list(range(185)) and (m < 0).sum() == 7
    assert np.array_equal(m[T.cat_of_ref()], np.arange(185))
    # a weight gradient accumulated in buffer order, [cout][192][tap]: element (co, k, t) holds 1000 co + 4 k + t
    dw_cat = (1000 * np.arange(2)[:, None, None] + 4 * np.arange(192)[None, :, None] + np.arange(4)[None, None, :]).reshape(2, 192, 2, 2)
    dw_ref = T.to_ref(dw_cat, axis=1)
    assert dw_ref.shape == (2, 185, 2, 2)
    for r, k in ((0, 128), (37, 165), (38, 168), (56, 186), (57, 0), (184, 127)):
        assert np.array_equal(dw_ref[:, r], dw_cat[:, k]), (r, k)


def test_sum_orders_are_left_to_right_float32():
    big, one = np.float32(2.0 ** 24), np.float32(1.0)
    lg, d1, d2 = np.array([one, big], 'f'), np.array([big, one], 'f'), np.array([-big, one], 'f')
    u = T.stage_sum(lg, d1, d2)
    assert u.dtype == np.float32
    assert np.array_equal(u, np.array([(one + big) - big, (big + one) + one], 'f'))          # [0, 2^24]: any other order gives [1, 2^24 + 2]
    assert np.array_equal(u, np.array([0.0, 2.0 ** 24], 'f'))
    assert np.array_equal(T.stage_sum(lg), lg)
    names = T.feature_order(6)
    assert len(names) == 12 and names[0] == 'Mconv1_stage6_L1' and names[1] == 'Mconv1_stage6_L2' and names[2] == 'Mconv1_stage5_L1'
    assert names[9] == 'Mconv1_stage2_L2' and names[10:] == ['conv5_1_CPM_L1', 'conv5_1_CPM_L2']
    assert T.feature_order(1) == ['conv5_1_CPM_L1', 'conv5_1_CPM_L2'] and len(T.feature_order(2)) == 4
    # twelve contributions whose float32 sum depends on the order: 2^24, then ten ones (each lost), then -2^24
    contrib = [np.array([big], 'f')] + [np.array([one], 'f')] * 10 + [np.array([-big], 'f')]
    assert T.feature_sum(contrib)[0] == 0.0          # left to right: every 2^24 + 1 rounds back to 2^24
    assert T.feature_sum(contrib[::-1])[0] == 10.0   # (the reverse order keeps every one: -2^24 + 1 is exact)
    assert np.array_equal(T.chain_sum(d1), d1)


def _cc():
    cc = shutil.which('gcc') or shutil.which('cc')
    assert cc, 'no host C compiler'
    return cc


def _build(tmp_path, name, extra):
    exe = os.path.join(str(tmp_path), name)
    cmd = [_cc(), '-O1', '-g', '-ffp-contract=off', '-Wall', '-Wextra', '-Werror', '-I', R.CSRC] + list(extra) + \
          [os.path.join(R.HERE, 'conv_flip_cat_main.c'), '-o', exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _words(line, what):
    head, *rest = line.split()
    assert head == what
    return np.array([int(v, 16) for v in rest], np.uint32).view(np.float32)


def test_transposed_pack_in_concat_order_plain_and_sanitized(tmp_path):
    def run(exe):
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
        return r.stdout
    plain = run(_build(tmp_path, 'flip_cat', []))
    san = run(_build(tmp_path, 'flip_cat_san', ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer']))
    assert plain.encode() == san.encode()
    lines = plain.splitlines()
    assert len(lines) == 1 + 3 * 3
    assert np.array_equal(np.array(lines[0].split()[1:], int), T.ref_of_cat())
    for c, (cout, ks) in enumerate(((2, 3), (1, 7), (3, 1))):
        assert lines[1 + 3 * c] == 'case %d cout %d ks %d' % (c, cout, ks)
        w = _words(lines[2 + 3 * c], 'w').reshape(cout, 185, ks, ks)
        wt = _words(lines[3 + 3 * c], 'wt').reshape(192, cout, ks, ks)
        assert np.abs(w).max() <= 1 and len(np.unique(w)) > 100
        want = T.flip_weights_cat(w)
        assert np.array_equal(wt.view(np.uint32), want.view(np.uint32))          # the pad rows +0.0f by bits, nothing of the 0xFF fill left
        flipped = R.flip_weights(w)                                               # (185, cout, k, k), reference order
        for r, k in ((0, 128), (37, 165), (38, 168), (56, 186), (57, 0), (184, 127)):
            assert np.array_equal(wt[k], flipped[r]), (r, k)
        assert not wt[[166, 167, 187, 188, 189, 190, 191]].view(np.uint32).any()


def test_transposed_layer_in_concat_order_gives_the_data_gradient():
    """conv(g, flip_weights_cat(w)) is the gradient at a 185-channel input, laid out in concat-buffer order (float64 autograd)."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(8)
    w = rng.standard_normal((3, 185, 7, 7)).astype('f')
    g = rng.standard_normal((1, 3, 4, 5)).astype('f')
    dx64 = R.conv_grads64(g, np.zeros((1, 185, 4, 5), 'f'), w)[0]
    got = F.conv2d(torch.tensor(g, dtype=torch.float64), torch.tensor(T.flip_weights_cat(w), dtype=torch.float64), padding=3).numpy()
    assert got.shape == (1, 192, 4, 5)
    assert np.abs(T.to_ref(got) - dx64).max() <= 1e-12 * np.abs(dx64).max()
    assert not got[:, T.ref_of_cat() < 0].any()


def test_head_backward_entries_declared_exported_and_bound(native):
    syms = native.header_symbols()
    lib = native.load()
    for e in ENTRIES:
        assert e in syms and hasattr(lib, e) and e in lib._pmx_sig, e
    assert [len(lib._pmx_sig[e][1]) for e in ENTRIES] == [2, 1, 4, 2, 4]
    for m in ('backward_enable', 'backward_head', 'layer_grad', 'trunk_grad', 'retained', 'head_layers'):
        assert callable(getattr(native.Engine, m)), m
    assert callable(pkg('pose_detector').PoseDetector.head_gradients)
    assert open(native.HEADER).read().count('#define PMX_ABI_VERSION 2') == 1
    table = pkg('weights').layer_table()
    assert len([n for n, _, _, _ in table if n not in native.Engine.TRUNK_LAYERS]) == 82
