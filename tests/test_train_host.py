"""Host side of the head training step, no GPU: the NumPy twin of the Adam contract (tests/adam_twin.py) against a float64 evaluation of
Chainer's formula, alpha_t against its closed form, the zero-gradient case, and the definition of the weight packs the device packers
evaluate (csrc/pack_index.h, through the stand-alone program tests/pack_index_main.c): its index arithmetic and, on seeded weights, every
float of every pack bit for bit against the NumPy restatement tests/pack_ref.py."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import adam_twin as A
import conv_bwd_ref as R
import pack_ref as P
from conftest import pkg

ENTRIES = ['pmx_train_enable', 'pmx_train_set_adam', 'pmx_train_set_grad_scale', 'pmx_train_step_head', 'pmx_get_layer',
           'pmx_train_get_state', 'pmx_train_set_state', 'pmx_get_pack', 'pmx_adam_apply']


def _case(seed, n=4096, first=False):
    rng = np.random.default_rng(seed)
    w = rng.normal(0, 0.05, n).astype('f')
    grad = (rng.normal(0, 1, n) * 10.0 ** rng.uniform(-6, 0, n)).astype('f')
    if first:
        return w, np.zeros(n, 'f'), np.zeros(n, 'f'), grad
    m = (rng.normal(0, 1, n) * 10.0 ** rng.uniform(-6, 0, n)).astype('f')
    v = (rng.uniform(0, 1, n) * 10.0 ** rng.uniform(-12, 0, n)).astype('f')
    return w, m, v, grad


@pytest.mark.parametrize('first,t,scale,alpha', [(True, 1, 1.0, 1e-4), (True, 1, 0.25, 1e-4), (False, 2, 1.0, 1e-4), (False, 1000, 0.25, 1e-5),
                                                 (False, 7, 0.3, 1e-4)])
def test_twin_against_float64_chainer_formula(first, t, scale, alpha):
    w, m, v, grad = _case(10 * t + int(first), first=first)
    scale = float(np.float32(scale))          # (the library rounds the scale to float32 once; both evaluations get that value)
    w32, m32, v32 = A.step32(w, m, v, grad, scale, t, alpha=alpha)
    w64, m64, v64 = A.step64(w, m, v, grad, scale, t, alpha=alpha)
    err = np.abs(w32.astype(np.float64) - w64)
    # the bound: adam_twin.bound32 -- the absolute error carried through the thirteen float32 roundings between gradient and weight and
    # the rounded constants, each at most u = 2^-24 relative, first order (its docstring has the derivation line by line)
    bound = A.bound32(w, m, v, grad, scale, t, alpha=alpha)
    print('max err', err.max(), 'max err / bound', (err / bound).max(), 'max |dw|', np.abs(w64 - w).max())
    assert np.isfinite(w32).all() and (err <= bound).all()
    assert (np.abs(w64 - w) > 0).any()
    # the bound is no loose one: a weight change off by one part in 1000 of the largest change breaks it somewhere
    assert (np.abs((w64 - w) * 1e-3) > bound).any()


def test_alpha_t_closed_form():
    for t in (1, 2, 1000):
        want = 1e-4 * math.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        assert A.alpha_t64(t) == want and A.alpha_t(t) == np.float32(want)
    # t = 1: sqrt(1 - b2) / (1 - b1) = sqrt(0.001) / 0.1
    assert abs(A.alpha_t64(1) / (1e-4 * math.sqrt(0.001) / 0.1) - 1) < 1e-12
    assert abs(A.alpha_t64(2) / (1e-4 * math.sqrt(0.001 * 1.999) / 0.19) - 1) < 1e-12
    assert abs(A.alpha_t64(10 ** 6) / 1e-4 - 1) < 1e-12          # the correction dies out
    assert A.alpha_t(1, alpha=1e-5) == np.float32(1e-5 * math.sqrt(1 - 0.999) / (1 - 0.9))


def test_zero_gradient_on_fresh_state_leaves_the_weights():
    w = np.array([0.5, -0.25, 0.0, -0.0, 1e-30, 3.0], 'f')
    z = np.zeros_like(w)
    for g in (z, -z):
        w1, m1, v1 = A.step32(w, z, z, g, 1.0, 1)
        assert np.array_equal(w1.view(np.uint32), w.view(np.uint32))
        assert not np.isnan(w1).any() and not m1.any() and not v1.any()


# ---- the shared index arithmetic -----------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _index_program(tmp_path_factory):
    cc = shutil.which('gcc') or shutil.which('cc')
    assert cc, 'no host C compiler'
    exe = os.path.join(str(tmp_path_factory.mktemp('pack_index')), 'pack_index_main')
    r = subprocess.run([cc, '-O1', '-g', '-ffp-contract=off', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', R.CSRC,
                        os.path.join(R.HERE, 'pack_index_main.c'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope='module')
def index_exe(tmp_path_factory):
    return _index_program(tmp_path_factory)


@pytest.mark.parametrize('cout,cin,ks,kind', [(128, 128, 3, 0), (128, 185, 7, 1), (38, 512, 1, 0)])
def test_index_maps_against_numpy_packers(index_exe, cout, cin, ks, kind):
    T = ks * ks
    r = subprocess.run([index_exe, str(cout), str(cin), str(ks), str(kind)], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    words = np.frombuffer(r.stdout, np.int64)
    nch, cout_pad, cin_pad, t_nch, t_cout_pad, t_cout, planes = words[:7]
    cmap = P.channel_map(kind, cin)
    assert cout_pad == (64 if cout <= 64 else -(-cout // 128) * 128) and cin_pad == len(cmap) and nch * 16 == cin_pad
    assert np.array_equal(words[7:7 + cin_pad], cmap)
    nw = cout * cin * T
    pairs = words[7 + cin_pad:7 + cin_pad + 2 * nw].reshape(nw, 2)
    ids = np.arange(nw, dtype=np.int64).reshape(cout, cin, T)
    # the forward pack
    wp = P.pack_weights(ids, cmap, cout_pad)
    assert np.array_equal(wp[pairs[:, 0]], ids.reshape(-1)) and (wp >= 0).sum() == nw
    # the transposed pack: transposed, rotated by 180 degrees, rows in the packed order of the layer's input, through pack_weights with the
    # g map (cout channels, padded to 64 at least)
    wt = P.transposed_weights(ids, cmap, len(cmap) if kind == 1 else cin)
    gmap = np.concatenate([np.arange(cout), np.full(max(64, -(-cout // 16) * 16) - cout, -1)])
    assert t_cout == wt.shape[0] and t_nch * 16 == len(gmap)
    wpt = P.pack_weights(wt, gmap, t_cout_pad)
    assert np.array_equal(wpt[pairs[:, 1]], ids.reshape(-1)) and (wpt >= 0).sum() == nw
    # the Winograd pack's layout: [plane][chunk32][cout_pad / 32][k8-step][32][8]
    if ks > 1:
        wi = words[7 + cin_pad + 2 * nw:].reshape(planes, cout_pad, cin_pad)
        assert planes == (16 if ks == 3 else 81)
        p, n, ci = np.meshgrid(np.arange(planes), np.arange(cout_pad), np.arange(cin_pad), indexing='ij')
        want = (((((p * (cin_pad // 32) + ci // 32) * (cout_pad // 32) + n // 32) * 4 + (ci % 32) // 8) * 32 + n % 32) * 8 + ci % 8)
        assert np.array_equal(wi, want)
        assert np.array_equal(np.sort(wi.reshape(-1)), np.arange(wi.size))          # a bijection onto the pack
    else:
        assert planes == 0 and len(words) == 7 + cin_pad + 2 * nw


@pytest.mark.parametrize('cout,cin,ks,kind', [(128, 128, 3, 0), (128, 185, 7, 1), (38, 512, 1, 0), (64, 3, 3, 0), (128, 199, 7, 2 + 71),
                                              (128, 150, 7, 2 + 22), (100, 20, 3, 0), (19, 128, 1, 0)])
def test_pack_values_against_numpy_packers(index_exe, tmp_path, cout, cin, ks, kind):
    """Every element of every pack, pads included, from the header's value functions on seeded weights == tests/pack_ref.py, bit for bit: the
    direct pack and bias, the transposed pack, the Winograd packs of both (float64, one rounding), conv1_1's fused-kernel pack, the f16
    pack and the bf16x3 pack; and the un-pack of the direct pack is the identity.  The weights carry pack_ref.edge_values() (+-0,
    subnormals, rounding ties of f16 and bf16, the f16 saturation edge, +-inf, a NaN) in real cells."""
    T = ks * ks
    rng = np.random.default_rng(cout * 1000 + cin + ks)
    W, edge_at = P.splice_edge_values(rng.normal(0, 0.05, (cout, cin, ks, ks)).astype('f'))
    b = rng.normal(0, 0.05, cout).astype('f')
    path = str(tmp_path / 'master.f32')
    np.concatenate([W.reshape(-1), b]).tofile(path)
    r = subprocess.run([index_exe, str(cout), str(cin), str(ks), str(kind), path, '16'], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    cp, cin_pad = P.cout_pad(cout), len(P.channel_map(kind, cin))
    words = 7 + cin_pad + 2 * cout * cin * T + (P.G.shape[0] ** 2 if ks == 3 else 81 if ks == 7 else 0) * cp * cin_pad
    want = P.layer_packs(W, b, kind)
    halves = 4 * want['w'].size          # the uint16 words that follow the floats: the f16 pack and the three planes of the bf16x3 pack
    got = np.frombuffer(r.stdout[8 * words:len(r.stdout) - 2 * halves], np.float32)
    got16 = np.frombuffer(r.stdout[len(r.stdout) - 2 * halves:], np.uint16)
    conv1 = (cout, cin, ks) == (64, 3, 3)          # ('wino' of that layer is its fused-kernel pack, emitted after the Winograd packs)
    assert ('wino' in want) == (conv1 or (ks > 1 and cin_pad % 32 == 0)) and ('t_wino' in want) == (ks > 1 and max(64, -(-cout // 16) * 16) % 32 == 0)
    assert want['wino'].size == 2 * 14 * 2 * 32 if conv1 else True
    order = ['w', 'b', 't_w', 't_wino', 'wino'] if conv1 else ['w', 'b', 't_w', 'wino', 't_wino']
    parts = [want[k] for k in order if k in want]
    parts += [W.reshape(-1), b]
    assert got.size == sum(x.size for x in parts)
    at = 0
    for i, x in enumerate(parts):
        assert x.dtype == np.float32 and np.array_equal(got[at:at + x.size].view(np.uint32), x.view(np.uint32)), (i, x.size)
        at += x.size
    # (the spliced +0 and -0 are the only zeros among the weights; every edge value sits in a real cell of the direct pack)
    assert (want['w'] != 0).sum() == W.size - 2
    assert sorted(_bits(W.reshape(-1)[edge_at])) == sorted(_bits(P.edge_values())) and np.isin(_bits(P.edge_values()), _bits(want['w'])).all()
    want16 = np.concatenate([P.f16_pack(want['w']), P.bf16x3_pack(want['w'], T, cin_pad // 16, cp)])
    assert want16.dtype == np.uint16 and got16.size == want16.size and np.array_equal(got16, want16), np.flatnonzero(got16 != want16)[:10]


def test_c_abi_surface():
    native = pkg('native')
    names = native.header_symbols()
    for e in ENTRIES:
        assert e in names, e
    srcs = dict(native.SOURCES)
    assert '-ffp-contract=off' in srcs['pmx_train.hip']
    assert '-ffp-contract=off' in srcs['pmx_packs.hip']          # (the Winograd transform's double multiplies and adds stay apart)
    assert 'pack_index.h' in native.HEADERS
