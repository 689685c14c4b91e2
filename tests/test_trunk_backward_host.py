"""CPU: the host side of the trunk backward (include/pose_mi355x.h: pmx_backward_trunk) -- the C ABI surface, the strip rules of
csrc/wgrad_strips.h through a stand-alone program (tests/trunk_strips_main.c, host compiler) against their restatement in Python, the
2048 waves the rules promise at the training shapes, the NumPy twin of the pooled layers against float64 autograd on the lattice, and its scatter in the dtype of the gradient."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import conv_bwd_ref as R
import trunk_backward_ref as T
from conftest import pkg

ENTRIES = ['pmx_backward_trunk', 'pmx_conv1_wgrad', 'pmx_pool_backward_test']
SHAPES = [(2, 64, 48), (10, 368, 368), (32, 368, 368)]


def test_trunk_entries_declared_exported_and_bound(native):
    syms = native.header_symbols()
    lib = native.load()
    for e in ENTRIES:
        assert e in syms and hasattr(lib, e) and e in lib._pmx_sig, e
    assert [len(lib._pmx_sig[e][1]) for e in ENTRIES] == [1, 10, 9]
    for m in ('backward_trunk', 'conv1_wgrad', 'pool_backward_test'):
        assert callable(getattr(native.Engine, m)), m
    assert callable(pkg('pose_detector').PoseDetector.network_gradients)
    hdr = open(native.HEADER).read()
    assert hdr.count('#define PMX_WGRAD_TRUNK_MAX_STRIPS %d\n' % T.TRUNK_MAX_STRIPS) == 1
    assert hdr.count('#define PMX_WGRAD_CONV1_STRIPS %d\n' % T.CONV1_STRIPS) == 1
    assert hdr.count('#define PMX_WGRAD_MAX_STRIPS 32\n') == 1
    assert tuple(T.NAMES) == native.Engine.TRUNK_LAYERS and tuple(T.POOLED) == native.Engine.POOLED_LAYERS
    table = {n: (cin, cout, k) for n, cin, cout, k in pkg('weights').layer_table()}
    for name, cin, cout, level, _ in T.TRUNK:
        assert table[name] == (cin, cout, 3) and native.Engine.TRUNK_LEVEL[name] == level, name


@pytest.fixture(scope='module')
def strips_exe(tmp_path_factory):
    cc = shutil.which('gcc') or shutil.which('cc')
    assert cc, 'no host C compiler'
    exe = os.path.join(str(tmp_path_factory.mktemp('trunk_strips')), 'trunk_strips_main')
    r = subprocess.run([cc, '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', R.CSRC,
                        '-I', os.path.join(R.ROOT, 'include'), os.path.join(R.HERE, 'trunk_strips_main.c'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _program(exe, B, H, forced):
    r = subprocess.run([exe, str(B), str(H), str(forced)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert [w[0] for w in rows] == T.NAMES + ['head']
    return {w[0]: tuple(int(v) for v in w[1:]) for w in rows}


@pytest.mark.parametrize('B,H,W', SHAPES)
@pytest.mark.parametrize('forced', [0, 3, 5])
def test_strip_rules_restated_equal_the_library_s(strips_exe, B, H, W, forced):
    got = _program(strips_exe, B, H, forced)
    for name, cin, cout, level, _ in T.TRUNK:
        s, r, waves = T.trunk_strips(name, B, H, forced)
        assert got[name] == (s, r, waves), (name, got[name], (s, r, waves))
        total = B * (H >> level)
        assert (s - 1) * r < total <= s * r, name                      # the strips cover the rows, none is empty
        if forced:
            assert forced <= s < 2 * forced, (name, s)
    assert got['head'] == R.strips_for(B, H // 8, 128, 128, 7, forced)          # the head's rule has not moved


@pytest.mark.parametrize('B,H,W', SHAPES[1:])
def test_every_trunk_layer_gets_its_2048_waves(strips_exe, B, H, W):
    """The condition the trunk cap exists for (2048 waves = 256 CUs x 4 SIMDs x 2), by arithmetic, from the library's own rule."""
    got = _program(strips_exe, B, H, 0)
    for name in T.NAMES:
        s, r, waves = got[name]
        assert waves >= T.WAVES, (name, s, r, waves)
        assert waves == T.trunk_strips(name, B, H)[2]
    # pmx_conv2d_backward's cap of 32 strips is what left these layers short
    assert [32 * T.units(cin, cout) for _, cin, cout, _, _ in T.TRUNK[1:4]] == [192, 384, 768]
    # the workspace of the widest weight gradient
    ws = max(got[n][0] * 9 * cin * cout * 4 for n, cin, cout, _, _ in T.TRUNK[1:])
    assert ws < 2 * 57e6, ws          # (S < 2 S0, and S0 strips of any of these layers stay below 57 MB)


@pytest.mark.parametrize('C_,H,W', [(32, 2, 2), (64, 6, 10), (96, 16, 12)])
def test_pool_twin_equals_float64_autograd_on_the_lattice(C_, H, W):
    """pool_twin reads the gate and the argmax from a = relu(z) alone; torch float64 autograd of max_pool2d(relu(z)) is the reference."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(100 + C_)
    z = rng.integers(-2, 3, (2, C_, H, W)).astype('f')
    u = rng.choice(np.array([-2, -1, 1, 2], 'f'), (2, C_, H // 2, W // 2))
    census = R.lattice_census(z, u, 1, 1)
    zt = torch.tensor(z.astype(np.float64), requires_grad=True)
    y = F.max_pool2d(F.relu(zt), 2, 2)
    y.backward(torch.tensor(u.astype(np.float64)))
    pooled, g = T.pool_twin(np.maximum(z, np.float32(0)), u)
    assert np.array_equal(pooled.astype(np.float64), y.detach().numpy())
    assert np.array_equal(g.astype(np.float64), zt.grad.numpy()), census
    assert np.array_equal(g, R.mask_rule(u, z, 1, 1))
    assert census['tied'] and census['dead_windows'] and census['zeros'], census


@pytest.mark.parametrize('C_,H,W', [(32, 2, 2), (64, 6, 10), (96, 16, 12)])
def test_pool_scatter_is_pool_twin_s_scatter_in_the_dtype_of_u(C_, H, W):
    rng = np.random.default_rng(200 + C_)
    a = np.maximum(rng.integers(-2, 3, (2, C_, H, W)), 0).astype('f')          # ties and dead windows in plenty
    u = rng.standard_normal((2, C_, H // 2, W // 2))
    want = T.pool_twin(a, u.astype('f'))[1]
    g32 = T.pool_scatter(a, u.astype('f'))
    assert g32.dtype == np.float32 and np.array_equal(g32.view(np.uint32), want.view(np.uint32))
    g64 = T.pool_scatter(a, u)
    assert g64.dtype == np.float64 and np.array_equal(g64 != 0, want != 0) 
    live = T.windows(g64 != 0).any(axis=-1)
    assert np.array_equal(T.windows(g64).sum(axis=-1), np.where(live, u, 0.0))          # one non-zero per window: u itself, not rounded
    assert not np.signbit(g64[g64 == 0]).any()
