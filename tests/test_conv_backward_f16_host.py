"""CPU: the host side of the f16 gradients of one convolution layer (option "grad_precision" = 2; include/pose_mi355x.h:
pmx_conv2d_backward) -- the strip and group rule of csrc/wgrad_strips.h through a stand-alone program (tests/wgrad_f16_strips_main.c, host
compiler) against its restatement in tests/f16_grad_emulation.py, the emulation against float64 autograd on operands that f16 holds
exactly, and the arithmetic of the lattices the GPU tests use with zero tolerance."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import conv_bwd_ref as R
import f16_grad_emulation as G
from f16_emulation import f16_round

# (k, cin, cout, H, W, B, forced strips): the GPU file's lattice shapes
LATTICE_SHAPES = [(3, 5, 7, 1, 1, 3, 0), (3, 20, 40, 9, 1, 2, 0), (7, 33, 32, 1, 11, 1, 0), (7, 16, 32, 3, 2, 1, 0), (3, 32, 32, 46, 8, 3, 5),
                  (3, 32, 32, 46, 8, 3, 3), (3, 70, 64, 14, 17, 2, 0), (7, 185, 128, 6, 9, 2, 0), (3, 3, 64, 20, 24, 1, 0), (3, 512, 512, 4, 6, 1, 0),
                  (7, 40, 128, 12, 46, 1, 0)]
EDGE_SHAPES = [(3, 70, 64, 14, 17, 2, 0), (7, 40, 128, 12, 46, 1, 0)]


@pytest.fixture(scope='module')
def strips_exe(tmp_path_factory):
    cc = shutil.which('gcc') or shutil.which('cc')
    assert cc, 'no host C compiler'
    exe = os.path.join(str(tmp_path_factory.mktemp('wgrad_f16_strips')), 'wgrad_f16_strips_main')
    r = subprocess.run([cc, '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', R.CSRC,
                        '-I', os.path.join(R.ROOT, 'include'), os.path.join(R.HERE, 'wgrad_f16_strips_main.c'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _program(exe, B, H, W, cout, cin, ks, forced):
    r = subprocess.run([exe] + [str(v) for v in (B, H, W, cout, cin, ks, forced)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    first, second = (ln.split() for ln in r.stdout.splitlines())
    assert second[0] == 'fp32'
    return tuple(int(v) for v in first), tuple(int(v) for v in second[1:])


# the lattice shapes, the six rows of the measurement (EXPERIMENTS E54) and forced counts past the cap and past the rows
RULE_CASES = LATTICE_SHAPES + [(3, 512, 512, 46, 46, 8, 0), (3, 512, 512, 46, 46, 32, 0), (7, 128, 128, 46, 46, 8, 0), (7, 128, 128, 46, 46, 32, 0),
                               (7, 185, 128, 46, 46, 8, 0), (7, 185, 128, 46, 46, 32, 0), (3, 64, 64, 368, 368, 2, 100), (7, 32, 32, 2, 40, 1, 7)]


@pytest.mark.parametrize('shape', RULE_CASES)
def test_strip_and_group_rule_restated_equals_the_library_s(strips_exe, shape):
    k, cin, cout, H, W, B, forced = shape
    (blocks, strips, rows, groups), fp32 = _program(strips_exe, B, H, W, cout, cin, k, forced)
    assert blocks == G.blocks(cout, cin, k)
    assert (strips, rows) == G.strips_for(B, H, cout, cin, k, forced)
    assert groups == G.groups(W) == -(-W // 16)
    assert (strips - 1) * rows < B * H <= strips * rows and strips <= G.MAX_STRIPS          # the strips cover the rows, none is empty
    assert G.mfmas_per_strip(B, H, W, cout, cin, k, forced) == (rows * groups, strips)
    assert fp32 == R.strips_for(B, H, cout, cin, k, forced)                               # the fp32 rule has not moved


def test_forced_strips_fall_where_the_gpu_tests_say():
    assert G.strips_for(3, 46, 32, 32, 3, 5) == (5, 28)          # borders at rows 28 / 56 / 84 / 112: inside images
    assert G.strips_for(3, 46, 32, 32, 3, 3) == (3, 46)          # borders at image borders


@pytest.mark.parametrize('shape', [(3, 20, 40, 9, 5, 2), (7, 33, 32, 4, 11, 1)])
def test_emulation_of_representable_inputs_equals_float64_autograd(shape):
    """Operands that f16 holds exactly are not changed by the rounding: dw_f16 and dx_f16 are the float64 gradients, rounded once."""
    k, cin, cout, H, W, B = shape
    rng = np.random.default_rng(k + cin)
    x, g = (rng.standard_normal(s).astype(np.float16).astype(np.float32) for s in ((B, cin, H, W), (B, cout, H, W)))
    w = rng.standard_normal((cout, cin, k, k)).astype(np.float16).astype(np.float32)
    assert np.array_equal(f16_round(x), x) and np.array_equal(f16_round(g), g)
    dx64, dw64, _ = R.conv_grads64(g, x, w)
    assert np.array_equal(G.dw_f16(g, x, k), dw64.astype(np.float32))
    assert np.array_equal(G.dx_f16(g, w), dx64.astype(np.float32))
    # and unrounded operands ARE changed: the emulation is not the plain gradient
    x2 = rng.standard_normal(x.shape).astype(np.float32)
    assert not np.array_equal(G.dw_f16(g, x2, k), R.conv_grads64(g, x2, w)[1].astype(np.float32))


def _exact(name, a64, unit, sum_abs):
    """Every value a multiple of `unit`, every partial sum of every order below 2^24 units: representable in fp32, no addition rounds."""
    q = a64 / unit
    assert np.array_equal(q, np.rint(q)), name
    assert sum_abs.max() < 2.0 ** 24 * unit, (name, float(sum_abs.max()), unit)
    assert np.array_equal(a64.astype(np.float32).astype(np.float64), a64), name


@pytest.mark.parametrize('shape', LATTICE_SHAPES)
def test_integer_lattice_is_exact_in_every_order(shape):
    k, cin, cout, H, W, B, _ = shape
    x, w, b, dy = G.lattice_inputs(k, cin, cout, H, W, B, seed=sum(shape))
    assert np.array_equal(f16_round(x), x) and np.array_equal(f16_round(dy), dy) and np.array_equal(f16_round(w), w)
    assert 32 * B * H * W <= 32 * 1104 < 2 ** 24
    _exact('dw', G.dw64_of_rounded(dy, x, k), 1.0, G.abs_products(dy, x, k))
    dx64, dw64, _ = R.conv_grads64(dy, x, w)
    assert np.array_equal(G.dw_f16(dy, x, k), dw64.astype(np.float32))
    _exact('dx', dx64, 1.0, R.conv_grads64(np.abs(dy), x, np.abs(w))[0])
    assert np.array_equal(G.dx_f16(dy, w), dx64.astype(np.float32))


@pytest.mark.parametrize('shape', EDGE_SHAPES)
@pytest.mark.parametrize('kind,on', [('b', 'g'), ('b', 'x'), ('d', 'g'), ('d', 'x')])
def test_edge_lattice_is_exact_in_every_order(shape, kind, on):
    k, cin, cout, H, W, B, _ = shape
    x, w, b, dy = G.edge_lattice_inputs(kind, on, k, cin, cout, H, W, B, seed=sum(shape))
    edge = dy if on == 'g' else x
    assert not np.array_equal(f16_round(edge), edge)          # the conversion has something to do
    if kind == 'b':
        assert (np.abs(edge) == np.float32(2.0 ** -25)).sum() >= 4 and (edge == np.float32(-2.0 ** -26)).sum() == 4
    unit_dw = 2.0 ** -16 if kind == 'b' else 2.0 ** -10
    _exact('dw', G.dw64_of_rounded(dy, x, k), unit_dw, G.abs_products(dy, x, k))
    unit_dx = {('b', 'g'): 2.0 ** -24, ('b', 'x'): 2.0 ** 8, ('d', 'g'): 2.0 ** -10, ('d', 'x'): 1.0}[(kind, on)]
    dx64 = R.conv_grads64(f16_round(dy), x, w)[0]
    _exact('dx', dx64, unit_dx, R.conv_grads64(np.abs(f16_round(dy)), x, np.abs(w))[0])
    assert np.array_equal(G.dx_f16(dy, w), dx64.astype(np.float32))
