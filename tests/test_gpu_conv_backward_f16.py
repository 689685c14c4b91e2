"""GPU: pmx_conv2d_backward under option "grad_precision" = 2 (include/pose_mi355x.h) -- dw of a 3x3 / 7x7 layer from conv_wgrad_f16_kernel
(f16 operands, fp32 sums on v_mfma_f32_32x32x16_f16) and dx from the dispatcher's f16 form on the transposed pack.  The order inside one
MFMA's 16 products belongs to the hardware, so there is no bit-exact host twin for arbitrary inputs: on lattice inputs, where every
summation order is exact (tests/test_conv_backward_f16_host.py asserts the arithmetic), the device must EQUAL the emulation
(tests/f16_grad_emulation.py); on random inputs it must stay within a bound derived from the documented grouping and strip rule.  The masks
of the references are computed from the z the call returned (conv_bwd_ref.mask_rule), as in tests/test_gpu_conv_backward.py."""
import numpy as np
import pytest

import conv_bwd_ref as R
import f16_grad_emulation as G
from test_conv_backward_f16_host import EDGE_SHAPES, LATTICE_SHAPES
from test_gpu_conv_backward import SHAPES, _inputs, _reset

pytestmark = pytest.mark.gpu

F16_LAYER_TOL = 2e-5        # tests/test_gpu_f16.py::test_single_layer_matches_emulation: err <= 2e-5 * max(1, |ref|max)
INVALID, STATE = 1, 6

RANDOM_CASES = [(s, relu, pool) for s in SHAPES if s[0] > 1 for relu, pool in ((0, 0), (1, 0), (1, 1))
                if not pool or (s[3] % 2 == 0 and s[4] % 2 == 0)]


def _f16_grads(engine, x, w, b, dy, s0=0, **kw):
    """One call under grad_precision 2 (and s0 forced strips), the options reset whatever happens."""
    _reset(engine)
    engine.set_option('grad_precision', 2)
    engine.set_option('wgrad_strips', s0)
    try:
        return engine.conv2d_backward(x, w, b, dy, **kw)
    finally:
        engine.set_option('wgrad_strips', 0)
        engine.set_option('grad_precision', 0)


def test_the_option_takes_0_and_2_only(native, engine):
    x, w, b, dy = G.lattice_inputs(3, 20, 40, 9, 5, 2, seed=3)
    _reset(engine)
    x = x + np.float32(2.0 ** -12)          # not representable in f16: the two paths give different dw
    fp32 = engine.conv2d_backward(x, w, b, dy, want=('dw',))['dw']
    try:
        engine.set_option('grad_precision', 2)
        f16 = engine.conv2d_backward(x, w, b, dy, want=('dw',))['dw']
        assert not np.array_equal(f16, fp32)
        for bad in (1, 3, -1):
            with pytest.raises(native.PmxError) as e:
                engine.set_option('grad_precision', bad)
            assert e.value.code == INVALID and 'grad_precision' in str(e.value), (bad, str(e.value))
            assert np.array_equal(engine.conv2d_backward(x, w, b, dy, want=('dw',))['dw'], f16), bad      # the option is still 2
        engine.set_option('grad_precision', 0)
        with pytest.raises(native.PmxError):
            engine.set_option('grad_precision', 1)
        assert np.array_equal(engine.conv2d_backward(x, w, b, dy, want=('dw',))['dw'], fp32)              # ... and still 0
    finally:
        engine.set_option('grad_precision', 0)


@pytest.mark.parametrize('shape', LATTICE_SHAPES)
def test_integer_lattice_equals_the_emulation(engine, shape):
    """Zero tolerance: g integers in [-4, 4], x in [-8, 8], w in [-2, 2]; |sum| <= 32 * B * H * W <= 32 * 1104 < 2^24, any order is exact."""
    k, cin, cout, H, W, B, s0 = shape
    x, w, b, dy = G.lattice_inputs(k, cin, cout, H, W, B, seed=sum(shape))
    out = _f16_grads(engine, x, w, b, dy, s0)
    for name, a in out.items():
        assert np.isfinite(a).all(), 'unwritten (poisoned) or non-finite %s' % name
    dw, dx = G.dw_f16(dy, x, k), G.dx_f16(dy, w)
    assert np.array_equal(out['dw'], dw), (int((out['dw'] != dw).sum()), float(np.abs(out['dw'] - dw).max()))
    assert np.array_equal(out['dx'], dx), (int((out['dx'] != dx).sum()), float(np.abs(out['dx'] - dx).max()))
    assert np.array_equal(out['db'], R.db_rule(dy))


@pytest.mark.parametrize('shape', EDGE_SHAPES)
@pytest.mark.parametrize('kind,on', [('b', 'g'), ('b', 'x'), ('d', 'g'), ('d', 'x')])
def test_edge_lattice_pins_the_conversion_of_both_operands(engine, shape, kind, on):
    """Subnormal ties, 2^-25, its successor, -2^-26 ('b') and ties of normals ('d') in g or in x: the device's conversion is f16_rn_sat."""
    k, cin, cout, H, W, B, s0 = shape
    x, w, b, dy = G.edge_lattice_inputs(kind, on, k, cin, cout, H, W, B, seed=sum(shape))
    out = _f16_grads(engine, x, w, b, dy, s0, want=('dw', 'dx'))
    dw, dx = G.dw_f16(dy, x, k), G.dx_f16(dy, w)
    assert np.array_equal(out['dw'], dw), (int((out['dw'] != dw).sum()), float(np.abs(out['dw'] - dw).max()))
    assert np.array_equal(out['dx'], dx), (int((out['dx'] != dx).sum()), float(np.abs(out['dx'] - dx).max()))


def _clip_to_normal(a):
    """|a| >= 2^-14, the smallest f16 normal, signs kept: the operand-rounding bound (relative error 2^-11) is then rigorous."""
    tiny = np.float32(2.0 ** -14)
    return np.where(np.abs(a) < tiny, np.where(a < 0, -tiny, tiny), a).astype(np.float32)


@pytest.mark.parametrize('shape,relu,pool', RANDOM_CASES)
def test_random_inputs_within_the_derived_bounds(engine, shape, relu, pool):
    k, cin, cout, H, W, B, s0 = shape
    x, w, b, dy = _inputs(k, cin, cout, H, W, B, pool, seed=1300 + k + cin + 2 * relu + pool)
    x, dy = _clip_to_normal(x), _clip_to_normal(dy)
    out = _f16_grads(engine, x, w, b, dy, s0, relu=relu, pool=pool)
    for name, a in out.items():
        assert np.isfinite(a).all(), 'unwritten (poisoned) or non-finite %s' % name
    g = R.mask_rule(dy, out['z'], relu, pool)          # (a masked element is an exact zero: it rounds without error)
    Gm, S = G.mfmas_per_strip(B, H, W, cout, cin, k, s0)
    sum_bound = G.dw_sum_bound(g, x, k, 16 + Gm + S)
    err = np.abs(out['dw'].astype(np.float64) - G.dw64_of_rounded(g, x, k))
    dx_ref = G.dx_f16(g, w)
    edx, tol = float(np.abs(out['dx'] - dx_ref).max()), F16_LAYER_TOL * max(1.0, float(np.abs(dx_ref).max()))
    dw64 = R.conv_grads64(g, x, w)[1]
    err64, bound64 = np.abs(out['dw'].astype(np.float64) - dw64), G.operand_rounding_bound(g, x, k) + sum_bound
    print(shape, relu, pool, 'm', 16 + Gm + S, 'dw err / sum bound %.4f' % float((err / np.maximum(sum_bound, 1e-300)).max()),
          'dx err / tol %.4f' % (edx / tol), 'dw err / unrounded bound %.4f' % float((err64 / np.maximum(bound64, 1e-300)).max()))
    assert (err <= sum_bound).all()
    assert edx <= tol, (edx, tol)
    assert (err64 <= bound64).all()
    # negative control: the rounding of the operands is visible in dw, i.e. the f16 kernel ran
    assert (err64 > 64 * R.U * np.abs(dw64)).any()


def test_z_db_and_the_1x1_layers_do_not_depend_on_the_option(engine):
    for shape, relu, pool in (((3, 70, 64, 14, 10, 2, 0), 1, 1), ((7, 40, 128, 12, 15, 1, 0), 1, 0), ((1, 100, 38, 9, 13, 1, 0), 1, 0)):
        k, cin, cout, H, W, B, s0 = shape
        x, w, b, dy = _inputs(k, cin, cout, H, W, B, pool, seed=55 + k)
        _reset(engine)
        base = engine.conv2d_backward(x, w, b, dy, relu=relu, pool=pool)
        out = _f16_grads(engine, x, w, b, dy, relu=relu, pool=pool)
        assert np.array_equal(out['z'], base['z']) and np.array_equal(out['db'], base['db']), shape
        if k == 1:          # fp32, bit for bit, as the f16 inference mode leaves them
            assert np.array_equal(out['dw'], base['dw']) and np.array_equal(out['dx'], base['dx'])
        else:
            assert not np.array_equal(out['dw'], base['dw']) and not np.array_equal(out['dx'], base['dx']), shape


@pytest.mark.parametrize('k,cin,cout,H,W', [(3, 64, 64, 16, 24), (7, 32, 128, 12, 46)])
def test_same_bits_on_every_run_and_under_the_forward_options(engine, k, cin, cout, H, W):
    x, w, b, dy = _inputs(k, cin, cout, H, W, 2, False, seed=31 + k)
    base = _f16_grads(engine, x, w, b, dy)
    again = _f16_grads(engine, x, w, b, dy)
    assert np.array_equal(again['dw'], base['dw']) and np.array_equal(again['dx'], base['dx'])
    settings = [('conv_algo', 0, 1), ('conv_algo', 2, 1), ('ksplit', 2, 0), ('f16_bn', 64, 0), ('f16_bn', 128, 0)]
    _reset(engine)
    engine.set_option('grad_precision', 2)
    try:
        for key, val, default in settings:
            engine.set_option(key, val)
            out = engine.conv2d_backward(x, w, b, dy)
            engine.set_option(key, default)
            assert np.array_equal(out['dw'], base['dw']) and np.array_equal(out['db'], base['db']), (key, val)
            if key == 'f16_bn':
                assert np.array_equal(out['dx'], base['dx']), (key, val)
    finally:
        for key, val, default in settings:
            engine.set_option(key, default)
        engine.set_option('grad_precision', 0)


@pytest.mark.parametrize('k', [3, 7])
def test_non_finite_operands_stay_in_their_row_and_column(engine, k):
    """One NaN in x and one +inf in dy (relu = pool = 0), both at pixels no tap of which leaves the image.  The behaviour the header states:
    every sum of dw[:, ci0] holds the NaN and is NaN; f16() saturates, so the inf enters the sums of dw[co0] as 65504 -- still on the lattice
    (65504 * 8 + 32 * 180 < 2^24) -- and every element outside column ci0 EQUALS the emulation."""
    cin, cout, H, W, B = 20, 40, 9, 20, 1
    x, w, b, dy = G.lattice_inputs(k, cin, cout, H, W, B, seed=70 + k)
    ci0, co0 = 7, 33
    dy[0, co0, 4, 10] = np.inf
    emu = G.dw_f16(dy, x, k)          # (f16_round saturates as the device does)
    assert np.isfinite(emu).all() and np.abs(emu[co0]).max() > 65504 / 2
    x[0, ci0, 4, 9] = np.nan
    dw = _f16_grads(engine, x, w, b, dy, want=('dw',))['dw']
    assert np.isnan(dw[:, ci0]).all()
    rest = np.ones(dw.shape, bool)
    rest[:, ci0] = False
    assert np.array_equal(dw[rest], emu[rest])


def test_f16_mode_is_still_refused_with_the_option_set(native, engine):
    x, w, b, dy = _inputs(3, 16, 32, 8, 8, 1, False, seed=4)
    _reset(engine)
    want = _f16_grads(engine, x, w, b, dy)
    engine.set_option('grad_precision', 2)
    engine.set_option('precision', 2)
    try:
        with pytest.raises(native.PmxError) as e:
            engine.conv2d_backward(x, w, b, dy)
        assert e.value.code == STATE and 'precision' in str(e.value) and 'fp32 only' in str(e.value)
        engine.set_option('precision', 0)
        out = engine.conv2d_backward(x, w, b, dy)          # the context still runs
        for name in ('dx', 'dw', 'db', 'z'):
            assert np.array_equal(out[name], want[name]), name
    finally:
        engine.set_option('precision', 0)
        engine.set_option('grad_precision', 0)
