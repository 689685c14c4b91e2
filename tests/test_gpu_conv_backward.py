"""GPU: pmx_conv2d_backward (include/pose_mi355x.h) -- the gradients of one convolution layer through the C ABI.  z against the torch
reference of pmx_conv2d's own test, dw bit for bit against the order-defined host twin (tests/conv_wgrad_twin.c) and within the bound of a
float32 sum of products against float64 autograd, db and dx against float64 autograd, dx also by its error over that of torch's float32
data gradient for the same g (conv_bwd_ref.ratio, at most MARGIN; figures: EXPERIMENTS.md E40).  The masks of the references are computed from the z
the call returned (tests/conv_bwd_ref.py::mask_rule), so no element is left out for a near-tie."""
import numpy as np
import pytest

import conv_bwd_ref as R
from oracle import network_ref as N

pytestmark = pytest.mark.gpu

TOL = 2e-5          # tests/test_gpu_conv.py: err <= TOL * max(1, |ref|max)
MARGIN = R.MARGIN

# (k, cin, cout, H, W, B, forced strips)
SHAPES = [(7, 40, 128, 12, 15, 1, 0), (3, 70, 64, 14, 10, 2, 0), (1, 100, 38, 9, 13, 1, 0), (3, 3, 64, 20, 24, 1, 0),
          (7, 185, 128, 6, 9, 2, 0), (1, 128, 19, 8, 6, 1, 0), (7, 16, 32, 3, 2, 1, 0),
          (3, 32, 32, 46, 8, 3, 5),          # 138 rows in 5 strips of 28: borders inside images (28, 56, 84, 112) -- and with 3 strips at 46, 92
          # the network's channel extremes (512 -> 512 3x3, 128 -> 512 and 512 -> 38 1x1) on the smallest maps; 1x1 with six ci tiles, the
          # second group of four half empty; maps one pixel wide or high (W = 1: the half-wave's column wraps twice on every step), a map of
          # one pixel; 21 one-pixel rows in 2 strips of 11: the border falls inside the second image
          (3, 512, 512, 4, 6, 1, 0), (1, 128, 512, 6, 4, 2, 0), (1, 512, 38, 6, 4, 1, 0), (1, 185, 19, 5, 7, 1, 0),
          (3, 20, 40, 9, 1, 2, 0), (7, 33, 32, 1, 11, 1, 0), (3, 5, 7, 1, 1, 3, 0), (3, 32, 32, 7, 1, 3, 2)]
CASES = [(s, relu, pool) for s in SHAPES for relu, pool in ((0, 0), (1, 0), (1, 1)) if not pool or (s[3] % 2 == 0 and s[4] % 2 == 0)]


def _inputs(k, cin, cout, H, W, B, pool, seed):
    rng = np.random.default_rng(seed)          # the inputs of tests/test_gpu_conv.py::_case, plus dy
    x = rng.standard_normal((B, cin, H, W)).astype('f')
    w = (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype('f')
    b = rng.standard_normal(cout).astype('f')
    dy = rng.standard_normal((B, cout, H // 2 if pool else H, W // 2 if pool else W)).astype('f')
    return x, w, b, dy


def _reset(engine):
    for kk in (1, 3, 7):
        engine.set_option('force_variant_k%d' % kk, -1)
    engine.set_option('wgrad_strips', 0)


def _check(engine, shape, relu, pool, out, x, w, b, dy):
    k, cin, cout, H, W, B, s0 = shape
    for name, a in out.items():
        assert np.isfinite(a).all(), 'unwritten (poisoned) or non-finite %s' % name
    z = out['z']
    zref = N.conv2d_ref(x, w, b, relu=False, pool=False)
    ez = np.abs(z - zref).max()
    g = R.mask_rule(dy, z, relu, pool)
    dx64, dw64, db64 = R.conv_grads64(g, x, w)
    twin = R.wgrad_twin(g, x, k, s0)
    err = np.abs(out['dw'].astype(np.float64) - dw64)
    bound = R.dw_bound(g, x, w, dw64)
    edb = np.abs(out['db'].astype(np.float64) - db64)
    edx = np.abs(out['dx'] - dx64).max()
    rdx = R.ratio(out['dx'], dx64, R.dx_pair(g, w)[1])
    print(shape, relu, pool, 'z', ez, 'dw != twin', int((out['dw'] != twin).sum()), 'dw err / bound', float((err / np.maximum(bound, 1e-300)).max()),
          'db', float((edb / np.maximum(np.abs(db64), 1e-300)).max()), 'dx', edx, np.abs(dx64).max(), 'dx r_l2 %.3f r_max %.3f rel. L2 %.3e' % rdx)
    assert ez <= TOL * max(1.0, np.abs(zref).max())
    assert np.array_equal(out['dw'], twin), (int((out['dw'] != twin).sum()), np.abs(out['dw'] - twin).max())
    assert (err <= bound).all()
    assert (edb <= 2.0 ** -23 * np.abs(db64)).all()
    assert edx <= TOL * max(1.0, np.abs(dx64).max())
    assert rdx[0] <= MARGIN and rdx[1] <= MARGIN, rdx


@pytest.mark.parametrize('shape,relu,pool', CASES)
def test_gradients_of_one_layer(engine, shape, relu, pool):
    k, cin, cout, H, W, B, s0 = shape
    x, w, b, dy = _inputs(k, cin, cout, H, W, B, pool, seed=1300 + k + cin + 2 * relu + pool)
    _reset(engine)
    engine.set_option('wgrad_strips', s0)
    try:
        out = engine.conv2d_backward(x, w, b, dy, relu=relu, pool=pool)
    finally:
        engine.set_option('wgrad_strips', 0)
    assert out['dx'].shape == x.shape and out['dw'].shape == w.shape and out['db'].shape == (cout,) and out['z'].shape == (B, cout, H, W)
    _check(engine, shape, relu, pool, out, x, w, b, dy)


def test_strips_that_end_at_image_borders(engine):
    shape = (3, 32, 32, 46, 8, 3, 3)          # 3 strips of 46 rows: every border is an image border
    x, w, b, dy = _inputs(3, 32, 32, 46, 8, 3, True, seed=77)
    _reset(engine)
    engine.set_option('wgrad_strips', 3)
    try:
        out = engine.conv2d_backward(x, w, b, dy, relu=True, pool=True)
    finally:
        engine.set_option('wgrad_strips', 0)
    _check(engine, shape, 1, 1, out, x, w, b, dy)


def test_same_bits_on_every_run(engine):
    x, w, b, dy = _inputs(7, 40, 128, 12, 15, 2, False, seed=5)
    _reset(engine)
    a = engine.conv2d_backward(x, w, b, dy, relu=True)
    c = engine.conv2d_backward(x, w, b, dy, relu=True)
    for name in ('dx', 'dw', 'db', 'z'):
        assert np.array_equal(a[name], c[name]), name


@pytest.mark.parametrize('k,cin,cout,H,W', [(3, 64, 64, 16, 24), (7, 32, 128, 12, 46)])
def test_dw_and_db_keep_their_bits_under_the_forward_options(engine, k, cin, cout, H, W):
    """The kernel form of z and dx follows the options; the weight and bias gradients do not (for the same g: relu and pool off)."""
    x, w, b, dy = _inputs(k, cin, cout, H, W, 2, False, seed=31 + k)
    _reset(engine)
    base = engine.conv2d_backward(x, w, b, dy)
    dx64, dx32 = R.dx_pair(dy, w)
    settings = [('conv_algo', 0, 1), ('conv_algo', 2, 1), ('wino_tail', 1, -1), ('wino_geom', 0, -1), ('ksplit', 2, 0)]
    try:
        for key, val, default in settings:
            engine.set_option('conv_algo', 2 if key.startswith('wino') else 1)
            engine.set_option(key, val)
            out = engine.conv2d_backward(x, w, b, dy)
            engine.set_option(key, default)
            assert np.array_equal(out['dw'], base['dw']) and np.array_equal(out['db'], base['db']), (key, val)
            assert np.abs(out['dx'] - dx64).max() <= TOL * max(1.0, np.abs(dx64).max()), (key, val)
            rdx = R.ratio(out['dx'], dx64, dx32)
            print(k, key, val, 'dx r_l2 %.3f r_max %.3f rel. L2 %.3e' % rdx)
            assert rdx[0] <= MARGIN and rdx[1] <= MARGIN, (key, val, rdx)
        engine.set_option('conv_algo', 1)
        for variant in {3: (2, 6, 14, 16), 7: (0, 5, 12, 15, 17, 21)}[k]:          # (conv_mfma.hip g_variants; one that does not fit a plan is not taken)
            engine.set_option('force_variant_k%d' % k, variant)
            out = engine.conv2d_backward(x, w, b, dy)
            assert np.array_equal(out['dw'], base['dw']) and np.array_equal(out['db'], base['db']), variant
    finally:
        for key, val, default in settings:
            engine.set_option(key, default)
        _reset(engine)


def test_null_outputs_are_skipped_and_dx_passes_through(engine):
    x, w, b, dy = _inputs(3, 70, 64, 14, 10, 2, True, seed=9)
    _reset(engine)
    full = engine.conv2d_backward(x, w, b, dy, relu=True, pool=True)
    for want in (('dx',), ('dw',), ('db',), ('z',), ('dx', 'db'), ('dw', 'z')):
        out = engine.conv2d_backward(x, w, b, dy, relu=True, pool=True, want=want)
        assert set(out) == set(want)
        for name in want:
            assert np.array_equal(out[name], full[name]), (want, name)
    out = engine.conv2d_backward(x, w, None, dy[:, :, :1, :1].repeat(14, 2).repeat(10, 3), want=('dx',))          # no bias, no z needed
    assert np.isfinite(out['dx']).all()


def test_timing_of_the_three_parts(engine):
    x, w, b, dy = _inputs(3, 32, 32, 16, 16, 1, False, seed=2)
    _reset(engine)
    out = engine.conv2d_backward(x, w, b, dy, relu=True, iters=2)
    assert len(out['ms']) == 3 and all(m > 0 for m in out['ms'])
    out = engine.conv2d_backward(x, w, b, dy, relu=True, iters=2, want=('dw',))
    assert out['ms'][0] == 0 and out['ms'][1] > 0 and out['ms'][2] > 0


def _rc(native, engine, *args):
    rc = engine.lib.pmx_conv2d_backward(engine._ctx, *args)
    return rc, engine.lib.pmx_last_error().decode()


def test_error_codes_and_messages(native, engine):
    from ctypes import c_double
    x, w, b, dy = _inputs(3, 4, 5, 6, 8, 1, False, seed=1)
    dx, dw, db, z = np.empty_like(x), np.empty_like(w), np.empty(5, 'f'), np.empty((1, 5, 6, 8), 'f')
    p = lambda a: None if a is None else a.ctypes.data
    ms = (c_double * 3)()
    INVALID, STATE = 1, 6

    def call(x_=x, w_=w, dy_=dy, shape=(1, 4, 6, 8, 5, 3), relu=0, pool=0, outs=(dx, dw, db, z)):
        B, cin, H, W, cout, k = shape
        return _rc(native, engine, p(x_), p(w_), p(b), p(dy_), B, cin, H, W, cout, k, relu, pool, p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), 0, ms)
    _reset(engine)
    assert call()[0] == 0
    for kw in (dict(x_=None), dict(w_=None), dict(dy_=None)):
        rc, msg = call(**kw)
        assert rc == INVALID and 'null' in msg, (kw, rc, msg)
    rc, msg = call(outs=(None, None, None, None))
    assert rc == INVALID and 'all four outputs' in msg
    for k in (0, 2, 5, 9):
        rc, msg = call(shape=(1, 4, 6, 8, 5, k))
        assert rc == INVALID and 'ksize' in msg
    for shape in ((0, 4, 6, 8, 5, 3), (1, 0, 6, 8, 5, 3), (1, 4, 0, 8, 5, 3), (1, 4, 6, -1, 5, 3), (1, 4, 6, 8, 0, 3)):
        rc, msg = call(shape=shape)
        assert rc == INVALID and 'shape' in msg, shape
    for shape in ((1, 4, 5, 8, 5, 3), (1, 4, 6, 7, 5, 3)):
        rc, msg = call(shape=shape, pool=1)
        assert rc == INVALID and 'even' in msg, shape
    assert call()[0] == 0          # the context stays usable


def test_f16_mode_is_refused_and_the_context_still_runs(native, engine):
    x, w, b, dy = _inputs(3, 16, 32, 8, 8, 1, False, seed=4)
    _reset(engine)
    want = engine.conv2d(x, w, b, relu=True)
    engine.set_option('precision', 2)
    try:
        with pytest.raises(native.PmxError) as e:
            engine.conv2d_backward(x, w, b, dy)
        assert e.value.code == 6 and 'precision' in str(e.value) and 'fp32 only' in str(e.value)
    finally:
        engine.set_option('precision', 0)
    assert np.array_equal(engine.conv2d(x, w, b, relu=True), want)
    assert np.isfinite(engine.conv2d_backward(x, w, b, dy)['dw']).all()
