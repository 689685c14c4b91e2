"""GPU: pmx_conv2d_backward (include/pose_mi355x.h) on the integer lattice of tests/conv_bwd_ref.py, where every fp32 summation order gives
the same bits.  All four outputs are compared for EQUALITY with torch-CPU float64 autograd of the whole chain conv2d -> relu -> max_pool2d
(conv_bwd_ref.autograd64; neither mask_rule nor the order twin takes part), on inputs that hold pooling windows with equal maxima, exact
zeros of z and windows with nothing above zero by the hundred (conv_bwd_ref.lattice_census; the floors are asserted before anything is
compared, and tests/test_conv_backward_host.py pins torch's behaviour on them to the stated rule).  So conv_bwd_mask_kernel's first-of-equal-
maxima choice and its strict z > 0 gate are checked on the device, on the z of every forward plan.  The data gradient alone at the width of
the trunk's last layers (256 and 512 channels on maps with partial Winograd tiles), under every conv_algo, for the same equality."""
import numpy as np
import pytest

import conv_bwd_ref as R

pytestmark = pytest.mark.gpu

CASES = [(s, relu, pool) for s in R.LATTICE_TIE_SHAPES for relu, pool in R.LATTICE_VARIANTS]


def _reset(engine):
    for kk in (1, 3, 7):
        engine.set_option('force_variant_k%d' % kk, -1)
    engine.set_option('wgrad_strips', 0)


def _assert_exact(out, ref, what):
    """z first: if it differs, the lattice premise failed under this plan (a forward form that is not exact on these inputs) and nothing can
    be said about the mask; then the three gradients."""
    for name, a in out.items():
        assert a.shape == ref[name].shape and np.isfinite(a).all(), 'unwritten (poisoned) or non-finite %s: %r' % (name, what)
    bad = int((out['z'] != ref['z']).sum())
    assert bad == 0, 'the lattice premise failed, not the mask: z is not exact in %d elements (max |diff| %g): %r' % (
        bad, np.abs(out['z'] - ref['z']).max(), what)
    for name in ('dx', 'dw', 'db'):
        ne = out[name] != ref[name]
        assert not ne.any(), '%s differs from float64 autograd in %d elements, first at %r: %r' % (name, int(ne.sum()), tuple(np.argwhere(ne)[0]), what)


def _floors(census):
    assert min(census.values()) >= R.LATTICE_FLOOR, census


@pytest.mark.parametrize('shape,relu,pool', CASES)
def test_ties_and_zeros_follow_chainers_rule(engine, shape, relu, pool):
    x, w, b, dy, ref, census = R.lattice_case(shape, relu, pool)
    _floors(census)
    _reset(engine)
    out = engine.conv2d_backward(x, w, b, dy, relu=relu, pool=pool)
    print(shape, relu, pool, census, 'max |z|', np.abs(ref['z']).max(), 'max |dw|', np.abs(ref['dw']).max())
    _assert_exact(out, ref, (shape, relu, pool))


@pytest.mark.parametrize('relu,pool', R.LATTICE_VARIANTS)
def test_identity_weights_show_the_masked_gradient_element_for_element(engine, relu, pool):
    """w = I (1x1): dx is g, the mask kernel's own output -- the chosen position inside windows of equal values included -- and it is +0.0,
    by bit pattern, wherever the gate is closed (dy has no zero, so dx is zero exactly there).  The data gradient's accumulators start at
    +0.0, which would absorb a -0.0 of g: the bit check sees dx, the value checks see g."""
    x, w, b, dy, ref, census = R.lattice_case(R.LATTICE_IDENTITY, relu, pool, identity=True)
    assert min(census.values()) >= 1, census
    _reset(engine)
    out = engine.conv2d_backward(x, w, b, dy, relu=relu, pool=pool)
    _assert_exact(out, ref, ('identity', relu, pool))
    closed = ref['dx'] == 0
    assert closed.sum() >= R.LATTICE_FLOOR
    assert (out['dx'].view(np.uint32)[closed] == 0).all(), 'a closed gate holds -0.0'


@pytest.mark.parametrize('shape', R.LATTICE_SWEEP_SHAPES)
def test_mask_reads_the_z_of_every_plan(engine, shape):
    """The settings and forced variants of test_gpu_conv_backward.py::test_dw_and_db_keep_their_bits_under_the_forward_options at its two
    shapes, with ReLU and pool ON: the mask kernel runs on the z that a Winograd, a split-K or a forced-variant plan wrote, and all four
    outputs equal float64 autograd under every setting -- and so each other.  The plans of pmx_conv2d_backward carry no profile label, so the
    per-launch profiler does not see which kernel ran.  By the selection rules (csrc/conv_select.hip::wino_eligible: 128 padded output
    channels) the 3x3 / 64 -> 64 shape has no Winograd form and the 7x7 shape has one for z only; the third shape, 3x3 / 128 -> 128, has one
    for z and for the data gradient."""
    k = shape[0]
    x, w, b, dy, ref, census = R.lattice_case(shape, 1, 1)
    _floors(census)
    _reset(engine)
    _assert_exact(engine.conv2d_backward(x, w, b, dy, relu=True, pool=True), ref, 'defaults')
    settings = [('conv_algo', 0, 1), ('conv_algo', 2, 1), ('wino_tail', 1, -1), ('wino_geom', 0, -1), ('ksplit', 2, 0)]
    try:
        for key, val, default in settings:
            engine.set_option('conv_algo', 2 if key.startswith('wino') else 1)
            engine.set_option(key, val)
            out = engine.conv2d_backward(x, w, b, dy, relu=True, pool=True)
            engine.set_option(key, default)
            _assert_exact(out, ref, (key, val))
        engine.set_option('conv_algo', 1)
        for variant in {3: (2, 6, 14, 16), 7: (0, 5, 12, 15, 17, 21)}[k]:          # (conv_mfma.hip g_variants; one that does not fit a plan is not taken)
            engine.set_option('force_variant_k%d' % k, variant)
            _assert_exact(engine.conv2d_backward(x, w, b, dy, relu=True, pool=True), ref, ('force_variant', variant))
    finally:
        for key, val, default in settings:
            engine.set_option(key, default)
        _reset(engine)


@pytest.mark.parametrize('algo', (0, 1, 2))
@pytest.mark.parametrize('shape', list(R.LATTICE_WIDE))
def test_wide_data_gradients_are_exact_in_every_form(engine, shape, algo):
    """dx of the transposed layers of conv4_1 (512 -> 256 at 6 x 10) and conv4_2 (512 -> 512 at 5 x 7, batch 3), dense lattice weights, no
    relu, no pool: direct, split-K and Winograd launches give the bits of float64 autograd (|dx| <= 2 * 512 * 9 < 2^22; the cast is checked
    in tests/test_conv_backward_host.py)."""
    x, w, dy, dx = R.lattice_wide_case(shape)
    _reset(engine)
    engine.set_option('conv_algo', algo)
    try:
        out = engine.conv2d_backward(x, w, None, dy, want=('dx',))
    finally:
        engine.set_option('conv_algo', 1)
    assert set(out) == {'dx'} and out['dx'].shape == dx.shape and np.isfinite(out['dx']).all()
    ne = out['dx'] != dx
    print(shape, algo, 'dx != float64 autograd', int(ne.sum()), 'max |dx|', np.abs(dx).max())
    assert not ne.any(), 'dx differs from float64 autograd in %d elements, first at %r' % (int(ne.sum()), tuple(np.argwhere(ne)[0]))


def test_lattice_under_forced_strips(engine):
    """On the lattice -- and only there -- the weight gradient does not depend on how the rows are cut into strips: 1, 3 (every border an
    image border), 5 (borders inside images) and 32 strips give the same dw, float64 autograd's."""
    shape = (3, 32, 32, 46, 8, 3)
    x, w, b, dy, ref, census = R.lattice_case(shape, 1, 1)
    _floors(census)
    _reset(engine)
    try:
        for strips in (1, 3, 5, 32):
            engine.set_option('wgrad_strips', strips)
            _assert_exact(engine.conv2d_backward(x, w, b, dy, relu=True, pool=True), ref, ('wgrad_strips', strips))
    finally:
        engine.set_option('wgrad_strips', 0)
