"""GPU: the opt-in bf16x3 mode ("precision" = 1): 3x3 / 7x7 layers of large batches on the bf16 matrix cores, every fp32 value
split into three bf16 terms (hi + mid + lo), six products, fp32 accumulation.  It is NOT the fp32 FMA chain of the default
path (no bit-exact oracle); the bar is fp32-GRADE accuracy: each convolution as close to a float64 reference as the fp32
path is (within a small factor), whole-network maps within 1e-4 of the reference goldens, and the detector's results on the
reference's own images unchanged."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, pkg
from test_reference_network import load_e2e

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _needs_bf16x3_build(native):
    """The bf16x3 kernels are frozen and left out of the default library: these tests run only against a library built
    with PMX_BUILD_BF16X3=1 (native.py::SOURCES); the default build refuses the option, which is what the first test below checks."""
    if not native.has_bf16x3():
        pytest.skip('default build: no bf16x3 kernels (PMX_BUILD_BF16X3=1 adds conv_bf16x3.hip)')


def _f64_conv(x, w, b, relu, pool):
    import torch
    with torch.no_grad():
        y = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(),
                                       padding=w.shape[-1] // 2)
        if relu:
            y = torch.relu(y)
        if pool:
            y = torch.nn.functional.max_pool2d(y, 2, 2)
    return y.numpy()


@pytest.mark.parametrize('cin,h,w,cout,k,pool,force', [
    (128, 46, 46, 128, 7, False, 17), (185, 13, 46, 256, 7, False, 17), (48, 20, 46, 128, 7, False, 21),      # 7x7: 17- and 9-tile blocks
    (256, 24, 92, 256, 3, False, 18), (128, 24, 92, 128, 3, True, 19), (64, 30, 46, 128, 3, False, 18),       # 3x3, pooled, 4 input chunks
    (100, 14, 46, 200, 3, True, 23)])                                                                          # partial chunk / channels
def test_bf16x3_conv_is_fp32_grade(native, cin, h, w, cout, k, pool, force):
    eng = native.Engine(0, max_batch=3, max_h=368, max_w=368)
    rng = np.random.default_rng(cin + h)
    x = rng.standard_normal((3, cin, h, w)).astype('f')
    wt = (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype('f')
    b = rng.standard_normal(cout).astype('f')
    ref = _f64_conv(x, wt, b, True, pool)
    eng.set_option('ksplit', 1)
    eng.set_option('force_variant_k%d' % k, force)
    y32 = eng.conv2d(x, wt, b, relu=True, pool=pool)
    eng.set_option('precision', 1)
    y3 = eng.conv2d(x, wt, b, relu=True, pool=pool)
    eng.close()
    scale = np.abs(ref).max()
    e32, e3 = np.abs(y32 - ref).max() / scale, np.abs(y3 - ref).max() / scale
    assert np.isfinite(y3).all()
    assert not np.array_equal(y3, y32), 'the bf16x3 kernel did not run'
    assert e3 <= 3e-6 and e3 <= 3 * e32 + 2e-7, (e32, e3)          # as close to float64 as the fp32 FMA chain is


@pytest.mark.parametrize('cin,h,w,cout,k,pool,force,ksplit', [
    (128, 46, 46, 128, 7, False, 15, 1), (128, 46, 46, 256, 7, False, 15, 4), (192, 20, 30, 128, 7, False, 15, 3),
    (512, 23, 23, 256, 3, False, 16, 5), (256, 24, 40, 128, 3, True, 16, 2), (70, 9, 13, 64, 3, False, 16, 1)])
def test_bf16x3_small_tile_kernel_is_fp32_grade(native, cin, h, w, cout, k, pool, force, ksplit):
    """v8: the bf16x3 arithmetic on the 8 x 8 x 64 tiles of single-image launches, with and without K slices."""
    eng = native.Engine(0, max_batch=2, max_h=368, max_w=368)
    rng = np.random.default_rng(cin + h + ksplit)
    x = rng.standard_normal((1, cin, h, w)).astype('f')
    wt = (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype('f')
    b = rng.standard_normal(cout).astype('f')
    ref = _f64_conv(x, wt, b, True, pool)
    eng.set_option('ksplit', ksplit)
    eng.set_option('force_variant_k%d' % k, force)
    y32 = eng.conv2d(x, wt, b, relu=True, pool=pool)
    eng.set_option('precision', 1)
    y3 = eng.conv2d(x, wt, b, relu=True, pool=pool)
    eng.close()
    scale = np.abs(ref).max()
    e32, e3 = np.abs(y32 - ref).max() / scale, np.abs(y3 - ref).max() / scale
    assert np.isfinite(y3).all() and not np.array_equal(y3, y32)
    assert e3 <= 3e-6 and e3 <= 3 * e32 + 2e-7, (e32, e3)


def test_bf16x3_single_image_detector(native):
    """BASELINE config 2 in the bf16x3 mode: a single 368 x 368 image uses the v8 kernels (+ K slices); result vs the reference run."""
    PD = pkg('pose_detector')
    g = load_e2e('e2e_people')
    det = PD.PoseDetector(weights=g['weights'], device=0, precision='bf16x3')
    det.engine.profile_enable(True)
    poses, scores = det(g['img'])
    names = {e['kernel'] for e in det.engine.profile()}
    det.engine.profile_enable(False)
    peaks = det.engine.peaks(0)
    det.engine.close()
    assert any('v8bf16x3' in k for k in names), names
    assert peaks.shape == g['all_peaks'].shape and np.array_equal(peaks[:, [0, 1, 2, 4]], g['all_peaks'][:, [0, 1, 2, 4]])
    assert np.array_equal(np.asarray(poses), g['poses']) and np.abs(np.asarray(scores) - g['scores']).max() <= 1e-4


def test_bf16x3_network_matches_reference_golden_and_fp32_path(native):
    """batch 32 x 368 x 368 (the shapes the bf16x3 kernels are chosen for): the kernels really run, the maps stay within 1e-4 of the
    fp32 path (summation-order-sized noise through 92 layers)."""
    W = pkg('weights')
    eng = native.Engine(0, max_batch=32, max_h=368, max_w=368)
    eng.set_weights(W.synthetic_weights(0))
    imgs = np.random.default_rng(3).integers(0, 256, (32, 368, 368, 3), dtype=np.uint8)
    eng.forward_u8(imgs)
    p32, h32 = eng.get_maps()
    eng.set_option('precision', 1)
    eng.profile_enable(True)
    eng.forward_u8(imgs)
    names = {e['kernel'] for e in eng.profile()}
    eng.profile_enable(False)
    p3, h3 = eng.get_maps()
    eng.close()
    assert sum('bf16x3' in k for k in names) >= 3, names
    assert np.abs(p3 - p32).max() <= 1e-4 * max(1.0, np.abs(p32).max())
    assert np.abs(h3 - h32).max() <= 1e-4 * max(1.0, np.abs(h32).max())


def test_bf16x3_packs_equal_numpy(native):
    """One 64 x 48 image with the small-tile bf16x3 kernels forced: every layer that then has a bf16x3 pack -- a 3x3 and a 7x7 layer among
    them -- holds tests/pack_ref.py::bf16x3_pack of its direct pack, bit for bit (three bf16 planes per tap and chunk)."""
    import pack_ref
    w = pkg('weights').synthetic_weights(0)
    eng = native.Engine(0, max_batch=1, max_h=64, max_w=48)
    try:
        eng.set_weights(w)
        eng.set_option('force_variant_k7', 15)
        eng.set_option('force_variant_k3', 16)
        eng.set_option('precision', 1)
        eng.forward_u8(np.random.default_rng(5).integers(0, 256, (1, 64, 48, 3), dtype=np.uint8))
        eng.get_maps()
        sizes = set()
        for nm in sorted(w):
            got = eng.get_pack(nm, 'bf16x3')
            if got is None:
                continue
            cout, cin, ks, _ = eng.layer_shape(nm)
            direct = eng.get_pack(nm, 'w')
            cp = pack_ref.cout_pad(cout)
            assert ks > 1 and got.dtype == np.uint16 and got.size == 3 * direct.size
            assert np.array_equal(got, pack_ref.bf16x3_pack(direct, ks * ks, direct.size // (ks * ks * cp * 16), cp)), nm
            sizes.add(ks)
        assert sizes == {3, 7}
    finally:
        eng.close()


@pytest.mark.parametrize('name', ['e2e_person', 'e2e_people'])
def test_bf16x3_detector_on_reference_images(native, name):
    """The reference's own images replicated to a batch of 32 (so that the bf16x3 kernels are selected): peak indices and poses
    equal the reference run's, scores within 1e-4."""
    PD = pkg('pose_detector')
    g = load_e2e(name)
    det = PD.PoseDetector(weights=g['weights'], device=0, max_batch=32, precision='bf16x3')
    det.engine.profile_enable(True)
    out = det.detect_batch([g['img']] * 32)
    names = {e['kernel'] for e in det.engine.profile()}
    det.engine.profile_enable(False)
    assert any('bf16x3' in k for k in names), names
    peaks = det.engine.peaks(31)
    det.engine.close()
    assert peaks.shape == g['all_peaks'].shape and np.array_equal(peaks[:, [0, 1, 2, 4]], g['all_peaks'][:, [0, 1, 2, 4]])
    assert np.abs(peaks[:, 3] - g['all_peaks'][:, 3]).max() <= 1e-4
    for poses, scores in (out[0], out[31]):
        assert np.array_equal(np.asarray(poses), g['poses'])
        assert np.abs(np.asarray(scores) - g['scores']).max() <= 1e-4


@pytest.mark.parametrize('k,force,W,cout,pools', [(3, 16, 36, 64, (0, 1)), (7, 15, 36, 64, (0,)),         # small-tile kernel: conv_direct.h's epilogue
                                                  (3, 18, 46, 128, (0,)), (3, 19, 46, 128, (1,)), (7, 17, 46, 128, (0,)),     # conv_bf16x3_kernel's own
                                                  (3, 23, 46, 128, (1,)), (7, 21, 46, 128, (0,))])                           # ... nine-tile blocks
def test_bf16x3_nan_and_infinities(native, k, force, W, cout, pools):
    """The forward contract for non-finite values (include/pose_mi355x.h) in the bf16x3 mode, through the ReLU and the fused 2x2 pool of
    both epilogues (the small-tile kernel shares conv_direct.h's, the one-block-per-CU kernel conv_bf16x3_kernel -- 46-wide maps, 128
    output channels -- has its own): a NaN activation splits into three NaN terms, so the output is NaN exactly where the float64
    reference is; an infinite activation becomes inf - inf = NaN in the split's second term (x - bf16(x)), so the outputs whose window
    holds it are NaN where the reference has +-inf (or relu(-inf) = 0), and nothing else is non-finite; one NaN weight at a centre tap
    makes exactly its output channel NaN."""
    eng = native.Engine(0, max_batch=2, max_h=368, max_w=368)
    rng = np.random.default_rng(40 + k)
    x = rng.standard_normal((2, 32, 12, W)).astype('f')
    wt = (rng.standard_normal((cout, 32, k, k)) / np.sqrt(32 * k * k)).astype('f')
    b = rng.standard_normal(cout).astype('f')
    eng.set_option('ksplit', 1)
    eng.set_option('force_variant_k%d' % k, force)
    try:
        y32 = eng.conv2d(x, wt, b, relu=True, pool=bool(pools[0]))
        eng.set_option('precision', 1)
        assert not np.array_equal(eng.conv2d(x, wt, b, relu=True, pool=bool(pools[0])), y32), 'the bf16x3 kernel did not run'
        for relu, pool in ((0, 0), (1, 0), (0, 1), (1, 1)):
            if pool not in pools:
                continue
            xn = x.copy()
            xn[0, 3, 4, 5] = np.nan
            ref = _f64_conv(xn, wt, b, bool(relu), bool(pool))
            y = eng.conv2d(xn, wt, b, relu=bool(relu), pool=bool(pool))
            assert np.isnan(ref).any() and np.array_equal(np.isnan(y), np.isnan(ref)) and not np.isinf(y).any(), (relu, pool)
            fin = ~np.isnan(ref)
            assert np.abs(y[fin] - ref[fin]).max() <= 3e-6 * np.abs(ref[fin]).max()
            xi = xn.copy()
            xi[0, 17, 5, 18] = np.inf
            xi[1, 8, 6, 30] = -np.inf
            refi = _f64_conv(xi, wt, b, bool(relu), bool(pool))
            win = np.zeros((2, 12, W), bool)
            for bi, yy, xx in ((0, 4, 5), (0, 5, 18), (1, 6, 30)):
                win[bi, max(0, yy - k // 2):yy + k // 2 + 1, max(0, xx - k // 2):xx + k // 2 + 1] = True
            if pool:
                win = win.reshape(2, 6, 2, W // 2, 2).any(axis=(2, 4))
            y = eng.conv2d(xi, wt, b, relu=bool(relu), pool=bool(pool))
            bad = ~np.isfinite(y)
            assert not (~np.isfinite(refi) & ~bad).any() and np.array_equal(bad.any(axis=1), win) and bad.all(axis=1)[win].all(), (relu, pool)
            wn = wt.copy()
            wn[37, 5, k // 2, k // 2] = np.nan
            y = eng.conv2d(x, wn, b, relu=bool(relu), pool=bool(pool))
            nan = np.zeros(y.shape, bool)
            nan[:, 37] = True
            assert np.array_equal(np.isnan(y), nan) and not np.isinf(y).any(), (relu, pool)
    finally:
        eng.close()
