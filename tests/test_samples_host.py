"""CPU: the sample preparation's host side (samples.py) against what the reference's own loader did (tests/golden/sample_ref.npz, recorded by
tools/record_sample_goldens.py), the NumPy restatement of its pixel steps (tests/sample_ref.py) against independent mathematics, and the
argument checks of the new entries."""
import colorsys
import json
import os
import random

import numpy as np
import pytest

import sample_ref
from conftest import GOLDEN, ROOT, pkg

ENTRIES = ('pmx_samples_prepare', 'pmx_samples_device_ptrs', 'pmx_get_samples', 'pmx_validate_samples')
BOUNDS = os.path.join(ROOT, 'profiles', 'sample_prep.json')
MISSING = -999


@pytest.fixture(scope='module')
def rec():
    z = np.load(os.path.join(GOLDEN, 'sample_ref.npz'))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def S():
    return pkg('samples')


def scene_of(rec, seed):
    i = seed % int(rec['n_scenes'])
    return rec['scene%d_img' % i], rec['scene%d_mask' % i], rec['scene%d_poses' % i]


def drawn(S, rec, seed):
    img, _, poses = scene_of(rec, seed)
    random.seed(seed)
    np.random.seed(seed)
    return S.draw_augmentation(img.shape[:2], poses, int(rec['insize']))


# ---- 1. draws and poses against the recorded reference ----------------------------------------------------------------------------
def test_draws_and_poses_equal_the_recorded_reference(S, rec):
    n = int(rec['n_seeds'])
    assert n >= 16
    for seed in range(n):
        r = drawn(S, rec, seed)
        pre, d = 'seed%d_' % seed, r.draws
        assert d['u'] == float(rec[pre + 'u']) and d['randn'] == float(rec[pre + 'randn']), seed
        assert d['bbox_index'] == int(rec[pre + 'index']) and d['r_xy'] == tuple(rec[pre + 'r_xy']), seed
        assert r.resized == tuple(rec[pre + 'resized']) and r.rotated == tuple(rec[pre + 'rotated']), seed
        assert np.array_equal(r.R, rec[pre + 'R']), seed
        want = rec[pre + 'distort']
        assert (r.distort is None) == (want[0] == MISSING) and (r.distort is None or r.distort == tuple(want)), seed
        assert r.flip == bool(rec[pre + 'flip']), seed
        assert [d['min_scale'], d['max_scale'], d['scale']] == list(rec[pre + 'scales']), seed
        assert list(d['center']) + list(r.offset) == list(rec[pre + 'center_offset']) and d['bounds'] == list(rec[pre + 'bounds']), seed
        got = S.transform_poses(scene_of(rec, seed)[2], r)
        assert got.dtype == np.int32 and np.array_equal(got, rec[pre + 'poses']), seed


def test_recorded_seeds_cover_every_branch_twice(rec):
    insize = int(rec['insize'])
    cover = dict(distort=0, plain=0, flip=0, noflip=0, left=0, top=0, right=0, bottom=0, min_lo=0, min_hi=0, max_lo=0, max_hi=0)
    for seed in range(int(rec['n_seeds'])):
        pre = 'seed%d_' % seed
        x_from, y_from, x_to, y_to = rec[pre + 'bounds'][4:]
        mn, mx, _ = rec[pre + 'scales']
        hits = dict(distort=rec[pre + 'distort'][0] != MISSING, plain=rec[pre + 'distort'][0] == MISSING, flip=rec[pre + 'flip'] == 1,
                    noflip=rec[pre + 'flip'] == 0, left=x_from > 0, top=y_from > 0, right=x_to < insize - 1, bottom=y_to < insize - 1,
                    min_lo=mn == 0.5, min_hi=mn == 1, max_lo=mx == 1, max_hi=mx == 2)
        for k, v in hits.items():
            cover[k] += bool(v)
    assert min(cover.values()) >= 2, cover


def test_restatement_reproduces_the_recorded_samples(S, rec):
    """the orchestration (crop bounds, seam, flip, dilation after the resize) of sample_ref.prepare = that of the verbatim loader"""
    insize = int(rec['insize'])
    for seed in range(int(rec['n_seeds'])):
        img, mask, _ = scene_of(rec, seed)
        got = sample_ref.prepare(img, mask, drawn(S, rec, seed), insize)
        assert np.array_equal(got[0], rec['seed%d_img' % seed]) and np.array_equal(got[2], rec['seed%d_mask' % seed]), seed
    for i in range(int(rec['n_scenes'])):
        img, mask, poses = rec['scene%d_img' % i], rec['scene%d_mask' % i], rec['scene%d_poses' % i]
        r = S.SampleRecord.val(img.shape[:2], insize)
        got = sample_ref.prepare(img, mask, r, insize)
        assert np.array_equal(got[0], rec['val%d_img' % i]) and np.array_equal(got[2], rec['val%d_mask' % i])
        assert np.array_equal(S.transform_poses(poses, r), rec['val%d_poses' % i])


# ---- 2. the warp against independent mathematics ------------------------------------------------------------------------------------
def noise_image(h=40, w=52, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3)).astype(np.uint8)


def smooth_image(n=48):
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float64)
    return np.clip(np.rint(100 + 1.5 * xx + 1.0 * yy + 20 * np.sin(xx / 6) * np.cos(yy / 7)), 0, 255).astype(np.uint8)


def keys(t, A=-0.75):
    t = abs(t)
    if t <= 1:
        return (A + 2) * t ** 3 - (A + 3) * t ** 2 + 1
    if t < 2:
        return A * t ** 3 - 5 * A * t ** 2 + 8 * A * t - 4 * A
    return 0.0


def bicubic_float(img, R, dsize):
    """float64 Keys bicubic at the exact source coordinate; NaN where a tap leaves the source"""
    M = np.array(sample_ref.invert_affine(R))
    h, w = img.shape
    out = np.full((dsize[1], dsize[0]), np.nan)
    for y in range(dsize[1]):
        for x in range(dsize[0]):
            sx, sy = M[0] * x + M[1] * y + M[2], M[3] * x + M[4] * y + M[5]
            ix, iy = int(np.floor(sx)), int(np.floor(sy))
            if ix < 1 or iy < 1 or ix + 2 > w - 1 or iy + 2 > h - 1:
                continue
            out[y, x] = sum(keys(sy - (iy + i)) * keys(sx - (ix + j)) * float(img[iy + i, ix + j]) for i in range(-1, 3) for j in range(-1, 3))
    return out


def rotation_of(S, w, h, degree):
    """the reference's matrix and rotated size (:108-115) for a given angle"""
    rad = degree * np.pi / 180
    R = S.rotation_matrix((w / 2, h / 2), degree, 1)
    bbox = (w * abs(np.cos(rad)) + h * abs(np.sin(rad)), w * abs(np.sin(rad)) + h * abs(np.cos(rad)))
    R[0, 2] += bbox[0] / 2 - w / 2
    R[1, 2] += bbox[1] / 2 - h / 2
    return R, (int(bbox[0] + 0.5), int(bbox[1] + 0.5))


def warp_noise_difference(S):
    """max and histogram of |fixed point - float64 bicubic| on a noise image rotated by 17 degrees, interior pixels"""
    img = noise_image()[:, :, 0]
    R, size = rotation_of(S, img.shape[1], img.shape[0], 17.0)
    ref = bicubic_float(img, R, size)
    got = sample_ref.warp_affine(img, R, size, True, 128).astype(np.float64)
    ok = ~np.isnan(ref)
    d = np.abs(got[ok] - np.clip(ref[ok], 0, 255))
    return float(d.max()), np.bincount(np.floor(d).astype(int)).tolist()


def test_weight_tables_sum_to_one():
    for tab in (sample_ref.cubic_table(), sample_ref.linear_table()):
        assert (tab.astype(np.int64).sum(axis=2) == 32768).all() and tab.shape[:2] == (32, 32)
    c, l = sample_ref.cubic_table()[0, 0], sample_ref.linear_table()[0, 0]
    assert c[5] == 32768 and np.count_nonzero(c) == 1 and l[0] == 32768 and np.count_nonzero(l) == 1


def test_identity_matrix_reproduces_the_source():
    img = noise_image()
    R = np.array([[1.0, 0, 0], [0, 1.0, 0]])
    assert np.array_equal(sample_ref.warp_affine(img, R, (img.shape[1], img.shape[0]), True, 128), img)
    assert np.array_equal(sample_ref.warp_affine(img[:, :, 0], R, (img.shape[1], img.shape[0]), False, 0), img[:, :, 0])


def test_rotation_by_90_degrees_is_rot90_shifted_by_one_row(S):
    """The reference's matrix for 90 degrees maps destination (x', y') to source (x, y) = (w - y', x'): np.rot90 reads (w - 1 - y', x').  So
    destination row y' is row y' - 1 of np.rot90, and row 0 reads the column x = w, outside the source: the border."""
    img = noise_image()
    h, w = img.shape[:2]
    R, size = rotation_of(S, w, h, 90.0)
    assert size == (h, w)
    out = sample_ref.warp_affine(img, R, size, True, 128)
    assert np.array_equal(out[1:], np.rot90(img)[:-1]) and (out[0] == 128).all()


def test_pixel_form_equals_array_form(S):
    img = noise_image(20, 24)
    R, size = rotation_of(S, 24, 20, -17.0)
    M = sample_ref.invert_affine(R)
    for cubic, src, border in ((True, img, 128), (False, (img[:, :, 0] > 128).astype(np.uint8) * 255, 0)):
        full = sample_ref.warp_affine(src, R, size, cubic, border)
        for y in range(0, size[1], 3):
            for x in range(0, size[0], 2):
                assert sample_ref.warp_pixel(src, M, x, y, cubic, border) == list(np.atleast_1d(full[y, x])), (cubic, x, y)


def test_fixed_point_cubic_is_within_one_level_of_float64_on_a_smooth_image(S):
    """position quantisation 1/64 pixel x gradient < 5 levels / pixel, 15-bit weights and the final rounding: below one level"""
    img = smooth_image()
    for degree in (17.0, -40.0):
        R, size = rotation_of(S, 48, 48, degree)
        ref = bicubic_float(img, R, size)
        got = sample_ref.warp_affine(img, R, size, True, 128).astype(np.float64)
        ok = ~np.isnan(ref)
        assert ok.sum() > 1000 and np.abs(got[ok] - ref[ok]).max() <= 1.0


def test_noise_difference_stays_at_the_recorded_maximum(S):
    want = json.load(open(BOUNDS))['restatement_bounds']['warp_noise_max']
    got, hist = warp_noise_difference(S)
    print('warp noise: max %.3f histogram %r (recorded max %.3f)' % (got, hist, want))
    assert got <= want + 1


# ---- 3. colour --------------------------------------------------------------------------------------------------------------------
def colour_lattice():
    g = np.arange(0, 256, 8)
    g[-1] = 255
    cube = np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=-1).reshape(-1, 3)
    greys = np.repeat(np.arange(256)[:, None], 3, axis=1)
    prim = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [255, 0, 255], [0, 255, 255]])
    return np.concatenate([cube, greys, prim]).astype(np.uint8)


def colour_roundtrip_max():
    px = colour_lattice()
    return int(np.abs(sample_ref.hsv2bgr(sample_ref.bgr2hsv(px)).astype(int) - px.astype(int)).max())


def test_hsv_is_within_one_of_colorsys():
    px = colour_lattice()
    hsv = sample_ref.bgr2hsv(px).astype(int)
    for (b, g, r), (h, s, v) in zip(px.tolist(), hsv.tolist()):
        ch, cs, cv = colorsys.rgb_to_hsv(r / 255.0, g / 255.0, b / 255.0)
        dh = abs(h - ch * 180.0)
        assert min(dh, 180 - dh) <= 1 and abs(s - cs * 255.0) <= 1 and abs(v - cv * 255.0) <= 1, (b, g, r, h, s, v)


def test_hsv_to_bgr_follows_colorsys():
    """HSV -> BGR alone: colorsys on the same 8-bit h, s, v; the float32 formula differs from the float64 one only at rounding ties"""
    rng = np.random.default_rng(5)
    hsv = np.stack([rng.integers(0, 180, 4000), rng.integers(0, 256, 4000), rng.integers(0, 256, 4000)], axis=-1).astype(np.uint8)
    got = sample_ref.hsv2bgr(hsv).astype(int)
    for (h, s, v), (b, g, r) in zip(hsv.tolist(), got.tolist()):
        cr, cg, cb = colorsys.hsv_to_rgb(h / 180.0, s / 255.0, v / 255.0)
        assert abs(r - cr * 255) <= 0.5 + 1e-3 and abs(g - cg * 255) <= 0.5 + 1e-3 and abs(b - cb * 255) <= 0.5 + 1e-3, (h, s, v)


def test_colour_round_trip_stays_at_the_recorded_maximum():
    want = json.load(open(BOUNDS))['restatement_bounds']['colour_roundtrip_max']
    got = colour_roundtrip_max()
    print('colour round trip: max %d (recorded %d)' % (got, want))
    assert got <= want + 1


def test_hue_is_clamped_not_wrapped():
    red = np.array([[[0, 0, 200]]], np.uint8)                  # h = 0
    pink = np.array([[[40, 0, 200]]], np.uint8)                # h = 174
    h_red, h_pink = int(sample_ref.bgr2hsv(red)[0, 0, 0]), int(sample_ref.bgr2hsv(pink)[0, 0, 0])
    assert h_red == 0 and h_pink >= 170
    # below 0: clamped to 0, the colour does not move to the other end of the circle
    assert np.array_equal(sample_ref.distort(red, (-10, 0, 0)), sample_ref.distort(red, (0, 0, 0)))
    # above 179: h + 10 stays as it is (<= 255) and counts modulo 180
    hsv = sample_ref.bgr2hsv(pink).astype(int)
    hsv[..., 0] = (h_pink + 10) % 180
    assert h_pink + 10 > 179 and np.array_equal(sample_ref.distort(pink, (10, 0, 0)), sample_ref.hsv2bgr(hsv.astype(np.uint8)))


# ---- 4. dilation ------------------------------------------------------------------------------------------------------------------
DILATE_BOXES = {            # set pixel (y, x) of a 32 x 32 mask -> rows y0 .. y1, columns x0 .. x1 (inclusive): [-7 .. +8], clipped
    (0, 0): (0, 8, 0, 8), (0, 31): (0, 8, 24, 31), (31, 0): (24, 31, 0, 8), (31, 31): (24, 31, 24, 31),
    (0, 16): (0, 8, 9, 24), (31, 16): (24, 31, 9, 24), (16, 0): (9, 24, 0, 8), (16, 31): (9, 24, 24, 31),
    (16, 16): (9, 24, 9, 24),
}


@pytest.mark.parametrize('fn', ['dilate16', 'dilate16_gather'])
def test_dilation_boxes(fn):
    f = getattr(sample_ref, fn)
    for (y, x), (y0, y1, x0, x1) in DILATE_BOXES.items():
        m = np.zeros((32, 32), bool)
        m[y, x] = True
        want = np.zeros((32, 32), bool)
        want[y0:y1 + 1, x0:x1 + 1] = True
        assert np.array_equal(f(m), want), (y, x)
    assert not f(np.zeros((32, 32), bool)).any() and f(np.ones((32, 32), bool)).all()


# ---- 5. the interface ---------------------------------------------------------------------------------------------------------------
def test_sample_entries_declared_and_bound():
    native = pkg('native')
    syms = native.header_symbols()
    for s in ENTRIES:
        assert s in syms, s
    assert ('pmx_samples.hip', ['-ffp-contract=off']) in native.SOURCES
    if native.needs_build():
        native.build()
    lib = native.load()
    for s in ENTRIES:
        assert getattr(lib, s) is not None and s in lib._pmx_sig, s
    for name in ('samples_prepare', 'samples_get', 'samples_device_ptrs', 'validate_samples'):
        assert callable(getattr(native.Engine, name))
    import ctypes
    assert ctypes.sizeof(native.PmxSample) == 16 + 15 * 4 + 4 + 48          # two pointers, fifteen ints, padding, six doubles


def test_sample_records_check_their_numbers(S):
    ok = dict(src_hw=(40, 60), insize=32, mode='train', offset=(3, 4))
    S.SampleRecord(**ok)
    bad = [dict(ok, insize=30), dict(ok, insize=0), dict(ok, src_hw=(0, 4)), dict(ok, mode='test'), dict(ok, offset=None),
           dict(ok, resized=(0, 5)), dict(ok, R=np.eye(2, 3)), dict(ok, R=np.zeros((2, 3)), rotated=(5, 5)),
           dict(ok, R=np.array([[1, 0, np.nan], [0, 1, 0]]), rotated=(5, 5)), dict(ok, R=np.eye(2, 3), rotated=(0, 5)),
           dict(ok, distort=(11, 0, 0)), dict(ok, distort=(0, -41, 0)), dict(ok, distort=(0, 0, 31)),
           dict(ok, mode='val'), dict(src_hw=(40, 60), insize=32, mode='val', flip=True)]
    for kw in bad:
        with pytest.raises(ValueError):
            S.SampleRecord(**kw)
    with pytest.raises(ValueError):
        S.draw_augmentation((40, 60), np.zeros((0, 18, 3), np.int32), 32)
    with pytest.raises(ValueError):
        S.draw_augmentation((40, 60), np.zeros((1, 18, 3), np.int32), 32)          # nobody visible
    with pytest.raises(ValueError):
        S.transform_poses(np.full((1, 18, 3), 0.5), S.SampleRecord.val((40, 60), 32))


def test_prepare_samples_checks_its_arguments_without_a_device(S):
    det = object.__new__(pkg('pose_detector').PoseDetector)          # no device context: the checks run before one is needed
    img = np.zeros((40, 60, 3), np.uint8)
    one = np.zeros((1, 18, 3), np.int32)
    val = S.SampleRecord.val((40, 60), 32)
    bad = [
        dict(imgs=[], poses_per_image=[]),
        dict(imgs=[img.astype(np.float32)], poses_per_image=[one]),
        dict(imgs=[img[:, :, :2]], poses_per_image=[one]),
        dict(imgs=[img], poses_per_image=[one, one]),
        dict(imgs=[img], poses_per_image=[np.zeros((1, 17, 3), np.int32)]),
        dict(imgs=[img], poses_per_image=[one + 0.5]),
        dict(imgs=[img], poses_per_image=[one], insize=36),
        dict(imgs=[img], poses_per_image=[one], insize=0),
        dict(imgs=[img], poses_per_image=[one], mode='eval'),
        dict(imgs=[img], poses_per_image=[one], ignore_masks=[np.zeros((32, 32), bool)]),
        dict(imgs=[img], poses_per_image=[one], ignore_masks=[None, None]),
        dict(imgs=[img], poses_per_image=[one], insize=32, records=[val, val]),
        dict(imgs=[img], poses_per_image=[one], insize=32, records=['val']),
        dict(imgs=[img], poses_per_image=[one], insize=64, records=[val]),
        dict(imgs=[img], poses_per_image=[one], insize=32, records=[S.SampleRecord.val((60, 40), 32)]),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            det.prepare_samples(**kw)
    for kw in bad[:8] + bad[9:11]:                                   # the cases without mode= / records=
        with pytest.raises(ValueError):
            det.validation_loss_raw(**kw)
