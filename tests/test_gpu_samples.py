"""GPU: the sample preparation (include/pose_mi355x.h: pmx_samples_*) -- bit-exact against the NumPy restatement tests/sample_ref.py,
equal to what the verbatim reference loader recorded (tests/golden/sample_ref.npz), independent of a sample's place in the call, and
`validation_loss_raw` against `validation_loss` on host-prepared inputs."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import sample_ref
from conftest import GOLDEN, pkg

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23          # one float32 ulp of 1: the label generator's bound against the reference's maps


@pytest.fixture(scope='module')
def S():
    return pkg('samples')


@pytest.fixture(scope='module')
def eng(native):
    e = native.Engine(0, max_batch=4, max_h=96, max_w=96)
    yield e
    e.close()


@pytest.fixture(scope='module')
def rec():
    z = np.load(os.path.join(GOLDEN, 'sample_ref.npz'))
    return {k: z[k] for k in z.files}


def image(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(xx * 5 + yy) % 256, (yy * 4 + 60) % 256, (xx * 3 + yy * 2) % 256], axis=-1) + rng.integers(-30, 31, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def border_mask(h, w):
    m = np.zeros((h, w), bool)
    m[0, :5] = True
    m[h - 1, w - 4:] = True
    m[h // 2:h // 2 + 3, 0] = True
    m[2:6, w - 1] = True
    m[h // 3, w // 2] = True
    return m


def rotation(S, w, h, degree):
    rad = degree * np.pi / 180
    R = S.rotation_matrix((w / 2, h / 2), degree, 1)
    bbox = (w * abs(np.cos(rad)) + h * abs(np.sin(rad)), w * abs(np.sin(rad)) + h * abs(np.cos(rad)))
    R[0, 2] += bbox[0] / 2 - w / 2
    R[1, 2] += bbox[1] / 2 - h / 2
    return R, (int(bbox[0] + 0.5), int(bbox[1] + 0.5))


def check(eng, imgs, masks, recs, insize):
    eng.samples_prepare(imgs, masks, recs, insize)
    got_i, got_m = eng.samples_get()
    for k, (img, r) in enumerate(zip(imgs, recs)):
        want = sample_ref.prepare(img, None if masks is None else masks[k], r, insize)
        assert np.array_equal(got_i[k], want[0]), (k, np.abs(got_i[k].astype(int) - want[0]).max())
        assert np.array_equal(got_m[k], want[2]), k
    return got_i, got_m


# ---- 6. bit-exact against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('insize', [32, 64])
def test_validation_samples_of_three_sizes_in_one_call(eng, S, insize):
    sizes = [(24, 40), (96, 72), (insize, insize)]                  # up-scale, down-scale, already at insize
    imgs = [image(h, w, 10 + i) for i, (h, w) in enumerate(sizes)]
    masks = [border_mask(h, w) for h, w in sizes]
    recs = [S.SampleRecord.val(s, insize) for s in sizes]
    got_i, _ = check(eng, imgs, masks, recs, insize)
    assert np.array_equal(got_i[2], imgs[2])
    _, got_m = check(eng, imgs, None, recs, insize)                  # mask = NULL
    assert not got_m.any()
    check(eng, imgs, [masks[0], None, masks[2]], recs, insize)


@pytest.mark.parametrize('degree', [0.0, 90.0, 17.0, -17.0, 40.0])
def test_rotations(eng, S, degree):
    insize = 64
    imgs = [image(48, 80, 21), image(72, 56, 22)]
    masks = [border_mask(48, 80), border_mask(72, 56)]
    recs = []
    for img, rs in zip(imgs, ((96, 60), None)):                      # one resized up first, one as it is
        w, h = rs if rs else (img.shape[1], img.shape[0])
        R, size = rotation(S, w, h, degree)
        recs.append(S.SampleRecord(img.shape[:2], insize, resized=rs, R=R, rotated=size, offset=((size[0] - insize) // 2, (size[1] - insize) // 2)))
    check(eng, imgs, masks, recs, insize)


@pytest.mark.parametrize('insize', [32, 64])
def test_crop_windows_colour_and_flip(eng, S, insize):
    img, mask = image(60, 84, 31), border_mask(60, 84)
    R, size = rotation(S, 84, 60, 17.0)
    offs = {'left': (-9, 10), 'top': (12, -7), 'right': (size[0] - insize + 11, 8), 'bottom': (6, size[1] - insize + 5),
            'inside': (14, 9) if insize == 32 else ((size[0] - insize) // 2, 2), 'corner': (-insize + 3, -insize + 2), 'outside': (-200, 5)}
    extremes = [None, (10, 40, 30), (-10, -40, -30), (10, -40, 30), (-10, 40, -30), (0, 0, 0), (7, -3, 0)]
    recs = []
    for k, (name, off) in enumerate(offs.items()):
        recs.append(S.SampleRecord(img.shape[:2], insize, R=R, rotated=size, offset=off, distort=extremes[k], flip=bool(k % 2)))
    for i in range(0, len(recs), 4):
        part = recs[i:i + 4]
        check(eng, [img] * len(part), [mask] * len(part), part, insize)
    # no rotation: the window straight from the (resized) source, down-scaled and as it is
    plain = [S.SampleRecord(img.shape[:2], insize, resized=(50, 37), offset=(-5, 4), distort=(10, 40, -30), flip=True),
             S.SampleRecord(img.shape[:2], insize, offset=(30, -6), distort=None, flip=False),
             S.SampleRecord(img.shape[:2], insize, resized=(168, 120), offset=(100, 70), flip=True)]
    check(eng, [img] * 3, [mask, None, mask], plain, insize)


def test_colour_on_every_hue_sector(eng, S):
    """a source whose pixels sweep the colour cube, cut out unrotated: the integer BGR -> HSV and the float32 HSV -> BGR on many colours"""
    g = np.arange(0, 256, 5, dtype=np.uint8)
    cube = np.stack(np.meshgrid(g, g[::2], g, indexing='ij'), axis=-1).reshape(-1, 3)
    img = np.ascontiguousarray(cube[:64 * 64 * 4].reshape(128, 128, 3))
    recs = [S.SampleRecord((128, 128), 64, offset=(ox, oy), distort=d) for (ox, oy), d in
            zip(((0, 0), (64, 0), (0, 64), (64, 64)), ((0, 0, 0), (10, 40, 30), (-10, -40, -30), (5, -20, 11)))]
    check(eng, [img] * 4, None, recs, 64)


# ---- 7. the recorded reference samples --------------------------------------------------------------------------------------------
def test_recorded_reference_samples(eng, S, rec):
    insize = int(rec['insize'])
    n, ns = int(rec['n_seeds']), int(rec['n_scenes'])
    scene = lambda i: (rec['scene%d_img' % i], rec['scene%d_mask' % i], rec['scene%d_poses' % i])
    recs = []
    for seed in range(n):
        random.seed(seed)
        np.random.seed(seed)
        recs.append(S.draw_augmentation(scene(seed % ns)[0].shape[:2], scene(seed % ns)[2], insize))
    for i in range(0, n, 4):
        seeds = list(range(i, min(i + 4, n)))
        eng.samples_prepare([scene(s % ns)[0] for s in seeds], [scene(s % ns)[1] for s in seeds], [recs[s] for s in seeds], insize)
        got_i, got_m = eng.samples_get()
        for k, s in enumerate(seeds):
            assert np.array_equal(got_i[k], rec['seed%d_img' % s]) and np.array_equal(got_m[k], rec['seed%d_mask' % s]), s
    vals = [S.SampleRecord.val(scene(i)[0].shape[:2], insize) for i in range(ns)]
    eng.samples_prepare([scene(i)[0] for i in range(ns)], [scene(i)[1] for i in range(ns)], vals, insize)
    got_i, got_m = eng.samples_get()
    for i in range(ns):
        assert np.array_equal(got_i[i], rec['val%d_img' % i]) and np.array_equal(got_m[i], rec['val%d_mask' % i]), i
    for s in rec['label_seeds']:                           # transform_poses + the device's label generator = the reference's label maps
        poses = S.transform_poses(scene(int(s) % ns)[2], recs[int(s)])
        eng.loss_set_poses([poses], insize, insize)
        paf, heat = eng.labels(0)
        # the bound of the device label generator against the reference's own maps (tests/test_gpu_validation_loss.py: one float32 ulp of 1)
        assert np.array_equal(paf != 0, rec['seed%d_pafs' % s] != 0)
        assert np.abs(paf - rec['seed%d_pafs' % s]).max() <= ULP and np.abs(heat - rec['seed%d_heats' % s]).max() <= ULP, s


# ---- 8. independence --------------------------------------------------------------------------------------------------------------
def test_a_sample_does_not_depend_on_its_place_or_its_neighbours(eng, S):
    insize = 32
    sizes = [(24, 40), (96, 72), (40, 40), (64, 48)]
    imgs = [image(h, w, 40 + i) for i, (h, w) in enumerate(sizes)]
    masks = [border_mask(h, w) for h, w in sizes]
    R, size = rotation(S, 72, 96, -17.0)
    recs = [S.SampleRecord.val(sizes[0], insize), S.SampleRecord(sizes[1], insize, R=R, rotated=size, offset=(20, 30), distort=(3, -9, 12), flip=True),
            S.SampleRecord(sizes[2], insize, resized=(70, 66), offset=(-4, 40)), S.SampleRecord.val(sizes[3], insize)]
    a_i, a_m = check(eng, imgs, masks, recs, insize)
    order = [2, 0, 3, 1]
    eng.samples_prepare([imgs[k] for k in order], [masks[k] for k in order], [recs[k] for k in order], insize)
    b_i, b_m = eng.samples_get()
    for pos, k in enumerate(order):
        assert a_i[k].tobytes() == b_i[pos].tobytes() and a_m[k].tobytes() == b_m[pos].tobytes()
    for k in range(4):
        eng.samples_prepare([imgs[k]], [masks[k]], [recs[k]], insize)
        c_i, c_m = eng.samples_get()
        assert a_i[k].tobytes() == c_i[0].tobytes() and a_m[k].tobytes() == c_m[0].tobytes()


def test_window_warp_equals_the_crop_of_the_full_warp(eng, S):
    """insize = the rotated size and offset 0 give the whole rotated image; a window of it is the same bytes"""
    img, mask = image(48, 48, 50), border_mask(48, 48)
    R, size = rotation(S, 48, 48, 40.0)
    assert size[0] == size[1]
    size_pad = -(-size[0] // 8) * 8                                # insize is a multiple of 8: the rest of the window is the crop's fill
    full = S.SampleRecord((48, 48), size_pad, R=R, rotated=size, offset=(0, 0))
    eng.samples_prepare([img], [mask], [full], size_pad)
    f_i, _ = eng.samples_get()
    want = sample_ref.warp_affine(img, R, size, True, 128)
    assert np.array_equal(f_i[0][:size[1], :size[0]], want) and (f_i[0][size[1]:] == 127).all() and (f_i[0][:, size[0]:] == 127).all()
    win = S.SampleRecord((48, 48), 32, R=R, rotated=size, offset=(13, 21))
    eng.samples_prepare([img], [mask], [win], 32)
    w_i, _ = eng.samples_get()
    assert np.array_equal(w_i[0], f_i[0][21:53, 13:45])


# ---- 9. validation_loss_raw -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['f32', 'f16'])
def test_validation_loss_raw_equals_validation_loss_on_host_prepared_inputs(S, precision):
    PD = pkg('pose_detector')
    det = PD.PoseDetector(weights=pkg('weights').synthetic_weights(0), device=0, max_batch=3, max_size=(64, 64), precision=precision)
    sizes = [(24, 40), (96, 72), (64, 64)]
    imgs = [image(h, w, 60 + i) for i, (h, w) in enumerate(sizes)]
    masks = [border_mask(*sizes[0]), np.zeros(sizes[1], bool), border_mask(*sizes[2])]
    rng = np.random.default_rng(61)
    poses = []
    for h, w in sizes:
        p = np.zeros((2, 18, 3), np.int32)
        p[:, :, 0], p[:, :, 1], p[:, :, 2] = rng.integers(0, w, (2, 18)), rng.integers(0, h, (2, 18)), rng.choice([0, 1, 2], (2, 18))
        poses.append(p)
    before = det.detect_batch([imgs[2]])
    got = det.validation_loss_raw(imgs, poses, masks, insize=64)
    after = det.detect_batch([imgs[2]])                            # the prepared buffers are not the activation buffers
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(before, after))
    host = [sample_ref.prepare(im, m, S.SampleRecord.val(im.shape[:2], 64), 64) for im, m in zip(imgs, masks)]
    host_poses = [S.transform_poses(p, S.SampleRecord.val(im.shape[:2], 64)) for p, im in zip(poses, imgs)]
    want = det.validation_loss([h[0] for h in host], host_poses, [h[2] for h in host])
    assert got == want, (got, want)
    assert np.isfinite(got['val/loss']) and got['val/loss'] > 0
    out_i, out_p, out_m = det.prepare_samples(imgs, poses, masks, insize=64)
    assert all(np.array_equal(out_i[k], host[k][0]) and np.array_equal(out_m[k], host[k][2]) and np.array_equal(out_p[k], host_poses[k])
               for k in range(3))
    random.seed(4)
    np.random.seed(4)
    t_i, t_p, t_m = det.prepare_samples(imgs[1:], poses[1:], masks[1:], insize=64, mode='train')
    random.seed(4)
    np.random.seed(4)
    for k in (1, 2):
        r = S.draw_augmentation(imgs[k].shape[:2], poses[k], 64)
        w = sample_ref.prepare(imgs[k], masks[k], r, 64)
        assert np.array_equal(t_i[k - 1], w[0]) and np.array_equal(t_m[k - 1], w[2]) and np.array_equal(t_p[k - 1], S.transform_poses(poses[k], r))


# ---- 10. errors -------------------------------------------------------------------------------------------------------------------
def test_error_statuses_leave_the_context_usable(native, eng, S):
    INVALID, CAPACITY, STATE = 1, 5, 6
    lib = eng.lib
    img = image(40, 56, 70)

    def sample(**kw):
        s = native.PmxSample()
        s.bgr, s.src_h, s.src_w = native._ptr(img), 40, 56
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def call(s, n=1, insize=32, ctx=None):
        arr = (native.PmxSample * 1)(s)
        rc = lib.pmx_samples_prepare((ctx or eng)._ctx, C.cast(arr, C.c_void_p), n, insize, 0)
        assert rc == 0 or lib.pmx_last_error().decode().strip()
        return rc

    ident = (C.c_double * 6)(1, 0, 0, 0, 1, 0)
    train = dict(has_crop=1, off_x=2, off_y=3)
    check(eng, [img], None, [S.SampleRecord.val((40, 56), 32)], 32)
    before = eng.samples_get()
    assert lib.pmx_samples_prepare(eng._ctx, None, 1, 32, 0) == INVALID
    assert call(sample(bgr=None)) == INVALID
    assert call(sample(), n=0) == INVALID and call(sample(), n=-1) == INVALID
    assert call(sample(), insize=36) == INVALID and call(sample(), insize=0) == INVALID and call(sample(), insize=-8) == INVALID
    assert call(sample(src_h=0)) == INVALID and call(sample(src_w=-3)) == INVALID
    assert call(sample(resized_w=10, resized_h=-1, **train)) == INVALID
    assert call(sample(has_rotate=1, rot_w=0, rot_h=40, inv=ident, **train)) == INVALID
    assert call(sample(has_rotate=1, rot_w=40, rot_h=40, inv=(C.c_double * 6)(1, 0, float('nan'), 0, 1, 0), **train)) == INVALID
    assert call(sample(has_rotate=1, rot_w=40, rot_h=40, inv=(C.c_double * 6)(1, 0, 0, 0, float('inf'), 0), **train)) == INVALID
    assert call(sample(has_rotate=1, rot_w=40, rot_h=40, inv=(C.c_double * 6)(1, 2, 0, 2, 4, 0), **train)) == INVALID          # singular
    for d in ((11, 0, 0), (0, 41, 0), (0, 0, -31)):
        assert call(sample(has_distort=1, delta=(C.c_int32 * 3)(*d), **train)) == INVALID
    assert call(sample(flip=1)) == INVALID and call(sample(resized_w=20, resized_h=20)) == INVALID          # validation sample with another step
    assert call(sample(), n=5) == CAPACITY
    assert call(sample(), insize=104) == CAPACITY
    assert call(sample(resized_w=16384, resized_h=16384, **train)) == CAPACITY                                 # 1 GiB of intermediates
    for arch in ('facenet', 'handnet'):
        f = native.Engine(0, max_batch=1, max_h=64, max_w=64, arch=arch)
        assert call(sample(), ctx=f) == STATE
        assert lib.pmx_validate_samples(f._ctx, None, None, None) == INVALID
        one, out = np.zeros(1, np.int32), np.zeros(13)
        assert lib.pmx_validate_samples(f._ctx, None, native._ptr(one), native._ptr(out)) == STATE
        f.close()
    fresh = native.Engine(0, max_batch=1, max_h=64, max_w=64)
    one, out = np.zeros(1, np.int32), np.zeros(13)
    assert lib.pmx_validate_samples(fresh._ctx, None, native._ptr(one), native._ptr(out)) == STATE            # nothing prepared
    assert lib.pmx_get_samples(fresh._ctx, None, None, 1, 32) == STATE
    assert lib.pmx_samples_device_ptrs(fresh._ctx, None, None) == STATE
    fresh.close()
    # a refused call leaves the prepared samples and the context as they were
    after = eng.samples_get()
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    assert lib.pmx_get_samples(eng._ctx, None, None, 2, 32) == INVALID
    a, b = eng.samples_device_ptrs()
    assert a and b and a != b
    check(eng, [img], None, [S.SampleRecord((40, 56), 32, offset=(2, 3))], 32)
