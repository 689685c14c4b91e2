"""GPU: the result images drawn on the device (pmx_render; native.Engine.render, PoseDetector.draw_batch, demo.render_batch) against the
package's host functions, which are their contract: pose_detector.draw_person_pose, demo.add_weighted and demo.render.  Every comparison
is np.array_equal: there are no tolerances.  Shapes are the smallest that still break a wrong kernel (tiles are 64 x 16 pixels, the
primitives of an image are culled in chunks of 256)."""
import ctypes as C

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def _torch_runtime_first():
    """torch brings its own HIP runtime; it initialises only while the library's has not opened the device yet in this process (run alone,
    this module would otherwise create its engines first and the device-tensor tests could not allocate)."""
    import torch
    torch.cuda.init()


@pytest.fixture(scope='module')
def eng(native):
    e = native.Engine(0, max_batch=1, max_h=64, max_w=64)          # no weights: drawing needs none
    yield e
    e.close()


def _image(rng, h, w):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def _people(rng, n, h, w, lo=-20, pad=20):
    """n people with joints uniform over lo .. size + pad (some off the image: clipped limbs and discs), a third of the joints with v = 0,
    a few v that only round to 0 or to 1, and coordinates ending in .5 at even and odd integers (np.round: 10.5 -> 10, 11.5 -> 12)."""
    p = np.zeros((n, 18, 3))
    p[:, :, 0] = rng.uniform(lo, w + pad, (n, 18))
    p[:, :, 1] = rng.uniform(lo, h + pad, (n, 18))
    p[:, :, 2] = np.where(rng.random((n, 18)) < 1 / 3, 0, 2)
    if n:
        p[0, 0, :2], p[0, 1, :2] = (10.5, 11.5), (11.5, 10.5)
        p[0, 0, 2] = p[0, 1, 2] = 2
        p[-1, 2] = (w / 2 + 0.5, h / 2 - 0.5, 0.6)                  # v rounds to 1: drawn
        p[-1, 3] = (w / 2, h / 2, 0.5)                              # v rounds to 0 (half to even): not drawn
        p[-1, 5] = (w / 3, h / 3, -0.75)                            # v rounds to -1: drawn
    return p


def _host_pose(PD, img, poses, blend):
    canvas = PD.draw_person_pose(img, poses)
    return pkg('demo').add_weighted(img, 0.6, canvas, 0.4, 0) if blend else np.array(canvas, copy=True)


def _check_equal(got, want, what=''):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.uint8 and g.shape == w.shape, (what, k, g.shape, w.shape)
        bad = np.argwhere((g != w).any(axis=2))
        assert len(bad) == 0, '%s image %d: %d pixels differ, first (y, x) = %s: got %s, want %s' % (
            what, k, len(bad), bad[0], g[tuple(bad[0])], w[tuple(bad[0])])


# ---- 1. the pose layer, no blend ----------------------------------------------------------------------------------------------------
def test_pose_layer_equals_draw_person_pose(native):
    PD = pkg('pose_detector')
    rng = np.random.default_rng(101)
    imgs = [_image(rng, 37, 53), _image(rng, 64, 64), _image(rng, 45, 130)]     # no tile multiples; one wider than a tile row
    poses = [_people(rng, n, *im.shape[:2]) for n, im in zip((0, 1, 7), imgs)]
    assert [float(np.round(v)) for v in (10.5, 11.5)] == [10.0, 12.0]
    keep = [im.copy() for im in imgs]
    det = PD.PoseDetector(device=0)
    try:
        got = det.draw_batch(imgs, poses)
    finally:
        det.engine.close()
    want = [PD.draw_person_pose(im, p) for im, p in zip(imgs, poses)]
    assert want[0] is imgs[0] and got[0] is not imgs[0]             # nobody: the host hands the input back, the device an equal copy
    _check_equal(got, want, 'pose layer')
    assert any((w != im).any() for w, im in zip(want[1:], imgs[1:]))          # (something was drawn)
    _check_equal(imgs, keep, 'inputs untouched')


# ---- 2. the blend ---------------------------------------------------------------------------------------------------------------------
def test_blend_equals_add_weighted_on_all_levels(eng):
    """An image with all 256 levels in every channel.  Without people every pixel is blended with itself: on the host that is the
    identity for all 256 levels, and a multiply-add contracted on the device would not be."""
    PD = pkg('pose_detector')
    rng = np.random.default_rng(102)
    lv = np.arange(256, dtype=np.uint8)
    img = np.stack([np.tile(lv, 3), np.tile(np.roll(lv, 85), 3), np.tile(lv[::-1], 3)], axis=1).reshape(24, 32, 3)
    assert all(len(np.unique(img[:, :, ch])) == 256 for ch in range(3))
    people = _people(rng, 3, 24, 32, lo=-5, pad=5)
    want = [_host_pose(PD, img, people, True), _host_pose(PD, img, [], True)]
    assert np.array_equal(want[1], img)
    assert len(np.unique(want[0].reshape(-1, 3), axis=0)) > 256     # (drawn colours blended over many levels)
    _check_equal(eng.render([img, img], [people, np.zeros((0, 18, 3))], blend=True), want, 'blend')


# ---- 3. the parts ---------------------------------------------------------------------------------------------------------------------
def _keypoints(rng, n, bw, bh, missing):
    kps = [[float(rng.uniform(-4, bw + 4)), float(rng.uniform(-4, bh + 4)), np.float32(rng.random())] for _ in range(n)]
    for j in rng.choice(n, missing, replace=False):
        kps[j] = None
    return kps


def _person_parts(rng, face_box, left_box, right_box):
    part = lambda box, n, missing: None if box is None else {
        'bbox': box, 'keypoints': _keypoints(rng, n, box[2] - box[0], box[3] - box[1], missing)}
    return {'unit_length': 20.0, 'face': part(face_box, 70, 9), 'left': part(left_box, 21, 4), 'right': part(right_box, 21, 0)}


def test_parts_equal_demo_render(native):
    PD, demo = pkg('pose_detector'), pkg('demo')
    rng = np.random.default_rng(103)
    img = _image(rng, 96, 120)
    poses = _people(rng, 2, 96, 120, lo=0, pad=0)
    parts = [_person_parts(rng, (30, 10, 75, 55), (-12, -7, 25, 30), (90, 60, 140, 110)),        # negative left / top; partly outside
             _person_parts(rng, (50, 40, 100, 90), (5, 50, 45, 90), None)]
    img2 = _image(rng, 40, 70)                                      # a second image: its own people, one hand, in the same call
    poses2 = _people(rng, 1, 40, 70)
    parts2 = [_person_parts(rng, None, None, (20, 5, 60, 38))]
    want = [demo.render(img, poses, parts), demo.render(img2, poses2, parts2)]
    eng = native.Engine(0, max_batch=1, max_h=64, max_w=64, arch='handnet')
    det = object.__new__(PD.PoseDetector)
    det.engine = eng
    try:
        got = demo.render_batch(det, [img, img2], [poses, poses2], [parts, parts2])
        _check_equal(got, want, 'parts')
        # integer key points, as the detectors return them, and a person without any part
        ints = [{'unit_length': 1.0, 'face': None, 'right': None,
                 'left': {'bbox': (8, 9, 60, 70), 'keypoints': [[int(rng.integers(0, 52)), int(rng.integers(0, 61)), np.float32(0.5)] for _ in range(21)]}},
                {'unit_length': 1.0, 'face': None, 'left': None, 'right': None}]
        _check_equal(demo.render_batch(det, [img], [poses], [ints]), [demo.render(img, poses, ints)], 'integer key points')
    finally:
        eng.close()


# ---- 4. drawing order across cull chunks ----------------------------------------------------------------------------------------------
def test_order_across_cull_chunks(eng):
    """Forty people inside one 12 x 12 region: about 1 400 primitives on one tile, six chunks, so nearly every pixel of the region is
    decided by drawing order.  The second image's people lie in another tile: its primitives start at its own offset of the table."""
    PD = pkg('pose_detector')
    rng = np.random.default_rng(104)
    imgs = [_image(rng, 48, 80), _image(rng, 48, 80)]
    crowd = np.zeros((40, 18, 3))
    crowd[:, :, 0] = rng.uniform(30, 42, (40, 18))
    crowd[:, :, 1] = rng.uniform(10, 22, (40, 18))
    crowd[:, :, 2] = 2
    other = crowd[:5].copy()
    other[:, :, 0] += 36                                            # x 66 .. 78: the second tile column
    other[:, :, 1] += 20                                            # y 30 .. 42: the second and third tile rows
    for blend in (False, True):
        want = [_host_pose(PD, im, p, blend) for im, p in zip(imgs, (crowd, other))]
        _check_equal(eng.render(imgs, [crowd, other], blend=blend), want, 'crowd, blend %d' % blend)
    region = want[0][10:22, 30:42].reshape(-1, 3)
    assert len(np.unique(region, axis=0)) > 10


# ---- 5. degenerate geometry -----------------------------------------------------------------------------------------------------------
def test_degenerate_geometry(eng):
    PD = pkg('pose_detector')
    rng = np.random.default_rng(105)
    p = np.zeros((4, 18, 3))
    # person 0: Neck and RightWaist (limb 0) round to the same pixel: L2 == 0
    p[0, 1], p[0, 8] = (5.4, 3.2, 2), (4.6, 2.8, 2)
    # person 1: limb 1 (RightWaist - RightKnee) with one end at 10^6; limb 14 (Neck - Nose) from inside to far above left
    p[1, 8], p[1, 9] = (2, 1, 2), (1e6, 7e5, 2)
    p[1, 1], p[1, 0] = (30, 0, 2), (-1e6, -3e5, 2)
    # person 2: a limb (LeftWaist - LeftKnee) and its discs entirely off the image, on all four sides over the people
    p[2, 11], p[2, 12] = (-40, -9, 2), (-7, -30, 2)
    p[2, 2], p[2, 3] = (500, 10, 2), (500, 500, 2)
    # person 3: joints that are not drawn may hold anything
    p[3, 4] = (np.nan, np.inf, 0)
    p[3, 6] = (1e300, -1e300, 0.4)
    p[3, 7] = (0, 0, 2)
    imgs = [_image(rng, 1, 1), _image(rng, 1, 70), _image(rng, 70, 1), _image(rng, 33, 65)]
    with np.errstate(invalid='ignore'):
        for blend in (False, True):
            want = [_host_pose(PD, im, p, blend) for im in imgs]
            _check_equal(eng.render(imgs, [p] * 4, blend=blend), want, 'degenerate, blend %d' % blend)
    assert (want[3] != _host_pose(PD, imgs[3], [], True)).any()


# ---- 6. forms -------------------------------------------------------------------------------------------------------------------------
def _mixed_call(seed):
    rng = np.random.default_rng(seed)
    imgs = [_image(rng, 50, 90), _image(rng, 17, 64), _image(rng, 80, 33)]
    poses = [_people(rng, n, *im.shape[:2]) for n, im in zip((3, 0, 2), imgs)]
    parts = [[('hand', (10, 5, 60, 45), _keypoints(rng, 21, 50, 40, 3))], [('face', (-5, -5, 40, 12), _keypoints(rng, 70, 45, 17, 10))], []]
    return imgs, poses, parts


def test_device_images_mixed_sizes_and_repeat(eng):
    import torch
    imgs, poses, parts = _mixed_call(106)
    first = eng.render(imgs, poses, parts)
    _check_equal(eng.render(imgs, poses, parts), first, 'second run')
    for k in range(3):                                              # one call per image
        _check_equal(eng.render([imgs[k]], [poses[k]], [parts[k]]), [first[k]], 'image %d alone' % k)
    dev = [torch.from_numpy(im).cuda() for im in imgs]
    out = eng.render(dev, poses, parts)
    assert all(o.is_cuda and o.dtype == torch.uint8 for o in out)
    eng.synchronize()
    _check_equal([o.cpu().numpy() for o in out], first, 'device images')
    _check_equal([d.cpu().numpy() for d in dev], imgs, 'device inputs untouched')
    assert eng.render([], [], None) == []


def test_render_leaves_the_detection_state_alone(native):
    W = pkg('weights')
    rng = np.random.default_rng(107)
    e = native.Engine(0, max_batch=2, max_h=64, max_w=64)
    try:
        e.set_weights(W.synthetic_weights(0))
        batch = rng.integers(0, 256, (2, 64, 64, 3), dtype=np.uint8)
        e.detect_batch(batch, map_h=64, map_w=64)
        imgs, poses, parts = _mixed_call(108)
        drawn = e.render(imgs, poses, parts)
        rec, (paf, heat) = e.results(), e.get_maps()
        e.detect_batch(batch, map_h=64, map_w=64)
        rec0, (paf0, heat0) = e.results(), e.get_maps()
        assert rec.tobytes() == rec0.tobytes() and paf.tobytes() == paf0.tobytes() and heat.tobytes() == heat0.tobytes()
        plain = native.Engine(0, max_batch=1, max_h=64, max_w=64, arch='facenet')
        try:
            _check_equal(plain.render(imgs, poses, parts), drawn, 'facenet context')
        finally:
            plain.close()
    finally:
        e.close()


def test_render_buffers_go_with_the_context(native):
    """Contexts whose render buffers grew (an image far larger than the network input) give their device memory back: the free-memory
    reading after cycles 2, 3 and 4 is the same (cycle 1 also pays for what the runtime keeps for the process)."""
    import torch
    rng = np.random.default_rng(109)
    small, large = _image(rng, 30, 40), _image(rng, 600, 800)
    people = _people(rng, 2, 30, 40)
    free = []
    for cycle in range(4):
        e = native.Engine(0, max_batch=1, max_h=64, max_w=64, arch='handnet')
        try:
            e.render([small], [people])
            e.render([large, small], [people, people])
        finally:
            e.close()
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info(0)[0])
    assert max(free[1:]) == min(free[1:]), free


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------------
def _raw(native, e, images, poses=None, n_people=None, parts=(), kps=None, blend=1, n_images=None, n_parts=None):
    """pmx_render itself.  images: (array | None, h, w) per image; parts: (image, kind, left, top, right, bottom) rows.
    -> (return code, message, the canvases as one byte array)"""
    arr = (native.PmxBoxImage * max(1, len(images)))()
    keep, total = [], 0
    for k, (im, h, w) in enumerate(images):
        arr[k].bgr, arr[k].h, arr[k].w = (im.ctypes.data if im is not None else None), h, w
        keep.append(im)
        total += max(h, 0) * max(w, 0) * 3
    pt = (native.PmxRenderPart * max(1, len(parts)))()
    for k, row in enumerate(parts):
        pt[k].image, pt[k].kind, pt[k].left, pt[k].top, pt[k].right, pt[k].bottom = row
    poses = np.ascontiguousarray(poses if poses is not None else np.zeros((0, 18, 3)), dtype=np.float64)
    n_people = np.ascontiguousarray(n_people if n_people is not None else [0] * len(images), dtype=np.int32)
    kps = np.ascontiguousarray(kps if kps is not None else np.zeros((0, 4)), dtype=np.float64)
    out = np.zeros(max(total, 1), np.uint8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = e.lib.pmx_render(e._ctx, arr, len(images) if n_images is None else n_images, 0, ptr(poses), ptr(n_people), pt,
                          len(parts) if n_parts is None else n_parts, ptr(kps), blend, ptr(out), 0)
    return rc, e.lib.pmx_last_error().decode(), out[:total]


def _one_person(x=5.0, y=6.0, v=2.0, joint=4):
    p = np.zeros((1, 18, 3))
    p[0, joint] = (x, y, v)
    return p


def _hand_rows(x=3.0, y=4.0, point=7):
    r = np.zeros((21, 4))
    r[point] = (x, y, 0.5, 1)
    return r


def _error_cases():
    img = np.full((12, 20, 3), 7, np.uint8)
    ok = (img, 12, 20)
    hand = [(0, 1, 2, 2, 15, 10)]
    return [
        ('null image', dict(images=[ok, (None, 12, 20)]), 'image 1'),
        ('zero height', dict(images=[ok, ok, (img, 0, 20)]), 'image 2'),
        ('negative width', dict(images=[(img, 12, -20)]), 'image 0'),
        ('negative image count', dict(images=[ok], n_images=-1), 'n_images = -1'),
        ('negative people count', dict(images=[ok, ok], n_people=[0, -3]), 'image 1'),
        ('negative part count', dict(images=[ok], n_parts=-2), 'n_parts = -2'),
        ('part image index', dict(images=[ok], parts=[(1, 1, 2, 2, 15, 10)], kps=_hand_rows()), 'part 0'),
        ('negative part image index', dict(images=[ok], parts=hand + [(-1, 1, 2, 2, 15, 10)], kps=np.concatenate([_hand_rows()] * 2)), 'part 1'),
        ('part kind', dict(images=[ok], parts=[(0, 2, 2, 2, 15, 10)], kps=_hand_rows()), 'part 0'),
        ('parts without blend', dict(images=[ok], parts=hand, kps=_hand_rows(), blend=0), 'blend'),
        ('NaN joint', dict(images=[ok], poses=_one_person(x=np.nan), n_people=[1]), 'joint 4'),
        ('infinite joint', dict(images=[ok, ok], poses=_one_person(y=-np.inf, joint=17), n_people=[0, 1]), 'image 1, person 0, joint 17'),
        ('joint at 2^30', dict(images=[ok], poses=_one_person(x=-2.0 ** 30), n_people=[1]), 'joint 4'),
        ('NaN v', dict(images=[ok], poses=_one_person(v=np.nan), n_people=[1]), 'joint 4'),
        ('NaN key point', dict(images=[ok], parts=hand, kps=_hand_rows(y=np.nan)), 'part 0, key point 7'),
        ('key point at 2^30', dict(images=[ok], parts=hand, kps=_hand_rows(x=2.0 ** 30 - 2)), 'part 0, key point 7'),      # + left = 2^30
    ]


@pytest.mark.parametrize('case', _error_cases(), ids=[c[0] for c in _error_cases()])
def test_invalid_arguments_are_named_and_leave_the_context_usable(native, eng, case):
    PD, demo = pkg('pose_detector'), pkg('demo')
    _, kwargs, offender = case
    rc, msg, _ = _raw(native, eng, **kwargs)
    assert rc == 1 and offender in msg, (rc, msg)
    # a valid call right after: a person just below the coordinate limit, joints that are not drawn holding anything, one hand
    img = np.full((12, 20, 3), 7, np.uint8)
    p = _one_person(x=2.0 ** 30 - 1, y=3.0)
    p[0, 5] = (np.nan, 2.0 ** 40, 0)
    p[0, 1], p[0, 0] = (4, 5, 2), (15, 8, 2)
    rows = _hand_rows()
    rows[2] = (np.nan, np.inf, 0.0, 0.0)
    rc, msg, out = _raw(native, eng, [(img, 12, 20)], poses=p, n_people=[1], parts=[(0, 1, 2, 2, 15, 10)], kps=rows)
    assert rc == 0, msg
    with np.errstate(invalid='ignore'):
        want = demo.render(img, p, [{'face': None, 'right': None, 'left': {'bbox': (2, 2, 15, 10), 'keypoints': [
            [r[0], r[1], r[2]] if r[3] else None for r in rows.tolist()]}}])
    _check_equal([out.reshape(12, 20, 3)], [want], 'valid call after "%s"' % case[0])


def test_nothing_to_do_is_ok(native, eng):
    assert _raw(native, eng, [])[0] == 0
    assert _raw(native, eng, [], n_parts=0, blend=0)[0] == 0


# ---- 8. the CLI -----------------------------------------------------------------------------------------------------------------------
def test_cli_render_device_writes_the_same_png(native, tmp_path):
    """`pose_detector.py posenet weights.npz --img X --render device` against the default (host) drawing: the recipe of
    test_gpu_network.py::test_cli_end_to_end_with_npz_weights."""
    W, PD = pkg('weights'), pkg('pose_detector')
    weights = W.synthetic_weights(0)
    rng = np.random.default_rng(10)
    img = rng.integers(0, 256, (368, 368, 3), dtype=np.uint8)
    e = native.Engine(0, max_batch=1, max_h=368, max_w=368)
    try:
        e.set_weights(weights)
        e.forward_u8(img[None])
        paf, heat = e.get_maps()
    finally:
        e.close()
    npz = str(tmp_path / 'coco_posenet.npz')
    W.save_npz(npz, W.calibrate_head(weights, paf[0], heat[0]))
    png_in, png_host, png_dev = (str(tmp_path / n) for n in ('in.png', 'host.png', 'device.png'))
    PD.imwrite_bgr(png_in, img)
    assert PD.main(['posenet', npz, '--img', png_in, '--gpu', '0', '--out', png_host]) == 0
    assert PD.main(['posenet', npz, '--img', png_in, '--gpu', '0', '--out', png_dev, '--render', 'device']) == 0
    host, dev = PD.imread_bgr(png_host), PD.imread_bgr(png_dev)
    assert (host != img).any()                                      # people were found and drawn
    assert np.array_equal(host, dev)
    assert open(png_host, 'rb').read() == open(png_dev, 'rb').read()
