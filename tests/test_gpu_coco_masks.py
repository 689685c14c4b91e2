"""GPU: the ignore masks rasterised on the device (pmx_coco_masks; native.Engine.coco_masks, PoseDetector.ignore_masks, coco.batches) against
the package's NumPy contract (coco.masks_numpy), byte for byte, for mask_miss and mask_all; and the all-device input of prepare_samples.
Shapes are the smallest that still break a wrong kernel: a block owns a strip of 32 columns (for these heights) and keeps a column's bits
in 32-bit words."""
import ctypes as C
import itertools
import json

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

POLYGON, RLE, KEEP, MISS, CROWD = 0, 1, 0, 1, 2
INVALID, CAPACITY = 1, 5


@pytest.fixture(scope='module', autouse=True)
def _torch_runtime_first():
    """torch brings its own HIP runtime; it initialises only while the library's has not opened the device yet in this process."""
    import torch
    torch.cuda.init()


@pytest.fixture(scope='module')
def eng(native):
    e = native.Engine(0, max_batch=1, max_h=64, max_w=64, arch='handnet')          # any kind of context, no weights
    yield e
    e.close()


@pytest.fixture(scope='module')
def det():
    PD = pkg('pose_detector')
    d = PD.PoseDetector(weights=pkg('weights').synthetic_weights(0), device=0, max_batch=3, max_size=(64, 64))
    yield d
    d.engine.close()


def _rle(rng, h, w, runs):
    cuts = np.sort(rng.integers(0, h * w + 1, runs - 1))
    return np.diff(np.concatenate([[0], cuts, [h * w]])).astype(np.uint32)


def _random_parts(rng, h, w, n_ann):
    parts = []
    for a in range(n_ann):
        cls = int(rng.integers(0, 3))
        for _ in range(int(rng.integers(1, 3))):
            if rng.random() < 0.25:
                parts.append((RLE, a, cls, _rle(rng, h, w, int(rng.integers(1, 9)))))
            else:
                k = int(rng.integers(3, 12))
                pts = rng.uniform(-0.3, 1.3, (k, 2)) * [w, h]
                parts.append((POLYGON, a, cls, np.round(pts.reshape(-1), int(rng.integers(0, 3)))))
    return parts


def _want(sizes, parts_per_image):
    coco = pkg('coco')
    return [coco.masks_numpy(h, w, p) for (h, w), p in zip(sizes, parts_per_image)]


def _check(eng, sizes, parts_per_image, want=None):
    want = _want(sizes, parts_per_image) if want is None else want
    miss, all_ = eng.coco_masks(sizes, parts_per_image)
    assert len(miss) == len(all_) == len(sizes)
    for k, (h, w) in enumerate(sizes):
        for name, got, ref in (('miss', miss[k], want[k][0]), ('all', all_[k], want[k][1])):
            assert got.shape == (h, w) and got.dtype == bool, (name, k, got.shape, got.dtype)
            bad = np.argwhere(got != ref.astype(bool))
            assert len(bad) == 0, 'image %d (%d x %d), mask_%s: %d pixels differ, first (y, x) = %s' % (k, h, w, name, len(bad), bad[0])
    return miss, all_


@pytest.mark.parametrize('h', [1, 31, 32, 33, 64, 65])
def test_heights_around_a_word_and_widths_around_a_strip(native, eng, h):
    strip = native.coco_masks_strip(h)
    assert strip == 32
    rng = np.random.default_rng(100 + h)
    sizes = [(h, w) for w in (1, 2, strip, strip + 1)]
    parts = []
    for _, w in sizes:
        p = [(POLYGON, 0, MISS, [-2, -2, w + 2, -2, w + 2, h + 2, -2, h + 2]),                      # everything: bit h of every column is toggled
             (POLYGON, 1, KEEP, [0, 0, w, 0, w, h, 0, h]), (RLE, 2, CROWD, _rle(rng, h, w, 6))]
        parts.append(p[1:] + [(k, a + 3, c, d) for k, a, c, d in _random_parts(rng, h, w, 3)] + [(p[0][0], 6) + p[0][2:]])
    miss, all_ = _check(eng, sizes, parts)
    assert all(m.all() for m in all_)


def test_one_call_mixes_three_sizes_and_an_image_without_parts(eng):
    rng = np.random.default_rng(7)
    sizes = [(40, 70), (9, 3), (5, 5), (66, 33)]
    parts = [_random_parts(rng, 40, 70, 4), _random_parts(rng, 9, 3, 2), [], _random_parts(rng, 66, 33, 5)]
    miss, all_ = _check(eng, sizes, parts)
    assert not miss[2].any() and not all_[2].any() and all_[0].any()


H, W = 37, 41          # one strip border at column 32


def _circle(n, cx, cy, r, jitter, seed):
    rng = np.random.default_rng(seed)
    ang = np.linspace(0, 2 * np.pi, n, endpoint=False)
    rad = r + rng.uniform(-jitter, jitter, n)
    return np.round(np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1).reshape(-1), 2)


GEOMETRY = {
    'outside_left': [(POLYGON, 0, MISS, [-20, 5, -3, 5, -3, 30, -20, 30])],
    'outside_right': [(POLYGON, 0, MISS, [W + 3, 5, W + 20, 5, W + 20, 30, W + 3, 30])],
    'outside_above': [(POLYGON, 0, MISS, [5, -30, 30, -30, 30, -3, 5, -3])],
    'outside_below': [(POLYGON, 0, MISS, [5, H + 3, 30, H + 3, 30, H + 30, 5, H + 30])],
    'clamped_to_0_and_h': [(POLYGON, 0, MISS, [3.3, -50, 38.2, -9, 36, H + 70, 2, H + 0.4])],
    'far_outside_vertices': [(POLYGON, 0, MISS, [-60000, -60000, 65536, -3000, 100, 65536, -65536, 200])],
    'repeated_vertices': [(POLYGON, 0, MISS, [4, 4, 4, 4, 35, 6, 35, 6, 35, 6, 20, 33, 20, 33, 4, 4])],
    'steep_and_shallow': [(POLYGON, 0, MISS, [10, 1, 13.4, 35, 8.2, 30]), (POLYGON, 1, MISS, [1, 20, 39, 22.6, 30, 25.2])],
    'diagonals_in_four_directions': [(POLYGON, 0, MISS, [20, 2, 36, 18, 20, 34, 4, 18]), (POLYGON, 1, KEEP, [20.4, 8.4, 10.4, 18.4, 20.4, 28.4, 30.4, 18.4])],
    'negative_coordinates': [(POLYGON, 0, MISS, [-3.7, -2.2, 12.3, 5.5, -1.4, 20.9]), (POLYGON, 1, MISS, [-0.3, 30.1, 8, 25, -0.7, 36.2, -7.5, 31])],
    'columns_0_and_w_minus_1': [(POLYGON, 0, MISS, [0, 1, W, 1, W, 5, 0, 5]), (POLYGON, 1, MISS, [0.4, 10, W - 0.6, 10, W - 0.6, 15, 0.4, 15])],
    'overlapping_parts_of_one_annotation': [(POLYGON, 0, MISS, [5, 5, 25, 5, 25, 25, 5, 25]), (POLYGON, 0, MISS, [15, 15, 39, 15, 39, 35, 15, 35])],
    'polygon_of_300_vertices': [(POLYGON, 0, MISS, _circle(300, 20, 18, 15, 2.5, 3))],
    'rle_with_an_empty_first_run': [(RLE, 0, MISS, [0, 5, H * W - 5])],
    'rle_runs_over_columns_and_the_strip_border': [(RLE, 0, MISS, [7, H * 3 + 2, 11, H * 30, 3, 1, 1, H * W - (7 + H * 3 + 2 + 11 + H * 30 + 5)])],
    'rle_of_single_pixels': [(RLE, 0, MISS, [1] * (H * W))],
    'rle_all_ones': [(RLE, 0, MISS, [0, H * W])],
}


@pytest.mark.parametrize('name', sorted(GEOMETRY))
def test_geometry(eng, name):
    miss, all_ = _check(eng, [(H, W)], [GEOMETRY[name]])
    if name.startswith('outside'):
        assert not all_[0].any()
    elif name == 'overlapping_parts_of_one_annotation':
        assert all_[0][20, 20] and all_[0].sum() == 20 * 20 + 24 * 20 - 10 * 10
    elif name == 'columns_0_and_w_minus_1':
        # x = 0.4 scales to 2 = 5 * 0 + 2: the crossing of column 0 itself; x = w - 0.6 scales to 5 w - 3: column w - 1 stays out
        assert all_[0][2, 0] and all_[0][2, W - 1] and all_[0][12, 0] and all_[0][12, W - 2] and not all_[0][12, W - 1]
    else:
        assert all_[0].any()


def test_crowd_miss_and_keep_in_every_order(eng):
    polys = {KEEP: [1, 1, 26, 1, 26, 26, 1, 26], MISS: [13, 0, 38, 0, 38, 14, 13, 14], CROWD: [0, 9.5, 40, 9.5, 40, 30, 0, 30]}
    orders = list(itertools.permutations([KEEP, MISS, CROWD]))
    parts = [[(POLYGON, i, c, polys[c]) for i, c in enumerate(order)] for order in orders]
    miss, _ = _check(eng, [(H, W)] * 6, parts)
    assert len({m.tobytes() for m in miss}) == 2          # what matters is whether the keep annotation came before the crowd


def test_random_batch_repeats_and_device_output(native, eng):
    import torch
    rng = np.random.default_rng(23)
    sizes = [(int(rng.integers(1, 97)), int(rng.integers(1, 97))) for _ in range(8)]
    parts = [_random_parts(rng, h, w, int(rng.integers(0, 7))) for h, w in sizes]
    want = _want(sizes, parts)
    first = _check(eng, sizes, parts, want)
    second = _check(eng, sizes, parts, want)
    assert all(np.array_equal(a, b) for x, y in zip(first, second) for a, b in zip(x, y))
    dm, da = eng.coco_masks(sizes, parts, device=True)
    eng.synchronize()
    for k in range(8):
        assert dm[k].is_cuda and dm[k].dtype == torch.uint8 and tuple(dm[k].shape) == sizes[k]
        assert np.array_equal(dm[k].cpu().numpy(), want[k][0]) and np.array_equal(da[k].cpu().numpy(), want[k][1])
    # either output alone
    images, tab, xy, counts = native.coco_mask_tables(sizes, parts)
    total = sum(h * w for h, w in sizes)
    for which in (0, 1):
        out = np.full(total, 9, np.uint8)
        ptrs = [None, None]
        ptrs[which] = native._ptr(out)
        eng._check(eng.lib.pmx_coco_masks(eng._ctx, native._ptr(images), len(images), native._ptr(tab), len(tab), native._ptr(xy), xy.size,
                                          native._ptr(counts), counts.size, ptrs[0], ptrs[1], 0))
        assert np.array_equal(out, np.concatenate([w[which].reshape(-1) for w in want]))


def test_a_context_on_the_callers_stream_gives_the_same_bytes(eng):
    import torch
    rng = np.random.default_rng(29)
    sizes = [(50, 45), (33, 64)]
    parts = [_random_parts(rng, h, w, 4) for h, w in sizes]
    want = _want(sizes, parts)
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    eng.set_stream(stream.cuda_stream)
    try:
        _check(eng, sizes, parts, want)
        dm, da = eng.coco_masks(sizes, parts, device=True)
        stream.synchronize()
        assert all(np.array_equal(dm[k].cpu().numpy(), want[k][0]) and np.array_equal(da[k].cpu().numpy(), want[k][1]) for k in range(2))
    finally:
        eng.set_stream(0)


def test_error_codes_leave_the_context_usable(native, eng):
    lib = eng.lib
    h, w = 6, 5
    poly = [1, 1, 4, 1, 4, 5, 1, 5]
    out = np.zeros(2 * h * w, np.uint8)

    def call(images, parts, xy, counts, n_images=None, miss=True, all_=True, null=()):
        images = np.ascontiguousarray(images, np.int32).reshape(-1, 4)
        parts = np.ascontiguousarray(parts, np.int32).reshape(-1, 6)
        xy = np.ascontiguousarray(xy, np.float64)
        counts = np.ascontiguousarray(counts, np.uint32)
        rc = lib.pmx_coco_masks(eng._ctx, None if 'images' in null else native._ptr(images), len(images) if n_images is None else n_images,
                                None if 'parts' in null else native._ptr(parts), len(parts), None if 'xy' in null else native._ptr(xy), xy.size,
                                None if 'counts' in null else native._ptr(counts), counts.size,
                                native._ptr(out[:h * w]) if miss else None, native._ptr(out[h * w:]) if all_ else None, 0)
        assert rc == 0 or lib.pmx_last_error().decode().strip()
        return rc

    img = [h, w, 0, 1]
    good = [0, 0, 1, 0, 8, 0]
    assert call([img], [good], poly, []) == 0
    bad = [
        dict(images=[img], parts=[good], xy=poly, counts=[], null=('images',)),
        dict(images=[img], parts=[good], xy=poly, counts=[], null=('parts',)),
        dict(images=[img], parts=[good], xy=poly, counts=[], null=('xy',)),
        dict(images=[img], parts=[[1, 0, 1, 0, 2, 0]], xy=[], counts=[10, 20], null=('counts',)),
        dict(images=[img], parts=[good], xy=poly, counts=[], n_images=0),
        dict(images=[img], parts=[good], xy=poly, counts=[], n_images=-1),
        dict(images=[img], parts=[good], xy=poly, counts=[], miss=False, all_=False),
        dict(images=[[0, w, 0, 1]], parts=[good], xy=poly, counts=[]),
        dict(images=[[h, 16385, 0, 1]], parts=[good], xy=poly, counts=[]),
        dict(images=[[h, w, 0, 2]], parts=[good], xy=poly, counts=[]),                      # part range past the table
        dict(images=[[h, w, -1, 1]], parts=[good], xy=poly, counts=[]),
        dict(images=[[h, w, 0, 3]], parts=[[0, 1, 1, 0, 8, 0], [0, 0, 1, 0, 8, 0], [0, 1, 1, 0, 8, 0]], xy=poly, counts=[]),      # not consecutive
        dict(images=[[h, w, 0, 2]], parts=[[0, 0, 1, 0, 8, 0], [0, 0, 2, 0, 8, 0]], xy=poly, counts=[]),                          # two classes
        dict(images=[img], parts=[[2, 0, 1, 0, 8, 0]], xy=poly, counts=[]),                 # kind
        dict(images=[img], parts=[[0, 0, 3, 0, 8, 0]], xy=poly, counts=[]),                 # class
        dict(images=[img], parts=[[0, 0, 1, 0, 4, 0]], xy=poly, counts=[]),                 # fewer than 6 numbers
        dict(images=[img], parts=[[0, 0, 1, 0, 7, 0]], xy=poly, counts=[]),                 # odd
        dict(images=[img], parts=[[0, 0, 1, 2, 8, 0]], xy=poly, counts=[]),                 # past the vertex array
        dict(images=[img], parts=[good], xy=[1, 1, 4, 1, float('nan'), 5, 1, 5], counts=[]),
        dict(images=[img], parts=[good], xy=[1, 1, 4, 1, float('inf'), 5, 1, 5], counts=[]),
        dict(images=[img], parts=[good], xy=[1, 1, 4, 1, 65536.5, 5, 1, 5], counts=[]),
        dict(images=[img], parts=[[1, 0, 1, 0, 2, 0]], xy=[], counts=[10, 21]),             # counts that do not sum to h * w
        dict(images=[img], parts=[[1, 0, 1, 0, 3, 0]], xy=[], counts=[10, 20]),             # past the counts array
    ]
    for kw in bad:
        out[:] = 7
        assert call(**kw) == INVALID, kw
        assert (out == 7).all()                                                             # nothing was enqueued
    # the table budget: a (valid) polygon whose vertices alone exceed it
    big = np.zeros((64 << 20) // 8 + 8)
    assert call([img], [[0, 0, 1, 0, big.size, 0]], big, []) == CAPACITY
    assert (out == 7).all()
    with pytest.raises(ValueError):
        eng.coco_masks([(h, w)], [[], []])
    _check(eng, [(h, w)], [[(POLYGON, 0, CROWD, poly), (RLE, 1, MISS, [3, 4, 23])]])


# ---- the way into training ------------------------------------------------------------------------------------------------------------
def _annotations(rng, h, w, n, valid=True):
    anns = []
    for i in range(n):
        k = int(rng.integers(3, 9))
        seg = [[float(v) for v in np.round((rng.uniform(-0.2, 1.2, (k, 2)) * [w, h]).reshape(-1), 1)]]
        kp = np.zeros((17, 3), np.int64)
        kp[:, 0], kp[:, 1], kp[:, 2] = rng.integers(0, w, 17), rng.integers(0, h, 17), rng.integers(0, 3, 17)
        cls = i % 3
        anns.append({'segmentation': seg if cls != 2 else {'counts': [int(v) for v in _rle(rng, h, w, 5)], 'size': [h, w]},
                     'iscrowd': int(cls == 2), 'num_keypoints': 9 if (cls == 0 and valid) else 2, 'area': 5000.0,
                     'keypoints': [int(v) for v in kp.reshape(-1)]})
    return anns


def _rotation(S, w, h, degree):
    """random_rotate_img's matrix and rotated size (coco_data_loader.py:88-101) for a fixed angle"""
    rad = degree * np.pi / 180
    R = S.rotation_matrix((w / 2, h / 2), degree, 1)
    bbox = (w * abs(np.cos(rad)) + h * abs(np.sin(rad)), w * abs(np.sin(rad)) + h * abs(np.cos(rad)))
    R[0, 2] += bbox[0] / 2 - w / 2
    R[1, 2] += bbox[1] / 2 - h / 2
    return R, (int(bbox[0] + 0.5), int(bbox[1] + 0.5))


def test_prepare_samples_takes_device_images_and_device_masks(det):
    import torch
    S, coco = pkg('samples'), pkg('coco')
    rng = np.random.default_rng(41)
    sizes = [(24, 40), (96, 72), (64, 64)]
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    anns = [_annotations(rng, h, w, 3) for h, w in sizes]
    poses = [coco.parse_annotations(a[:1]) for a in anns]
    host_masks = det.ignore_masks(anns, sizes)
    want = [coco.masks_numpy(h, w, coco.mask_parts(a, h, w))[0].astype(bool) for a, (h, w) in zip(anns, sizes)]
    assert all(np.array_equal(m, r) for m, r in zip(host_masks, want)) and any(m.any() for m in host_masks)
    dev_masks = det.ignore_masks(anns, sizes, device=True)
    dev_imgs = [torch.from_numpy(im).cuda() for im in imgs]
    assert all(m.is_cuda and m.dtype == torch.uint8 for m in dev_masks)
    R, size = _rotation(S, 72, 96, 20.0)
    recs = [S.SampleRecord((24, 40), 64, offset=(-5, 4), distort=(10, 40, -30), flip=True),
            S.SampleRecord((96, 72), 64, R=R, rotated=size, offset=(20, 30), distort=(3, -9, 12)),
            S.SampleRecord((64, 64), 64, resized=(70, 66), offset=(-4, 2), flip=True)]
    for kw in (dict(mode='val'), dict(mode='train', records=recs)):
        hi, hp, hm = det.prepare_samples(imgs, poses, host_masks, insize=64, **kw)
        di, dp, dm = det.prepare_samples(dev_imgs, poses, dev_masks, insize=64, **kw)
        assert np.array_equal(hi, di) and np.array_equal(hm, dm) and all(np.array_equal(a, b) for a, b in zip(hp, dp)), kw
        assert hm.any()
    hi, _, hm = det.prepare_samples(imgs, poses, [host_masks[0], None, host_masks[2]], insize=64)
    di, _, dm = det.prepare_samples(dev_imgs, poses, [dev_masks[0], None, dev_masks[2]], insize=64)
    assert np.array_equal(hi, di) and np.array_equal(hm, dm)
    for bad in ((imgs, dev_masks), (dev_imgs, host_masks), ([dev_imgs[0], imgs[1], dev_imgs[2]], None)):
        with pytest.raises(ValueError):
            det.prepare_samples(bad[0], poses, bad[1], insize=64)


def test_batches_from_an_annotation_file_feed_validation_loss(det, tmp_path):
    PD, coco = pkg('pose_detector'), pkg('coco')
    rng = np.random.default_rng(43)
    sizes = {3: (48, 80), 5: (72, 56), 9: (64, 64)}
    data = {'images': [], 'annotations': [], 'categories': [{'id': 1, 'name': 'person'}]}
    pixels = {}
    for img_id, (h, w) in sizes.items():
        data['images'].append({'id': img_id, 'file_name': 'im%d.png' % img_id, 'height': h, 'width': w})
        pixels[img_id] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        PD.imwrite_bgr(str(tmp_path / ('im%d.png' % img_id)), pixels[img_id])
        for a in _annotations(rng, h, w, 3, valid=img_id != 5):          # image 5 has no valid annotation
            data['annotations'].append(dict(a, id=len(data['annotations']) + 1, image_id=img_id, category_id=1))
    (tmp_path / 'ann.json').write_text(json.dumps(data))
    ds = coco.CocoKeypoints(str(tmp_path / 'ann.json'), mode='val')
    assert ds.img_ids == [3, 5, 9] and ds.valid_annotations(5) is None

    class Draws(object):
        def __init__(self):
            self.asked = []

        def randint(self, n):
            self.asked.append(n)
            return [1, 2][len(self.asked) - 1]          # first image 5 again (still nothing valid), then image 9

    draws = Draws()
    out = list(coco.batches(ds, det, str(tmp_path), 2, insize=64, mode='val', rng=draws))
    assert draws.asked == [3, 3] and [len(t[0]) for t in out] == [2, 1]
    for imgs, poses, masks in out:
        assert imgs.dtype == np.uint8 and imgs.shape[1:] == (64, 64, 3) and masks.dtype == bool and masks.shape == (len(imgs), 64, 64)
        loss = det.validation_loss(imgs, poses, masks)
        assert np.isfinite(loss['val/loss']) and loss['val/loss'] > 0
    # the triples are those of the host path on the same files; the image without valid annotations was replaced by image 9
    ids = [3, 9, 9]
    host_masks = [coco.masks_numpy(*sizes[i], coco.mask_parts(ds.annotations(i), *sizes[i]))[0] for i in ids]
    hi, hp, hm = det.prepare_samples([pixels[i] for i in ids], [coco.parse_annotations(ds.valid_annotations(i)) for i in ids], host_masks, insize=64)
    assert np.array_equal(np.concatenate([t[0] for t in out]), hi) and np.array_equal(np.concatenate([t[2] for t in out]), hm)
    assert all(np.array_equal(a, b) for a, b in zip([p for t in out for p in t[1]], hp)) and hm.any()
