"""CPU: the COCO annotation reader and the NumPy mask contract of coco.py, and the ABI surface of pmx_coco_masks."""
import itertools
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, pkg

FIXTURE = os.path.join(GOLDEN, 'coco_annotations.json')


def _synthetic_annotations():
    """One annotation file as a dictionary: five images; key points drawn from a seeded generator.  Image 11 has a valid person, a small one
    and a crowd; 12 only people with too few key points; 13 two valid people; 14 no annotation at all; 15 one annotation of a large area with
    four key points."""
    rng = np.random.default_rng(5)

    def person(ann_id, img_id, num_kp, area, iscrowd=0, seg=None):
        kp = np.zeros((17, 3), dtype=np.int64)
        kp[:, :2] = rng.integers(0, 200, (17, 2))
        kp[:, 2] = rng.integers(0, 3, 17)
        if ann_id % 2:
            kp[5, 2], kp[6, 2] = 2, 1                 # both shoulders labelled: a neck
            kp[5, :2], kp[6, :2] = (101, 50), (60, 33)    # odd sums: the mean truncates
        return {'id': ann_id, 'image_id': img_id, 'category_id': 1, 'num_keypoints': num_kp, 'area': area, 'iscrowd': iscrowd,
                'keypoints': [int(v) for v in kp.reshape(-1)], 'segmentation': seg if seg is not None else [[10, 10, 50, 10, 50, 60, 10, 60]]}
    anns = [person(1, 11, 9, 5000.0), person(2, 13, 17, 1025.0), person(3, 11, 2, 40.0), person(4, 12, 4, 9000.0),
            person(5, 11, 0, 7000.0, iscrowd=1, seg={'counts': [100, 50, 240 * 320 - 150], 'size': [240, 320]}),
            person(6, 13, 5, 1024.5), person(7, 12, 3, 100.0), person(8, 15, 4, 1e5), person(9, 13, 5, 1024.0)]
    images = [{'id': i, 'file_name': '%012d.png' % i, 'height': 240, 'width': 320} for i in (15, 12, 11, 14, 13)]
    return {'images': images, 'annotations': anns, 'categories': [{'id': 1, 'name': 'person'}]}


class _StubCoco(object):
    """the few calls CocoDataLoader makes on a pycocotools COCO object, over the same dictionary"""

    def __init__(self, data):
        self.data = data

    def getCatIds(self, catNms=None):
        return [c['id'] for c in self.data['categories']]

    def getImgIds(self, catIds=None):
        return list({a['image_id'] for a in self.data['annotations'] if a['category_id'] in catIds})

    def getAnnIds(self, imgIds=None, iscrowd=None):
        return [a['id'] for a in self.data['annotations'] if a['image_id'] in imgIds]

    def loadAnns(self, ids):
        by_id = {a['id']: a for a in self.data['annotations']}
        return [by_id[i] for i in ids]

    def loadImgs(self, ids):
        by_id = {im['id']: im for im in self.data['images']}
        return [by_id[i] for i in ids]


def _ours(data):
    coco = pkg('coco')
    ds = coco.CocoKeypoints(data)
    out = {'img_ids': [int(i) for i in ds.img_ids], 'valid': {}, 'poses': {}}
    for i in ds.img_ids:
        valid = ds.valid_annotations(i)
        out['valid'][str(i)] = None if valid is None else [a['id'] for a in valid]
        out['poses'][str(i)] = None if valid is None else coco.parse_annotations(valid).tolist()
    return out


def test_reader_matches_the_recorded_reference_results():
    """parse_annotations / valid_annotations / the image id list against what the verbatim reference gave (recorded by the test below)."""
    assert _ours(_synthetic_annotations()) == json.load(open(FIXTURE))
    coco = pkg('coco')
    poses = coco.parse_annotations(_synthetic_annotations()['annotations'][:1])
    assert poses.dtype == np.int32 and poses.shape == (1, 18, 3) and list(poses[0, 1]) == [80, 41, 2]      # int(161 / 2), int(83 / 2)
    assert coco.parse_annotations([]).shape == (0, 18, 3)


def test_reader_matches_the_verbatim_reference(monkeypatch):
    from oracle import _refimport as R
    if not R.reference_available():
        pytest.skip('the reference is not present')
    CDL = R.import_reference_modules()['coco_data_loader']
    monkeypatch.setattr(CDL.cv2, 'imread', lambda *a: np.zeros((4, 4, 3), np.uint8))
    data = _synthetic_annotations()
    coco = pkg('coco')
    ds = coco.CocoKeypoints(data)
    ref = CDL.CocoDataLoader(_StubCoco(data), 368, mode='train')
    assert list(ref.imgIds) == list(ds.img_ids)
    got = {'img_ids': [int(i) for i in ref.imgIds], 'valid': {}, 'poses': {}}
    for i in ref.imgIds:
        _, _, anns, _ = ref.get_img_annotation(img_id=i)
        ours = ds.valid_annotations(i)
        assert (anns is None) == (ours is None)
        got['valid'][str(i)] = None if anns is None else [a['id'] for a in anns]
        got['poses'][str(i)] = None
        if anns is not None:
            assert [a['id'] for a in anns] == [a['id'] for a in ours]
            rp, op = ref.parse_coco_annotation(anns), coco.parse_annotations(ours)
            assert rp.dtype == op.dtype and rp.shape == op.shape and np.array_equal(rp, op)
            got['poses'][str(i)] = rp.tolist()
    assert got == json.load(open(FIXTURE))          # the recorded fixture is what the reference gives
    ev = CDL.CocoDataLoader(_StubCoco(data), 368, mode='eval')
    assert [a['id'] for a in ev.get_img_annotation(img_id=11)[2]] == [a['id'] for a in coco.CocoKeypoints(data, 'eval').example_annotations(11)]


def test_reader_reads_files_and_keeps_file_order(tmp_path):
    coco, ent = pkg('coco'), pkg('entity')
    data = _synthetic_annotations()
    p = tmp_path / 'ann.json'
    p.write_text(json.dumps(data))
    ds = coco.CocoKeypoints(str(p), mode='val')
    assert ds.img_ids == [11, 12, 13, 15] and len(ds) == 4            # 14 has no annotation
    assert [a['id'] for a in ds.annotations(11)] == [1, 3, 5] and ds.annotations(14) == []
    assert [a['id'] for a in ds.valid_annotations(13)] == [2, 6]     # area 1024 is not > 32 * 32
    assert ds.valid_annotations(12) is None and ds.valid_annotations(15) is None
    assert ds.size(11) == (240, 320) and ds.file_name(13) == '%012d.png' % 13
    assert ent.params['min_keypoints'] == 5 and ent.params['min_area'] == 32 * 32
    assert list(coco.mask_classes(ds.annotations(11))) == [coco.KEEP, coco.MISS, coco.CROWD]
    assert list(coco.mask_classes(ds.annotations(13))) == [coco.KEEP, coco.KEEP, coco.MISS]
    with pytest.raises(ValueError):
        coco.CocoKeypoints(data, mode='test')


# ---- the mask contract ----------------------------------------------------------------------------------------------------------------
def _box(x0, x1, y0, y1, h=12, w=10):
    m = np.zeros((h, w), np.uint8)
    m[y0:y1 + 1, x0:x1 + 1] = 1
    return m


def test_polygon_mask_hand_computed_cases():
    coco = pkg('coco')
    assert np.array_equal(coco.polygon_mask([2, 3, 7, 3, 7, 9, 2, 9], 12, 10), _box(2, 6, 3, 8))
    assert np.array_equal(coco.polygon_mask([2.5, 3.5, 7.5, 3.5, 7.5, 9.5, 2.5, 9.5], 12, 10), _box(3, 7, 4, 9))
    full = coco.polygon_mask([-3, -3, 20, -3, 20, 20, -3, 20], 12, 10)
    assert full.shape == (12, 10) and full.dtype == np.uint8 and full.sum() == 120
    # repeated vertices change nothing
    assert np.array_equal(coco.polygon_mask([2, 3, 2, 3, 7, 3, 7, 9, 7, 9, 7, 9, 2, 9], 12, 10), _box(2, 6, 3, 8))


def _even_odd(xy, h, w):
    """(inside by the even-odd rule at pixel centres (x, y), distance of every pixel centre to the nearest edge) -- written independently of
    the contract: a ray toward +x from each centre."""
    pts = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    inside = np.zeros((h, w), bool)
    dist = np.full((h, w), np.inf)
    for (x0, y0), (x1, y1) in zip(pts, np.roll(pts, -1, axis=0)):
        if y0 != y1:
            cross = ((y0 <= ys) != (y1 <= ys)) & (xs < x0 + (ys - y0) * (x1 - x0) / (y1 - y0))
            inside ^= cross
        ex, ey = x1 - x0, y1 - y0
        L2 = ex * ex + ey * ey
        t = np.clip(((xs - x0) * ex + (ys - y0) * ey) / L2, 0, 1) if L2 > 0 else np.zeros_like(xs)
        dist = np.minimum(dist, np.hypot(xs - (x0 + t * ex), ys - (y0 + t * ey)))
    return inside, dist


def test_polygon_mask_against_an_even_odd_pixel_centre_test():
    coco = pkg('coco')
    rng = np.random.default_rng(11)
    compared = total = 0
    for it in range(120):
        h, w = int(rng.integers(20, 48)), int(rng.integers(20, 48))
        k = int(rng.integers(3, 12))
        if it % 2:          # convex-ish, inside the image: sorted angles around the centre
            ang = np.sort(rng.uniform(0, 2 * np.pi, k))
            r = rng.uniform(0.25, 0.48, k)
            pts = np.stack([w / 2 + r * w * np.cos(ang), h / 2 + r * h * np.sin(ang)], axis=1)
        else:               # self-intersecting, reaching outside
            pts = rng.uniform(-0.4, 1.4, (k, 2)) * [w, h]
        xy = np.round(pts.reshape(-1), 2)
        xd, yd = coco.polygon_crossings(xy, h, w)
        assert np.all(np.bincount(xd, minlength=w) % 2 == 0), it          # even crossing counts per column
        mask = coco.polygon_mask(xy, h, w)
        inside, dist = _even_odd(xy, h, w)
        far = dist > 1.0
        assert np.array_equal(mask.astype(bool)[far], inside[far]), it
        compared += int(far.sum())
        total += h * w
    assert compared >= 0.5 * total, (compared, total)


def test_rle_mask_and_the_class_rule_in_sequence():
    coco = pkg('coco')
    h, w = 6, 5
    m = coco.rle_mask([0, 4, 10, 3, 13], h, w)          # column-major: pixels 0 .. 3 and 14 .. 16
    assert m.shape == (h, w) and m.sum() == 7
    assert list(np.nonzero(m.T.reshape(-1))[0]) == [0, 1, 2, 3, 14, 15, 16]
    with pytest.raises(ValueError):
        coco.rle_mask([1, 2, 3], h, w)
    a = [1, 1, 4, 1, 4, 5, 1, 5]            # x 1 .. 3, y 1 .. 4
    b = [2, 2, 5, 2, 5, 6, 2, 6]            # x 2 .. 4, y 2 .. 5
    A, B = coco.polygon_mask(a, 8, 8).astype(bool), coco.polygon_mask(b, 8, 8).astype(bool)
    assert (A & B).sum() == 6 and A.sum() == 12 and B.sum() == 12
    # a crowd part over an earlier keep part leaves the overlap out of miss ...
    miss, all_ = coco.masks_numpy(8, 8, [(coco.POLYGON, 0, coco.KEEP, a), (coco.POLYGON, 1, coco.CROWD, b)])
    assert miss.dtype == np.uint8 and np.array_equal(miss.astype(bool), B & ~A) and np.array_equal(all_.astype(bool), A | B)
    # ... the same parts in the other order do not
    miss, all_ = coco.masks_numpy(8, 8, [(coco.POLYGON, 0, coco.CROWD, b), (coco.POLYGON, 1, coco.KEEP, a)])
    assert np.array_equal(miss.astype(bool), B) and np.array_equal(all_.astype(bool), A | B)
    # a miss annotation goes in whole; two overlapping parts of ONE annotation are a union
    miss, all_ = coco.masks_numpy(8, 8, [(coco.POLYGON, 0, coco.KEEP, a), (coco.POLYGON, 1, coco.MISS, b)])
    assert np.array_equal(miss.astype(bool), B)
    miss, all_ = coco.masks_numpy(8, 8, [(coco.POLYGON, 0, coco.MISS, a), (coco.POLYGON, 0, coco.MISS, b)])
    assert np.array_equal(miss.astype(bool), A | B)
    miss, all_ = coco.masks_numpy(8, 8, [])
    assert not miss.any() and not all_.any() and miss.shape == (8, 8)


def test_mask_parts_flattens_and_refuses():
    coco = pkg('coco')

    def ann(seg, iscrowd=0, nk=9, area=5000.0):
        return {'segmentation': seg, 'iscrowd': iscrowd, 'num_keypoints': nk, 'area': area}
    parts = coco.mask_parts([ann([[1, 1, 5, 1, 5, 5], [2, 2, 6, 2, 6, 6, 2, 6]]), ann({'counts': [3, 4, 13], 'size': [4, 5]}, iscrowd=1),
                             ann([[0, 0, 3, 0, 3, 3]], nk=1)], 4, 5)
    assert [(p[0], p[1], p[2]) for p in parts] == [(coco.POLYGON, 0, coco.KEEP), (coco.POLYGON, 0, coco.KEEP), (coco.RLE, 1, coco.CROWD),
                                                   (coco.POLYGON, 2, coco.MISS)]
    assert parts[0][3].dtype == np.float64 and list(parts[0][3]) == [1, 1, 5, 1, 5, 5]
    assert parts[2][3].dtype == np.uint32 and list(parts[2][3]) == [3, 4, 13]
    bad = [{'counts': 'abc', 'size': [4, 5]},               # compressed counts
           [[1, 1, 5, 1]],                                  # four numbers: the library's box form, refused
           [[1, 1, 5, 1, 5, 5, 2]],                         # odd count
           [[1, 1, 5, 1, float('nan'), 5]], [[1, 1, 5, 1, float('inf'), 5]], [[1, 1, 5, 1, 65537, 5]], [[1, 1, 5, 1, 5, -65536.5]],
           {'counts': [3, 4, 13], 'size': [5, 4]},          # another image's size
           {'counts': [3, 4, 12], 'size': [4, 5]}]          # counts that do not fill the image
    for seg in bad:
        with pytest.raises(ValueError):
            coco.mask_parts([ann(seg)], 4, 5)
    assert len(coco.mask_parts([ann([[1, 1, 65536, 1, 5, -65536]])], 4, 5)) == 1


def test_mask_tables_and_abi_surface(native):
    lib = native.load()
    assert ('pmx_masks.hip', ['-ffp-contract=off']) in native.SOURCES
    assert 'pmx_coco_masks' in native.header_symbols() and hasattr(lib, 'pmx_coco_masks')
    assert len(lib._pmx_sig['pmx_coco_masks'][1]) == 12
    import ctypes as C
    assert C.sizeof(native.PmxMaskImage) == 16 and C.sizeof(native.PmxMaskPart) == 24
    assert native.coco_masks_strip(480) == 32 and native.coco_masks_strip(16384) >= 1 and native.coco_masks_strip(0) == 0
    coco = pkg('coco')
    images, parts, xy, counts = native.coco_mask_tables(
        [(4, 5), (3, 3), (2, 2)], [[(coco.POLYGON, 0, 0, [1, 1, 5, 1, 5, 5]), (coco.RLE, 1, 2, [3, 4, 13])], [],
                                   [(coco.RLE, 0, 1, [0, 4]), (coco.POLYGON, 1, 0, [0, 0, 2, 0, 2, 2, 0, 2])]])
    assert images.dtype == np.int32 and images.tolist() == [[4, 5, 0, 2], [3, 3, 2, 0], [2, 2, 2, 2]]
    assert parts.dtype == np.int32 and parts.tolist() == [[0, 0, 0, 0, 6, 0], [1, 1, 2, 0, 3, 0], [1, 0, 1, 3, 2, 0], [0, 1, 0, 6, 8, 0]]
    assert xy.dtype == np.float64 and xy.size == 14 and counts.dtype == np.uint32 and counts.tolist() == [3, 4, 13, 0, 4]
    with pytest.raises(ValueError):
        native.coco_mask_tables([(4, 5)], [[], []])
    with pytest.raises(ValueError):
        native.coco_mask_tables([], [])


def test_every_order_of_three_classes_differs_as_the_rule_says():
    """crowd, miss and keep over one another in all six orders (the cases the GPU test replays)"""
    coco = pkg('coco')
    polys = {coco.KEEP: [1, 1, 6, 1, 6, 6, 1, 6], coco.MISS: [3, 0, 8, 0, 8, 4, 3, 4], coco.CROWD: [0, 3, 9, 3, 9, 8, 0, 8]}
    M = {c: coco.polygon_mask(p, 10, 10).astype(bool) for c, p in polys.items()}
    for order in itertools.permutations([coco.KEEP, coco.MISS, coco.CROWD]):
        miss, all_ = coco.masks_numpy(10, 10, [(coco.POLYGON, i, c, polys[c]) for i, c in enumerate(order)])
        before = np.zeros((10, 10), bool)
        for c in order:
            if c == coco.CROWD:
                break
            before |= M[c]
        assert np.array_equal(miss.astype(bool), M[coco.MISS] | (M[coco.CROWD] & ~before)), order
        assert np.array_equal(all_.astype(bool), M[coco.KEEP] | M[coco.MISS] | M[coco.CROWD])
