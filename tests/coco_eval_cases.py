"""Helper of tests/test_coco_eval_host.py and tests/test_gpu_coco_eval.py, not collected itself: the hand-built matching cases with their
expected tables written out, and the seeded generator of the images the device entry is compared on.  Nothing here imports the package:
the joint mapping and the sigmas are written out again.

An image is (poses (n, 18, 3) float64, scores (n,), annotations): what a detector returns and the annotation dictionaries of the file.

The generated images: detections are jittered copies of ground truths (several per ground truth, so that the walks compete), copies without
jitter, and strays; scores come from a coarse grid, so ties are common; ground truths carry crowd flags, num_keypoints == 0 with and
without labelled points (the box branch of the OKS), bit-identical duplicates, and areas on and around 32**2 and 96**2.  The host test
asserts the margins the equality of the tables rests on (every OKS at least 1e-9 from every threshold; two OKS above 0.4 of one detection
bit-equal or 1e-9 apart): the two sides' exp differ by about an ulp."""
import functools

import numpy as np

# COCO key point i -> row of an (18, 3) pose: Nose, LeftEye, RightEye, LeftEar, RightEar, LeftShoulder, RightShoulder, LeftElbow,
# RightElbow, LeftHand, RightHand, LeftWaist, RightWaist, LeftKnee, RightKnee, LeftFoot, RightFoot
JOINT_OF_COCO = [0, 15, 14, 17, 16, 5, 2, 6, 3, 7, 4, 11, 8, 12, 9, 13, 10]
NECK = 1
SIGMAS = [.026, .025, .025, .035, .035, .079, .079, .072, .072, .062, .062, .107, .107, .087, .087, .089, .089]
THRS = [0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95]
MAX_GT = 512

DETS = (0, 1, 2, 20, 21, 25)
GTS = (0, 1, 2, 17, 64, MAX_GT)


def pose_of(kps17, neck=(7.0, 9.0)):
    """(17, 2) or (17, 3) COCO points -> one (18, 3) pose row block: (x, y, 2) per point, (0, 0, 0) where a third column is 0; the neck
    is set too (the evaluation must drop it)"""
    kps17 = np.asarray(kps17, dtype=np.float64)
    pose = np.zeros((18, 3))
    for i, j in enumerate(JOINT_OF_COCO):
        if kps17.shape[1] == 2 or kps17[i, 2] != 0:
            pose[j] = (kps17[i, 0], kps17[i, 1], 2)
    pose[NECK] = (neck[0], neck[1], 2)
    return pose


def annotation(kps17, area, bbox=None, iscrowd=0, num_keypoints=None, v=2):
    """an annotation dictionary from (17, 2) points (all with visibility v) or (17, 3) rows"""
    kps17 = np.asarray(kps17, dtype=np.float64)
    if kps17.shape[1] == 2:
        kps17 = np.concatenate([kps17, np.full((17, 1), float(v))], axis=1)
    if bbox is None:
        x, y = kps17[:, 0], kps17[:, 1]
        bbox = [float(x.min()), float(y.min()), float(x.max() - x.min()), float(y.max() - y.min())]
    n = int(np.count_nonzero(kps17[:, 2] > 0)) if num_keypoints is None else int(num_keypoints)
    return {'keypoints': [float(t) for t in kps17.reshape(-1)], 'area': float(area), 'bbox': [float(t) for t in bbox],
            'iscrowd': int(iscrowd), 'num_keypoints': n, 'category_id': 1}


def grid_points(x0, y0, step=10.0):
    """17 distinct points on a grid from (x0, y0)"""
    return np.array([[x0 + step * (i % 5), y0 + step * (i // 5)] for i in range(17)], dtype=np.float64)


def shift_for_oks(target, area):
    """the common shift d of all 17 points (dx = d, dy = 0) that gives an OKS of about `target` against a ground truth of that area: bisection
    on mean_i exp(-d^2 / (8 sigma_i^2 area))"""
    lo, hi = 0.0, 1e4
    for _ in range(200):
        mid = (lo + hi) / 2
        v = np.mean([np.exp(-mid * mid / (8 * s * s * area)) for s in SIGMAS])
        lo, hi = (mid, hi) if v > target else (lo, mid)
    return lo


def _t(*rows):
    return np.array(rows)


def hand_cases():
    """name -> (poses, scores, annotations, expected): expected holds 'order', 'dt_match' / 'dt_ig' as {(range, threshold index): row} for
    the cells written out (or a (3, 10, D) array), 'gt_ig' (3, G)."""
    P = grid_points(100, 100)
    A = 5000.0          # an area inside 'all' and 'medium' (1024 .. 9216), outside 'large'
    cases = {}
    all10 = lambda row: np.tile(np.array(row), (10, 1))

    # two bit-identical ground truths: the later one wins (an equal value replaces the earlier one); the second detection takes the
    # first.  In 'large' both ground truths are ignored (area 5000 < 9216); the detections match them all the same (ignored ones are
    # visited last but are all there is) and carry their ignore flag
    cases['identical_ground_truths'] = (
        np.stack([pose_of(P), pose_of(P)]), np.array([0.9, 0.8]), [annotation(P, A), annotation(P, A)],
        dict(order=[0, 1], dt_match=np.stack([all10([1, 0]), all10([1, 0]), all10([1, 0])]),
             dt_ig=np.stack([all10([0, 0]), all10([0, 0]), all10([1, 1])]), gt_ig=_t([0, 0], [0, 0], [1, 1])))

    # a crowd ground truth is matched by every detection near it and stays available
    cases['crowd_matched_three_times'] = (
        np.stack([pose_of(P), pose_of(P + [1, 0]), pose_of(P + [0, 1])]), np.array([3.0, 2.0, 1.0]), [annotation(P, A, iscrowd=1)],
        dict(order=[0, 1, 2], dt_match={(0, 0): [0, 0, 0], (1, 0): [0, 0, 0], (2, 0): [0, 0, 0]},
             dt_ig={(0, 0): [1, 1, 1], (1, 0): [1, 1, 1], (2, 0): [1, 1, 1]}, gt_ig=_t([1], [1], [1])))

    # early stop: the kept ground truth (file index 1, OKS about 0.575) is taken although the ignored one (file index 0, crowd, OKS 1) is
    # better -- the walk visits kept ones first and stops at the first ignored one once it holds a kept match.  From the threshold 0.6
    # on the kept one fails and the crowd is matched.
    far = P + [shift_for_oks(0.575, A), 0]
    cases['kept_preferred_over_ignored'] = (
        pose_of(P)[None], np.array([1.0]), [annotation(P, A, iscrowd=1), annotation(far, A)],
        dict(order=[0], dt_match={(0, 0): [1], (0, 1): [1], (0, 2): [0], (0, 9): [0]}, dt_ig={(0, 0): [0], (0, 1): [0], (0, 2): [1], (0, 9): [1]},
             gt_ig=_t([1, 0], [1, 0], [1, 1])))

    # ground-truth areas exactly 32**2 and 96**2 lie inside both neighbouring ranges
    Q = grid_points(400, 100)
    cases['areas_on_the_range_borders'] = (
        np.zeros((0, 18, 3)), np.zeros(0), [annotation(P, 32 ** 2), annotation(Q, 96 ** 2), annotation(Q, 32 ** 2 - 0.5), annotation(Q, 96 ** 2 + 0.5)],
        dict(order=[], gt_ig=_t([0, 0, 0, 0], [0, 0, 1, 1], [1, 0, 1, 0])))

    # a detection whose area (40 x 30 = 1200 from grid_points with step 10: x spans 40, y spans 30) is inside 'medium' and outside 'large':
    # unmatched it is ignored in 'large' only; matched (to a ground truth that 'large' ignores) it takes the ground truth's flag
    cases['detection_area_outside_unmatched'] = (
        pose_of(P)[None], np.array([1.0]), [annotation(Q, 20000.0)],
        dict(order=[0], areas=[1200.0], dt_match=np.full((3, 10, 1), -1), dt_ig=np.stack([all10([0]), all10([0]), all10([1])]),
             gt_ig=_t([0], [1], [0])))
    cases['detection_area_outside_matched'] = (
        pose_of(P)[None], np.array([1.0]), [annotation(P, 20000.0)],
        dict(order=[0], areas=[1200.0], dt_match=np.zeros((3, 10, 1), int), dt_ig=np.stack([all10([0]), all10([1]), all10([0])]),
             gt_ig=_t([0], [1], [0])))

    # num_keypoints == 0 (taken from the field): ignored everywhere, though its points are labelled
    cases['num_keypoints_zero'] = (
        pose_of(P)[None], np.array([1.0]), [annotation(P, A, num_keypoints=0)],
        dict(order=[0], dt_match=np.zeros((3, 10, 1), int), dt_ig=np.ones((3, 10, 1), int), gt_ig=_t([1], [1], [1])))

    # detections and no ground truth: unmatched; ignored where their area (1200) is outside the range
    cases['no_ground_truth'] = (
        np.stack([pose_of(P), pose_of(Q)]), np.array([0.5, 0.7]), [],
        dict(order=[1, 0], dt_match=np.full((3, 10, 2), -1), dt_ig=np.stack([all10([0, 0]), all10([0, 0]), all10([1, 1])]), gt_ig=np.zeros((3, 0), int)))

    # ground truth and no detection
    cases['no_detection'] = (
        np.zeros((0, 18, 3)), np.zeros(0), [annotation(P, A), annotation(Q, 20000.0, iscrowd=1)],
        dict(order=[], dt_match=np.zeros((3, 10, 0), int), dt_ig=np.zeros((3, 10, 0), int), gt_ig=_t([0, 1], [0, 1], [1, 1])))
    return cases


def check_expected(e, want, name=''):
    """an evaluate_image result against the expected tables of a hand-built case"""
    assert e is not None, name
    assert list(e['order']) == list(want['order']), (name, e['order'])
    if 'areas' in want:
        assert list(e['areas']) == list(want['areas']), (name, e['areas'])
    assert np.array_equal(e['gt_ig'], np.asarray(want['gt_ig'], dtype=bool)), (name, e['gt_ig'])
    for key in ('dt_match', 'dt_ig'):
        if key not in want:
            continue
        if isinstance(want[key], dict):
            for (a, t), row in want[key].items():
                assert list(e[key][a, t].astype(int)) == list(row), (name, key, a, t, e[key][a, t])
        else:
            assert np.array_equal(e[key].astype(int), np.asarray(want[key]).astype(int)), (name, key, e[key].astype(int))


# ---- the seeded generator ----------------------------------------------------------------------------------------------------------------
def _person(rng):
    """17 points of one person: a box of random size somewhere in a 640 x 480 image"""
    w, h = rng.uniform(20, 200), rng.uniform(30, 300)
    x0, y0 = rng.uniform(0, 640 - w), rng.uniform(0, 480 - h)
    pts = np.round(np.stack([x0 + rng.uniform(0, w, 17), y0 + rng.uniform(0, h, 17)], axis=1))
    return pts, [float(np.floor(x0)), float(np.floor(y0)), float(np.ceil(w)), float(np.ceil(h))]


def _oks_row(pose, anns):
    """the OKS of one pose against every annotation, restated here once more (np.sum: close enough to judge a margin)"""
    row = np.zeros(len(anns))
    kd = np.array([pose[j] if pose[j][2] != 0 else (0.0, 0.0, 0.0) for j in JOINT_OF_COCO])
    var = (np.array(SIGMAS) * 2) ** 2
    for g, a in enumerate(anns):
        kg = np.array(a['keypoints']).reshape(17, 3)
        lab = kg[:, 2] > 0
        if lab.any():
            dx, dy = kd[:, 0] - kg[:, 0], kd[:, 1] - kg[:, 1]
        else:
            bb = a['bbox']
            dx = np.maximum(0, bb[0] - bb[2] - kd[:, 0]) + np.maximum(0, kd[:, 0] - (bb[0] + bb[2] * 2))
            dy = np.maximum(0, bb[1] - bb[3] - kd[:, 1]) + np.maximum(0, kd[:, 1] - (bb[1] + bb[3] * 2))
            lab = np.ones(17, bool)
        row[g] = np.exp(-(dx * dx + dy * dy) / var / (a['area'] + 2.0 ** -52) / 2)[lab].sum() / lab.sum()
    return row


def _has_margin(row, margin=1e-8):
    """ten times the margin the host test asserts: no value near a threshold, no two values above 0.39 close but unequal"""
    if row.size == 0:
        return True
    if np.abs(row[:, None] - np.array(THRS)[None, :]).min() < margin:
        return False
    step = np.diff(np.sort(row[row > 0.39]))
    return bool(((step == 0) | (step >= margin)).all())


def image(rng, n_det, n_gt):
    """one generated image; a detection that comes too close to a threshold or to another value of its row is drawn again"""
    anns, pts_of = [], []
    for g in range(n_gt):
        if g and rng.random() < 0.1:                         # a bit-identical duplicate of an earlier annotation
            k = int(rng.integers(0, g))
            anns.append(dict(anns[k]))
            pts_of.append(pts_of[k])
            continue
        pts, bbox = _person(rng)
        vis = rng.integers(0, 3, 17).astype(np.float64)
        kind = rng.random()
        nk = None
        if kind < 0.08:
            vis[:] = 0                                       # nothing labelled: the box branch
        elif kind < 0.14:
            nk = 0                                           # labelled points, but the field says none
        area = [32.0 ** 2, 96.0 ** 2, float(np.round(rng.uniform(200, 40000), 2)), float(np.round(bbox[2] * bbox[3] * 0.6, 2))][int(rng.integers(0, 4))]
        rows = np.concatenate([pts * (vis[:, None] > 0), vis[:, None]], axis=1)
        anns.append(annotation(rows, area, bbox=bbox, iscrowd=int(rng.random() < 0.12), num_keypoints=nk))
        pts_of.append(pts)
    poses, scores = np.zeros((n_det, 18, 3)), np.zeros(n_det)
    d = 0
    while d < n_det:
        jitter = -1.0
        if n_gt and rng.random() < 0.8:
            pts = pts_of[int(rng.integers(0, min(n_gt, 6)))]          # crowd around the first few ground truths
            jitter = [0.0, 1.5, 4.0, 12.0][int(rng.integers(0, 4))]
            pts = pts + rng.normal(0, 1, (17, 2)) * jitter
        else:
            pts, _ = _person(rng)
        found = rng.random(17) < 0.85
        if jitter == 0.0:
            found[:] = True          # an exact copy with missing joints would score k / n exactly: 9 / 12 and 9 / 10 are thresholds
        poses[d] = pose_of(np.concatenate([pts, found[:, None]], axis=1), neck=(rng.uniform(0, 640), rng.uniform(0, 480)))
        scores[d] = float(rng.integers(1, 8)) / 4 if rng.random() < 0.5 else float(np.round(rng.uniform(0.2, 30), 3))
        if _has_margin(_oks_row(poses[d], anns)):
            d += 1
    return poses, scores, anns


def shape_list():
    """(detections, ground truths) of the generated images: every pair up to 64 ground truths, and MAX_GT with 0, 2 and 21 detections"""
    return [(d, g) for g in GTS[:-1] for d in DETS] + [(0, MAX_GT), (2, MAX_GT), (21, MAX_GT)]


@functools.lru_cache(maxsize=None)
def batches():
    """name -> list of images: one image, three images, seventy images (empty ones first, in the middle and last); built once, read only"""
    rng = np.random.default_rng(20260)
    shapes = shape_list()
    seventy = [(0, 0)] + shapes[:17] + [(0, 0), (0, 0)] + shapes[17:] + [(int(rng.integers(0, 30)), int(rng.integers(0, 40))) for _ in range(70 - 4 - len(shapes))] + [(0, 0)]
    assert len(seventy) == 70
    return {'one': [image(rng, 21, 17)],
            'three': [image(rng, 0, 0), image(rng, 25, 64), image(rng, 20, 2)],
            'three_empty_last': [image(rng, 2, 17), image(rng, 0, 0), image(rng, 0, 0)],
            'seventy': [image(rng, d, g) for d, g in seventy]}
