"""CPU: the COCO key-point evaluation contract of coco.py (oks_matrix, evaluate_image, accumulate, summarize, results) against closed
forms, an independent scalar loop, hand-built matching cases with their tables written out, and hand-computed precision curves; and the
margins of the generated images that tests/test_gpu_coco_eval.py compares the device entry on."""
import math

import numpy as np
import pytest

import coco_eval_cases as CS
from conftest import pkg


@pytest.fixture(scope='module')
def coco():
    return pkg('coco')


def ref_oks(kps_d, ann):
    """one detection ((17, 3) rows in COCO order) against one annotation dictionary: a scalar loop of its own"""
    kg = [ann['keypoints'][3 * i:3 * i + 3] for i in range(17)]
    k1 = sum(1 for p in kg if p[2] > 0)
    bb = ann['bbox']
    x0, x1, y0, y1 = bb[0] - bb[2], bb[0] + bb[2] * 2, bb[1] - bb[3], bb[1] + bb[3] * 2
    total, n = 0.0, 0
    for i in range(17):
        xd, yd = float(kps_d[i][0]), float(kps_d[i][1])
        if k1 > 0:
            if not kg[i][2] > 0:
                continue
            dx, dy = xd - kg[i][0], yd - kg[i][1]
        else:
            dx = max(0.0, x0 - xd) + max(0.0, xd - x1)
            dy = max(0.0, y0 - yd) + max(0.0, yd - y1)
        var = (CS.SIGMAS[i] * 2) ** 2
        total += math.exp(-((dx * dx + dy * dy) / var / (ann['area'] + 2.0 ** -52) / 2))
        n += 1
    return total / n


def ref_matrix(coco, poses, scores, anns):
    d = coco.detections(poses, scores)
    order = sorted(range(len(scores)), key=lambda i: -scores[i])[:20]          # sorted() is stable
    return np.array([[ref_oks(d['keypoints'][i], a) for a in anns] for i in order]).reshape(len(order), len(anns)), order


def test_constants(coco):
    assert coco.KP_EPS == 2.0 ** -52 and coco.MAX_DETS == 20 and coco.EVAL_MAX_GT == CS.MAX_GT
    assert np.allclose(coco.KP_SIGMAS, CS.SIGMAS, rtol=1e-15) and np.array_equal(coco.KP_VARS, (coco.KP_SIGMAS * 2) ** 2)
    assert np.allclose(coco.IOU_THRS, CS.THRS, rtol=1e-15) and coco.IOU_THRS[0] == 0.5 and coco.IOU_THRS[5] == 0.75
    assert len(coco.REC_THRS) == 101 and coco.REC_THRS[50] == 0.5 and coco.REC_THRS[100] == 1.0
    assert coco.AREA_RNGS == [[0, 1e10], [1024, 9216], [9216, 1e10]]
    assert [int(j) for j in pkg('entity').params['coco_joint_indices']] == CS.JOINT_OF_COCO


def test_detections_drop_the_neck_zero_missing_joints_and_take_the_area_over_zeros(coco):
    P = CS.grid_points(100, 100)
    rows = np.concatenate([P, np.ones((17, 1))], axis=1)
    rows[3, 2] = 0
    d = coco.detections(CS.pose_of(rows)[None], [2.5])
    want = rows.copy()
    want[3] = 0
    assert np.array_equal(d['keypoints'][0], want) and d['score'][0] == 2.5
    assert d['area'][0] == (140 - 0) * (130 - 0)          # the zeros of the missing joint are part of the box
    assert coco.detections(np.array([]), np.empty(0))['keypoints'].shape == (0, 17, 3)


@pytest.mark.parametrize('d, area', [(0.0, 5000.0), (3.0, 5000.0), (1.0, 1024.0), (12.0, 40000.0)])
def test_oks_closed_form_all_points_visible(coco, d, area):
    P = CS.grid_points(50, 60)
    got = coco.oks_matrix(coco.detections(CS.pose_of(P + [d, 0])[None], [1.0]), [CS.annotation(P, area)])
    want = sum(math.exp(-d * d / (8 * s * s * area)) for s in CS.SIGMAS) / 17
    assert got.shape == (1, 1) and abs(got[0, 0] - want) <= 1e-15 * want, (got[0, 0], want)
    if d == 0:
        assert got[0, 0] == 1.0


def test_oks_box_branch_when_nothing_is_labelled(coco):
    rows = np.zeros((17, 3))
    ann = CS.annotation(rows, 5000.0, bbox=[100, 200, 40, 60])          # the doubled box: x 60 .. 180, y 140 .. 320
    assert ann['num_keypoints'] == 0
    inside = np.stack([np.linspace(60, 180, 17), np.linspace(140, 320, 17)], axis=1)
    assert coco.oks_matrix(coco.detections(CS.pose_of(inside)[None], [1.0]), [ann])[0, 0] == 1.0
    outside = np.stack([np.full(17, 185.0), np.full(17, 137.0)], axis=1)          # 5 to the right, 3 above
    got = coco.oks_matrix(coco.detections(CS.pose_of(outside)[None], [1.0]), [ann])[0, 0]
    want = sum(math.exp(-(25 + 9) / (8 * s * s * 5000.0)) for s in CS.SIGMAS) / 17
    assert abs(got - want) <= 1e-15 * want and got < 1
    # a missing joint of the detection sits at (0, 0): far outside this box
    rows_d = np.concatenate([inside, np.ones((17, 1))], axis=1)
    rows_d[0, 2] = 0
    got = coco.oks_matrix(coco.detections(CS.pose_of(rows_d)[None], [1.0]), [ann])[0, 0]
    want = (16 + math.exp(-(60.0 ** 2 + 140.0 ** 2) / (8 * CS.SIGMAS[0] ** 2 * 5000.0))) / 17
    assert abs(got - want) <= 1e-15 * want


def test_oks_counts_only_labelled_points(coco):
    P = CS.grid_points(50, 60)
    rows = np.concatenate([P, np.full((17, 1), 2.0)], axis=1)
    rows[[1, 4, 9], 2] = 0
    rows[[1, 4, 9], :2] = 0
    ann = CS.annotation(rows, 3000.0)
    det = P + [2.0, 0]
    det[4] += 500                                        # an unlabelled point: however wrong, it does not count
    got = coco.oks_matrix(coco.detections(CS.pose_of(det)[None], [1.0]), [ann])[0, 0]
    want = sum(math.exp(-4.0 / (8 * s * s * 3000.0)) for i, s in enumerate(CS.SIGMAS) if i not in (1, 4, 9)) / 14
    assert abs(got - want) <= 1e-15 * want
    assert abs(got - ref_oks(coco.detections(CS.pose_of(det)[None], [1.0])['keypoints'][0], ann)) <= 1e-15


@pytest.mark.parametrize('n', [21, 25])
def test_oks_rows_follow_the_stable_score_order_and_stop_at_20(coco, n):
    rng = np.random.default_rng(n)
    poses, _, anns = CS.image(rng, n, 5)
    scores = np.array([float(v) for v in rng.integers(1, 4, n)])          # three values: long runs of ties
    got = coco.oks_matrix(coco.detections(poses, scores), anns)
    want, order = ref_matrix(coco, poses, scores, anns)
    assert got.shape == (20, 5) and list(coco.detection_order(coco.detections(poses, scores))) == order
    assert len(set(scores[order])) > 1 and order != sorted(order)
    # the two sides add the same terms in the same order; their exp may differ by an ulp or two per term (<= 1), the mean of at most 17
    assert np.abs(got - want).max() <= 1e-14


def test_oks_against_the_scalar_loop_on_generated_images(coco):
    rng = np.random.default_rng(5)
    for n_det, n_gt in ((3, 4), (20, 17), (1, 1)):
        poses, scores, anns = CS.image(rng, n_det, n_gt)
        got = coco.oks_matrix(coco.detections(poses, scores), anns)
        want, _ = ref_matrix(coco, poses, scores, anns)
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-14
    assert coco.oks_matrix(coco.detections(poses, scores), []).size == 0
    assert coco.oks_matrix(coco.detections(np.zeros((0, 18, 3)), []), anns).size == 0


# ---- matching ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(CS.hand_cases()))
def test_matching_hand_built(coco, name):
    poses, scores, anns, want = CS.hand_cases()[name]
    e = coco.evaluate_image(coco.detections(poses, scores), anns)
    CS.check_expected(e, want, name)
    D, G = len(scores), len(anns)
    assert e['dt_match'].shape == (3, 10, D) and e['dt_match'].dtype == np.int32 and e['dt_ig'].shape == (3, 10, D) and e['dt_ig'].dtype == bool
    assert e['gt_ig'].shape == (3, G) and e['gt_ig'].dtype == bool and len(e['scores']) == len(e['areas']) == D


def test_an_image_with_neither_is_none(coco):
    assert coco.evaluate_image(coco.detections(np.array([]), np.empty(0)), []) is None


# ---- accumulate and summarize ------------------------------------------------------------------------------------------------------------
def _perfect_images(coco, areas, extra=None):
    out = []
    for k in range(5):
        pts = [CS.grid_points(60 + 150 * j, 40 + 13 * k) for j in range(len(areas))]
        anns = [CS.annotation(p, a) for p, a in zip(pts, areas)]
        poses = [CS.pose_of(p) for p in pts]
        scores = [5.0 + j + k / 10 for j in range(len(areas))]
        if extra is not None and (extra[1] is None or extra[1] == k):
            poses.append(CS.pose_of(CS.grid_points(500, 300)))
            scores.append(extra[0])
        out.append(coco.evaluate_image(coco.detections(np.stack(poses), scores), anns))
    return out


def test_perfect_detections_give_ones(coco):
    s = coco.summarize(*coco.accumulate(_perfect_images(coco, [5000.0, 20000.0])))
    assert list(s) == list(coco.SUMMARY_KEYS) and len(s) == 10
    assert all(abs(v - 1) <= 1e-12 for v in s.values()), s
    s = coco.summarize(*coco.accumulate(_perfect_images(coco, [5000.0, 6000.0])))          # nothing large: that range stays empty
    assert s['AP_large'] == -1 and s['AR_large'] == -1
    assert all(abs(v - 1) <= 1e-12 for k, v in s.items() if not k.endswith('large')), s


def test_a_low_score_false_positive_per_image_leaves_ap_unchanged(coco):
    base = coco.summarize(*coco.accumulate(_perfect_images(coco, [5000.0, 20000.0])))
    # (the stray detection's own area, 1200, lies in 'medium': it is a false positive there and in 'all', ignored in 'large')
    more = coco.summarize(*coco.accumulate(_perfect_images(coco, [5000.0, 20000.0], extra=(0.01, None))))
    assert all(abs(more[k] - base[k]) <= 1e-12 for k in base), (base, more)


def test_one_high_score_false_positive_lowers_the_curve_as_computed_by_hand(coco):
    # one image, two ground truths (medium), detections by score: a hit, a stray, a hit.  tp = 1 1 2, fp = 0 1 1, recall = .5 .5 1,
    # precision = 1, 1/2, 2/3 -> from the right 1, 2/3, 2/3.  searchsorted(recall, r, 'left') is 0 up to r = .5 (51 points) and 2 above (50)
    p0, p1 = CS.grid_points(60, 40), CS.grid_points(260, 40)
    anns = [CS.annotation(p0, 5000.0), CS.annotation(p1, 5000.0)]
    poses = np.stack([CS.pose_of(p0), CS.pose_of(CS.grid_points(500, 300)), CS.pose_of(p1)])
    e = coco.evaluate_image(coco.detections(poses, [0.9, 0.8, 0.7]), anns)
    assert list(e['dt_match'][0, 0]) == [0, -1, 1]
    precision, recall = coco.accumulate([e, None])
    curve = np.array([1.0] * 51 + [2.0 / 3.0] * 50)
    for t in range(10):
        assert np.abs(precision[t, :, 0] - curve).max() <= 1e-12 and np.abs(precision[t, :, 1] - curve).max() <= 1e-12
        assert recall[t, 0] == 1.0 and recall[t, 1] == 1.0
    assert (precision[:, :, 2] == -1).all() and (recall[:, 2] == -1).all()
    s = coco.summarize(precision, recall)
    assert abs(s['AP'] - (51 + 50 * 2 / 3) / 101) <= 1e-12 and abs(s['AP50'] - s['AP']) <= 1e-12 and s['AR'] == 1.0 and s['AP_large'] == -1
    # the same stray with the highest score on one of five otherwise perfect images: precision k / (k + 1) from the right is 10 / 11
    # everywhere but at recall 0, where idx = 0 picks the stray's own slot, pulled up to the same 10 / 11
    s = coco.summarize(*coco.accumulate(_perfect_images(coco, [5000.0, 6000.0], extra=(99.0, 2))))
    assert abs(s['AP_medium'] - 10 / 11) <= 1e-12 and abs(s['AR_medium'] - 1) <= 1e-12


def test_no_kept_ground_truth_gives_minus_one(coco):
    P = CS.grid_points(60, 40)
    e = coco.evaluate_image(coco.detections(CS.pose_of(P)[None], [1.0]), [CS.annotation(P, 5000.0, iscrowd=1)])
    precision, recall = coco.accumulate([e])
    assert (precision == -1).all() and (recall == -1).all()
    assert all(v == -1 for v in coco.summarize(precision, recall).values())
    precision, recall = coco.accumulate([])
    assert (precision == -1).all() and precision.shape == (10, 101, 3) and recall.shape == (10, 3)


def test_a_ground_truth_without_detections_gives_zero_recall(coco):
    e = coco.evaluate_image(coco.detections(np.array([]), []), [CS.annotation(CS.grid_points(60, 40), 5000.0)])
    precision, recall = coco.accumulate([e])
    assert (recall[:, :2] == 0).all() and (precision[:, :, :2] == 0).all() and (recall[:, 2] == -1).all()


# ---- results -----------------------------------------------------------------------------------------------------------------------------
def test_results_round_trip_of_an_annotation(coco):
    rng = np.random.default_rng(3)
    anns = []
    for _ in range(3):
        kp = np.zeros((17, 3), np.int64)
        kp[:, 0], kp[:, 1], kp[:, 2] = rng.integers(1, 600, 17), rng.integers(1, 400, 17), rng.integers(0, 3, 17)
        kp[kp[:, 2] == 0, :2] = 0
        anns.append({'keypoints': [int(v) for v in kp.reshape(-1)], 'num_keypoints': int((kp[:, 2] > 0).sum()), 'area': 1.0, 'iscrowd': 0})
    poses = coco.parse_annotations(anns)
    res = coco.results([42], [poses], [[0.5, 1.5, 2.5]])
    assert len(res) == 3 and all(r['image_id'] == 42 and r['category_id'] == 1 and len(r['keypoints']) == 51 for r in res)
    assert [r['score'] for r in res] == [0.5, 1.5, 2.5]
    for r, a in zip(res, anns):
        got, want = np.array(r['keypoints']).reshape(17, 3), np.array(a['keypoints']).reshape(17, 3)
        lab = want[:, 2] > 0
        assert lab.any() and not lab.all()
        assert np.array_equal(got[lab, :2], want[lab, :2]) and (got[lab, 2] == 1).all() and (got[~lab] == 0).all()
    assert coco.results([1, 2], [np.array([]), poses[:1]], [np.empty(0), [3.0]])[0]['image_id'] == 2


# ---- the margins of the GPU cases --------------------------------------------------------------------------------------------------------
def test_generated_images_keep_their_margins(coco):
    seen_shapes, n_dup, n_box = set(), 0, 0
    for name, images in CS.batches().items():
        for k, (poses, scores, anns) in enumerate(images):
            seen_shapes.add((len(scores), len(anns)))
            oks = coco.oks_matrix(coco.detections(poses, scores), anns)
            n_box += sum(1 for a in anns if not any(v > 0 for v in a['keypoints'][2::3]))
            if oks.size == 0:
                continue
            gap = np.abs(oks[:, :, None] - np.asarray(CS.THRS)[None, None, :]).min()
            assert gap >= 1e-9, (name, k, gap)
            for row in oks:
                v = np.sort(row[row > 0.4])
                step = np.diff(v)
                n_dup += int((step == 0).sum())
                assert ((step == 0) | (step >= 1e-9)).all(), (name, k, step[(step > 0) & (step < 1e-9)])
    assert set(CS.shape_list()) <= seen_shapes and (0, 0) in seen_shapes
    assert n_dup > 0 and n_box > 0
    assert [len(v) for v in CS.batches().values()] == [1, 3, 3, 70]
    b = CS.batches()['seventy']
    assert all(len(b[i][1]) == 0 and len(b[i][2]) == 0 for i in (0, 18, 19, 69))
