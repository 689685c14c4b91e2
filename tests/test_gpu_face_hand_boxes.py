"""GPU: face / hand key points for many boxes of one image (pmx_forward_u8_boxes / pmx_keypoints_images / pmx_keypoints_boxes,
FaceDetector / HandDetector.detect_boxes, detect_person_parts) against the one-crop-at-a-time path they batch."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, pkg
from test_reference_network import load_e2e

pytestmark = pytest.mark.gpu

SIZE = 368


def _detectors(native, arch, seed, max_batch=16):
    FH, W = pkg('face_hand_detector'), pkg('weights')
    cls = FH.FaceDetector if arch == 'facenet' else FH.HandDetector
    return cls(arch, weights=W.synthetic_weights(seed, arch), device=0, max_batch=max_batch)


def _crop(img, box):
    out = pkg('pose_detector').PoseDetector.crop_image(None, img, tuple(box[:4]))
    return np.ascontiguousarray(out[:, ::-1]) if box[4] else out


def _boxes_mixed(img_h, img_w):
    """inside, straddling every edge, fully outside, 1 x 1, up to 700 x 500, with and without flip"""
    b = [(10, 20, 110, 140), (-30, 5, 60, 90), (img_w - 40, 10, img_w + 25, 70), (15, -25, 80, 40), (30, img_h - 20, 95, img_h + 30),
         (-50, -50, img_w + 50, img_h + 50), (img_w + 5, img_h + 5, img_w + 40, img_h + 30), (-90, -80, -10, -5), (7, 9, 8, 10),
         (100, 50, 800, 550), (0, 0, img_w, img_h), (33, 44, 34, 120), (50, 60, 250, 61), (-3, 7, 400, 380), (60, 60, 428, 428),
         (20, 30, 388, 398), (5, 5, 50, 200), (120, 3, 300, 90), (1, 1, 2, 2), (-700, 10, 0, 510), (img_w - 1, img_h - 1, img_w + 1, img_h + 1)]
    return [tuple(x) + (i % 2,) for i, x in enumerate(b)]


def test_gather_bytes_equal_host_crop_then_device_resize(native):
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (300, 420, 3), dtype=np.uint8)
    boxes = _boxes_mixed(*img.shape[:2])
    assert len(boxes) >= 20
    eng = native.Engine(0, max_batch=12, max_h=SIZE, max_w=SIZE, arch='handnet')
    ref = native.Engine(0, max_batch=1, max_h=SIZE, max_w=SIZE, arch='handnet')
    for k0 in range(0, len(boxes), 12):            # two chunks of the batch capacity
        chunk = boxes[k0:k0 + 12]
        try:
            eng.forward_u8_boxes(img, chunk)
        except native.PmxError as e:
            assert e.code == 4                      # no weights: the gather ran, the network did not
        eng._B = len(chunk)
        got = eng.get_resized(SIZE, SIZE)
        for i, b in enumerate(chunk):
            crop = _crop(img, b)
            # (pmx_forward_u8_resized takes a crop already at the network size as it is: cv2.resize is the identity there)
            want = crop if crop.shape[:2] == (SIZE, SIZE) else ref.resize_u8(crop[None], SIZE, SIZE)[0]
            assert np.array_equal(got[i], want), (k0 + i, b)
    eng.close(); ref.close()


def _tie_maps(rng, B, n_heat, fh=46, fw=46):
    heat = (rng.standard_normal((B, n_heat, fh, fw)) * 0.1).astype(np.float32)
    heat[:, 1] = 0.3                                  # a flat channel: every smoothed value ties
    heat[:, 2] = -1.0                                 # below the threshold
    heat[:, 3, 10, 10] = 2.0; heat[:, 3, 10, 30] = 2.0    # two exactly equal peaks (mirror images of each other)
    return heat


@pytest.mark.parametrize('arch', ['facenet', 'handnet'])
def test_keypoints_images_bit_identical_to_single_calls(native, arch):
    rng = np.random.default_rng(2)
    n_heat = native.Engine.N_MAPS[arch]
    hwf = [(368, 368, 0), (120, 77, 1), (600, 431, 0), (33, 250, 1), (1, 1, 0), (64, 64, 1), (700, 500, 1)]
    B = len(hwf)
    heat = _tie_maps(rng, B, n_heat)
    eng = native.Engine(0, max_batch=B, max_h=SIZE, max_w=SIZE, arch=arch)
    eng.set_heat(heat)
    got = eng.keypoints_images(hwf, 0.1)
    one = native.Engine(0, max_batch=1, max_h=SIZE, max_w=SIZE, arch=arch)
    for i, (h, w, f) in enumerate(hwf):
        one.set_heat(heat[i:i + 1])
        one.set_option('kp_flip_x', f)
        want = one.keypoints(h, w, 0.1)[0]
        assert np.array_equal(got[i], want), (i, hwf[i], np.argwhere(got[i] != want)[:5])
    assert got[:, 1, 3].all() and not got[:, 2, 3].any()
    eng.close(); one.close()


def _check_near(kps, ref):
    """the near-tie rule of test_demo_chain_matches_reference_chain: conf within 1e-4 relative, a moved arg-max only by one pixel"""
    assert len(kps) == len(ref)
    for k, r in zip(kps, ref):
        assert (k is None) == (r is None)
        if k is None:
            continue
        assert abs(float(k[2]) - float(r[2])) <= 1e-4 * max(1.0, abs(float(r[2])))
        if k[:2] != r[:2]:
            assert abs(k[0] - r[0]) <= 1 and abs(k[1] - r[1]) <= 1, (k, r)


def _serial(det, img, boxes, hand):
    out = []
    for b in boxes:
        crop = pkg('pose_detector').PoseDetector.crop_image(None, img, tuple(b[:4]))
        if hand:
            out.append(det(crop, hand_type='left' if b[4] else 'right'))
        else:
            out.append(det(crop))
    return out


def _box_call(det, img, boxes, hand):
    if hand:
        return det.detect_boxes(img, [b[:4] for b in boxes], ['left' if b[4] else 'right' for b in boxes])
    return det.detect_boxes(img, [b[:4] for b in boxes])


@pytest.mark.parametrize('arch', ['facenet', 'handnet'])
def test_detect_boxes_equals_per_crop_calls(native, arch):
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (260, 330, 3), dtype=np.uint8)
    boxes = [b for b in _boxes_mixed(*img.shape[:2]) if (b[2] - b[0]) * (b[3] - b[1]) < 400 * 400][:10]
    hand = arch == 'handnet'
    if not hand:
        boxes = [b[:4] + (0,) for b in boxes]
    # pinned kernels (direct convolutions, no split-K) on both sides: every batch size runs the same summation order -> exact
    batched, serial = _detectors(native, arch, 5, max_batch=4), _detectors(native, arch, 5)
    for d in (batched, serial):
        d.engine.set_option('conv_algo', 0)
        d.engine.set_option('ksplit', 1)
    got = _box_call(batched, img, boxes, hand)
    want = _serial(serial, img, boxes, hand)
    assert got == want
    # default kernels: batch sizes pick their own kernels -> the near-tie rule
    d1, d2 = _detectors(native, arch, 5), _detectors(native, arch, 5)
    _check_all = [_check_near(g, w) for g, w in zip(_box_call(d1, img, boxes, hand), _serial(d2, img, boxes, hand))]
    assert len(_check_all) == len(boxes)
    for d in (batched, serial, d1, d2):
        d.engine.close()


def test_detect_person_parts_on_the_dinner_golden(native):
    PD, FH, W = pkg('pose_detector'), pkg('face_hand_detector'), pkg('weights')
    g = load_e2e('e2e_dinner')
    z = np.load(os.path.join(GOLDEN, 'demo_chain_dinner.npz'))
    img = g['img']
    det = PD.PoseDetector(weights=g['weights'], device=0)
    poses, _ = det(img)
    assert np.array_equal(np.asarray(poses), z['poses'])
    fdet = FH.FaceDetector('facenet', weights=W.synthetic_weights(int(z['face_seed']), 'facenet'), device=0)
    hdet = FH.HandDetector('handnet', weights=W.synthetic_weights(int(z['hand_seed']), 'handnet'), device=0)
    before = np.array(poses, copy=True)
    parts = FH.detect_person_parts(det, fdet, hdet, img, poses)
    assert np.array_equal(np.asarray(poses), before) and len(parts) == len(poses)

    def check(kps, ref, gaps):
        for k, r, gap in zip(kps, ref, gaps):
            assert (k is None) == (r[3] == 0)
            if k is None:
                continue
            assert abs(float(k[2]) - r[2]) <= 1e-4 * max(1.0, abs(r[2]))
            if k[0] != r[0] or k[1] != r[1]:
                assert gap < 1e-4 and abs(k[0] - r[0]) <= 1 and abs(k[1] - r[1]) <= 1, (k, r, gap)
    for i in z['persons']:
        p = parts[int(i)]
        assert p['unit_length'] == float(z['unit_%d' % i])
        for key, part in (('face', p['face']), ('left', p['left']), ('right', p['right'])):
            if '%s_kp_%d' % (key, i) in z.files:
                assert tuple(part['bbox']) == tuple(int(v) for v in z['%s_bbox_%d' % (key, i)])
                check(part['keypoints'], z['%s_kp_%d' % (key, i)], z['%s_gap_%d' % (key, i)])
            else:
                assert part is None
    # all people against the serial chain (fresh batch-1 detectors, demo.py's order)
    f1 = FH.FaceDetector('facenet', weights=W.synthetic_weights(int(z['face_seed']), 'facenet'), device=0)
    h1 = FH.HandDetector('handnet', weights=W.synthetic_weights(int(z['hand_seed']), 'handnet'), device=0)
    n_crops = 0
    for pose, p in zip(np.array(poses, copy=True), parts):
        unit = det.get_unit_length(pose)
        face, bbox = det.crop_face(img, pose, unit)
        assert (face is None) == (p['face'] is None)
        if face is not None:
            assert tuple(bbox) == tuple(p['face']['bbox'])
            _check_near(p['face']['keypoints'], f1(face))
            n_crops += 1
        hands = det.crop_hands(img, pose, unit)
        for side in ('left', 'right'):
            assert (hands[side] is None) == (p[side] is None)
            if hands[side] is not None:
                assert tuple(hands[side]['bbox']) == tuple(p[side]['bbox'])
                _check_near(p[side]['keypoints'], h1(hands[side]['img'], hand_type=side))
                n_crops += 1
    assert n_crops >= 10
    # the demo CLI's canvas from these parts equals the one built from the serial chain's key points
    demo = pkg('demo')
    canvas = demo.render(img, poses, parts)
    assert canvas.shape == img.shape and not np.array_equal(canvas, img)
    for d in (det, fdet, hdet, f1, h1):
        d.engine.close()


def test_launch_counts_independent_of_box_count(native):
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (200, 240, 3), dtype=np.uint8)
    det = _detectors(native, 'facenet', 6, max_batch=8)
    det._grow(8)
    counts = {}
    for n in (1, 3, 8):
        boxes = [(5 + i, 7 + i, 60 + 13 * i, 90 + 9 * i) for i in range(n)]
        det.engine.profile_reset()
        det.engine.profile_enable(True)
        det.detect_boxes(img, boxes)
        prof = det.engine.profile()
        det.engine.profile_enable(False)
        counts[n] = {e['kernel']: e['launches'] for e in prof if e['layer'] in ('kp_boxes', 'resize_boxes')}
    assert counts[1] == counts[3] == counts[8] and len(counts[1]) == 3 and all(v == 1 for v in counts[1].values()), counts
    det.engine.close()


def test_empty_calls_errors_and_growth(native):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (150, 170, 3), dtype=np.uint8)
    hdet = _detectors(native, 'handnet', 7, max_batch=16)
    assert hdet.detect_boxes(img, [], []) == []
    with pytest.raises(native.PmxError):
        hdet.detect_boxes(img, [(10, 10, 40, 40), (20, 20, 20, 50)], ['left', 'right'])
    assert hdet._cap == 1
    with pytest.raises(native.PmxError, match='box 1'):
        hdet.engine.keypoints_boxes(img, [(10, 10, 40, 40, 0), (20, 20, 50, 19, 0)], 0.1)
    crop = img[20:90, 30:120]
    fresh = _detectors(native, 'handnet', 7)
    want = fresh(crop, hand_type='left')
    assert hdet(crop, hand_type='left') == want            # still usable
    boxes = [(i, i, 60 + 3 * i, 70 + 2 * i) for i in range(20)]
    hdet.detect_boxes(img, boxes, ['left'] * 20)
    assert hdet._cap == 16 and hdet.engine.max_batch == 16
    assert hdet(crop, hand_type='left') == want            # after growth: what a fresh batch-1 detector returns
    hdet.engine.close(); fresh.engine.close()


@pytest.mark.parametrize('device_image', [False, True])
def test_one_image_entries_equal_the_many_image_entries(native, device_image):
    """pmx_forward_u8_boxes / pmx_keypoints_boxes are adapters onto the many-image implementation: on the same image and boxes both C
    entries of a pair leave the same network input bytes and return the same key-point rows, host image or device image"""
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (300, 420, 3), dtype=np.uint8)
    boxes5 = [b for b in _boxes_mixed(*img.shape[:2]) if (b[2] - b[0]) * (b[3] - b[1]) < 400 * 400][:10]
    boxes6 = [b + (0,) for b in boxes5]
    assert len(boxes5) == 10 and any(b[4] for b in boxes5)
    src = img
    if device_image:
        import torch
        src = torch.from_numpy(img).to('cuda:0')
        torch.cuda.synchronize()                                         # (the context's stream is not torch's)
    det = _detectors(native, 'handnet', 8, max_batch=4)
    det._grow(4)
    eng = det.engine
    one = eng.keypoints_boxes(src, boxes5, 0.05)                         # three chunks: 4, 4, 2
    many = eng.keypoints_boxes_images([src], boxes6, 0.05)
    assert one.shape == (10, 21, 4) and np.array_equal(one, many)
    if device_image:
        assert np.array_equal(one, eng.keypoints_boxes(img, boxes5, 0.05))
    eng.forward_u8_boxes(src, boxes5[:4])
    got_one, maps_one = eng.get_resized(SIZE, SIZE), eng.get_maps()
    eng.forward_u8_boxes_images([src], boxes6[:4])
    assert np.array_equal(got_one, eng.get_resized(SIZE, SIZE)) and np.array_equal(maps_one, eng.get_maps())
    eng.close()
