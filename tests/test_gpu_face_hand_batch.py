"""GPU: face / hand key points for the boxes of MANY images in one call (pmx_forward_u8_boxes_images / pmx_keypoints_boxes_images,
FaceDetector / HandDetector.detect_boxes_batch, detect_people_parts) against the one-image entries they generalise."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, pkg
from test_gpu_face_hand_boxes import SIZE, _box_call, _boxes_mixed, _check_near, _detectors, _serial
from test_reference_network import load_e2e

pytestmark = pytest.mark.gpu


def _images(seed):
    """three images of different sizes: one wider than the network input, one smaller than 100 pixels on a side"""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, s, dtype=np.uint8) for s in ((300, 420, 3), (90, 64, 3), (200, 517, 3))]


def _interleaved(imgs):
    """the mixed boxes, box k on image k % 3 (built for that image's size): consecutive boxes belong to different images"""
    per = [_boxes_mixed(*im.shape[:2]) for im in imgs]
    return [per[k % len(imgs)][k] + (k % len(imgs),) for k in range(len(per[0]))]


def test_gather_bytes_equal_the_one_image_gather(native):
    """contract A"""
    imgs = _images(11)
    boxes6 = _interleaved(imgs)
    assert len(boxes6) >= 20 and all(a[5] != b[5] for a, b in zip(boxes6, boxes6[1:]))
    assert max(im.shape[1] for im in imgs) > SIZE and min(min(im.shape[:2]) for im in imgs) < 100
    eng = native.Engine(0, max_batch=12, max_h=SIZE, max_w=SIZE, arch='handnet')
    one = native.Engine(0, max_batch=1, max_h=SIZE, max_w=SIZE, arch='handnet')
    for k0 in range(0, len(boxes6), 12):            # two chunks of the batch capacity
        chunk = boxes6[k0:k0 + 12]
        with pytest.raises(native.PmxError) as e:
            eng.forward_u8_boxes_images(imgs, chunk)
        assert e.value.code == 4                    # no weights: the gather ran, the network did not
        eng._B = len(chunk)
        got = eng.get_resized(SIZE, SIZE)
        for i, b in enumerate(chunk):
            with pytest.raises(native.PmxError) as e1:
                one.forward_u8_boxes(imgs[b[5]], [b[:5]])
            assert e1.value.code == 4
            one._B = 1
            want = one.get_resized(SIZE, SIZE)[0]
            assert np.array_equal(got[i], want), (k0 + i, b)
    eng.close(); one.close()


def _split(imgs, boxes6):
    """-> per image: boxes (5 columns), and the flat positions they came from"""
    per, pos = [[] for _ in imgs], [[] for _ in imgs]
    for k, b in enumerate(boxes6):
        per[b[5]].append(b[:5]); pos[b[5]].append(k)
    return per, pos


def _batch_call(det, imgs, per, hand):
    if hand:
        return det.detect_boxes_batch(imgs, [[b[:4] for b in bs] for bs in per], [['left' if b[4] else 'right' for b in bs] for bs in per])
    return det.detect_boxes_batch(imgs, [[b[:4] for b in bs] for bs in per])


def _cases(arch, seed):
    imgs = _images(seed)
    boxes6 = [b for b in _interleaved(imgs) if (b[2] - b[0]) * (b[3] - b[1]) < 400 * 400][:11]
    hand = arch == 'handnet'
    if not hand:
        boxes6 = [b[:4] + (0, b[5]) for b in boxes6]
    per, _ = _split(imgs, boxes6)
    assert len(boxes6) >= 10 and all(len(p) >= 2 for p in per)
    return imgs, per, hand


def _close(*dets):
    for d in dets:
        d.engine.close()


@pytest.mark.parametrize('arch', ['facenet', 'handnet'])
def test_batch_equals_per_image_and_per_crop_calls_with_pinned_kernels(native, arch):
    """contract B: direct convolutions, no split-K on every side: the summation order does not depend on the batch size -> exact"""
    imgs, per, hand = _cases(arch, 12)
    batched, boxed, serial = (_detectors(native, arch, 5, max_batch=4), _detectors(native, arch, 5, max_batch=4),
                              _detectors(native, arch, 5))
    for d in (batched, boxed, serial):
        d.engine.set_option('conv_algo', 0)
        d.engine.set_option('ksplit', 1)
    got = _batch_call(batched, imgs, per, hand)
    assert batched.engine.max_batch == 4            # 11 boxes in chunks of 4, 4, 3: every chunk crosses image borders
    assert len(got) == len(imgs)
    for im, bs, g in zip(imgs, per, got):
        assert g == _box_call(boxed, im, bs, hand)
        assert g == _serial(serial, im, bs, hand)
    _close(batched, boxed, serial)


@pytest.mark.parametrize('arch', ['facenet', 'handnet'])
def test_batch_equals_per_image_and_per_crop_calls_in_f16_mode(native, arch):
    """contract C: the f16 mode's maps of an image do not depend on batch size or position -> exact with default kernel selection"""
    FH, W = pkg('face_hand_detector'), pkg('weights')
    cls = FH.FaceDetector if arch == 'facenet' else FH.HandDetector
    imgs, per, hand = _cases(arch, 13)
    w = W.synthetic_weights(5, arch)
    batched, boxed, serial = (cls(arch, weights=w, device=0, max_batch=4, precision='f16'),
                              cls(arch, weights=w, device=0, max_batch=4, precision='f16'), cls(arch, weights=w, device=0, precision='f16'))
    got = _batch_call(batched, imgs, per, hand)
    for im, bs, g in zip(imgs, per, got):
        assert g == _box_call(boxed, im, bs, hand)
        assert g == _serial(serial, im, bs, hand)
    _close(batched, boxed, serial)


@pytest.mark.parametrize('arch', ['facenet', 'handnet'])
def test_batch_near_per_image_and_per_crop_calls_with_default_kernels(native, arch):
    """contract D: chunk sizes pick their own fp32 kernels -> the near-tie rule of test_gpu_face_hand_boxes.py::_check_near"""
    imgs, per, hand = _cases(arch, 14)
    batched, boxed, serial = _detectors(native, arch, 5, max_batch=4), _detectors(native, arch, 5, max_batch=4), _detectors(native, arch, 5)
    got = _batch_call(batched, imgs, per, hand)
    n = 0
    for im, bs, g in zip(imgs, per, got):
        for a, b, c in zip(g, _box_call(boxed, im, bs, hand), _serial(serial, im, bs, hand)):
            _check_near(a, b)
            _check_near(a, c)
            n += 1
    assert n >= 10
    _close(batched, boxed, serial)


def test_model_seam_runs_one_callable_per_crop(native):
    """`model=` as a callable: per crop the callable, the key points of all crops in chunks -- the same lists as detect_boxes per image"""
    FH = pkg('face_hand_detector')
    imgs, per, hand = _cases('handnet', 15)
    calls = []

    def model(x):
        calls.append(x.shape)
        r = np.random.default_rng(int(np.abs(x).sum() * 16) % (2 ** 31))      # maps that depend on the crop alone
        return [(r.standard_normal((1, 22, 46, 46)) * 0.2).astype(np.float32)]
    a, b = FH.HandDetector('handnet', model=model, device=0, max_batch=4), FH.HandDetector('handnet', model=model, device=0, max_batch=4)
    got = _batch_call(a, imgs, per, hand)
    assert len(calls) == sum(len(p) for p in per) and all(s == (1, 3, SIZE, SIZE) for s in calls)
    for im, bs, g in zip(imgs, per, got):
        assert g == _box_call(b, im, bs, hand)
    _close(a, b)


def _counts(det, imgs, per):
    det.engine.profile_reset()
    det.engine.profile_enable(True)
    det.detect_boxes_batch(imgs, per)
    prof = det.engine.profile()
    det.engine.profile_enable(False)
    return {e['kernel']: e['launches'] for e in prof if e['layer'] in ('kp_boxes', 'resize_boxes')}


def test_launch_counts_depend_on_chunks_not_on_images(native):
    """contract E"""
    rng = np.random.default_rng(17)
    imgs = [rng.integers(0, 256, (200 + 10 * i, 240 - 20 * i, 3), dtype=np.uint8) for i in range(4)]
    det = _detectors(native, 'facenet', 6, max_batch=8)
    det._grow(8)
    boxes = [(5 + i, 7 + i, 60 + 13 * i, 90 + 9 * i) for i in range(8)]
    one = _counts(det, imgs, [boxes, [], [], []])                        # 8 boxes of one image
    four = _counts(det, imgs, [boxes[0:2], boxes[2:4], boxes[4:6], boxes[6:8]])     # 8 boxes over 4 images
    assert one == four and len(one) == 3 and all(v == 1 for v in one.values()), (one, four)
    assert 'box_gather_resize_u8_images_kernel' in one
    # 20 boxes over 4 images on the batch-8 engine: ceil(20 / 8) = 3 chunks -> 3 gathers, 3 tile launches, one merge
    many = _counts(det, imgs, [[boxes[(5 * i + k) % 8] for k in range(5)] for i in range(4)])
    assert many == {'box_gather_resize_u8_images_kernel': 3, 'kp_tiles_kernel': 3, 'kp_merge_kernel': 1}, many
    det.engine.close()


def _parts_equal(a, b):
    assert len(a) == len(b)
    for p, q in zip(a, b):
        assert p['unit_length'] == q['unit_length'] or (np.isnan(p['unit_length']) and np.isnan(q['unit_length']))
        for key in ('face', 'left', 'right'):
            assert (p[key] is None) == (q[key] is None)
            if p[key] is not None:
                assert tuple(p[key]['bbox']) == tuple(q[key]['bbox']) and p[key]['keypoints'] == q[key]['keypoints']


def test_detect_people_parts_on_the_goldens(native):
    FH, W = pkg('face_hand_detector'), pkg('weights')
    z = np.load(os.path.join(GOLDEN, 'demo_chain_dinner.npz'))
    gs = [load_e2e(n) for n in ('e2e_person', 'e2e_dinner', 'e2e_people')]
    imgs, poses = [g['img'] for g in gs], [g['poses'] for g in gs]
    assert np.array_equal(np.asarray(poses[1]), z['poses'])
    det = object.__new__(pkg('pose_detector').PoseDetector)              # the host helpers: the golden poses need no pose network

    def pair():
        f = FH.FaceDetector('facenet', weights=W.synthetic_weights(int(z['face_seed']), 'facenet'), device=0)
        h = FH.HandDetector('handnet', weights=W.synthetic_weights(int(z['hand_seed']), 'handnet'), device=0)
        return f, h

    def pin(*dets):
        for d in dets:
            d.engine.set_option('conv_algo', 0)
            d.engine.set_option('ksplit', 1)
    # pinned kernels: per image exactly what detect_person_parts returns for that image alone
    fb, hb = pair(); f1, h1 = pair()
    pin(fb, hb, f1, h1)
    before = [np.array(p, copy=True) for p in poses]
    people = FH.detect_people_parts(det, fb, hb, imgs, poses)
    assert all(np.array_equal(np.asarray(p), b) for p, b in zip(poses, before)) and len(people) == len(imgs)
    for im, ps, got in zip(imgs, poses, people):
        _parts_equal(got, FH.detect_person_parts(det, f1, h1, im, ps))
    n_face = sum(p['face'] is not None for parts in people for p in parts)
    n_hand = sum((p['left'] is not None) + (p['right'] is not None) for parts in people for p in parts)
    assert (n_face, n_hand) == (12, 4) and n_face + n_hand >= 10
    _close(fb, hb, f1, h1)
    # default kernels: the dinner entry against the values the reference's own chain wrote (the checks of
    # test_gpu_face_hand_boxes.py::test_detect_person_parts_on_the_dinner_golden)
    fd, hd = pair()
    parts = FH.detect_people_parts(det, fd, hd, imgs, poses)[1]
    assert len(parts) == len(poses[1])

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
    _close(fd, hd)


def test_empty_calls_errors_and_growth(native):
    rng = np.random.default_rng(18)
    imgs = [rng.integers(0, 256, (150 + 7 * i, 170 - 11 * i, 3), dtype=np.uint8) for i in range(5)]
    hdet = _detectors(native, 'handnet', 7, max_batch=16)
    # n == 0: no device work (no kernel of the box layers, the engine does not grow)
    hdet.engine.profile_reset()
    hdet.engine.profile_enable(True)
    assert hdet.detect_boxes_batch(imgs, [[] for _ in imgs], [[] for _ in imgs]) == [[] for _ in imgs]
    assert hdet.engine.keypoints_boxes_images(imgs, [], 0.1).shape == (0, 21, 4)
    assert hdet.engine.keypoints_boxes_images([], [], 0.1).shape == (0, 21, 4)
    assert hdet.engine.profile() == []
    hdet.engine.profile_enable(False)
    assert hdet._cap == 1
    with pytest.raises(native.PmxError, match='box 1'):                  # an empty box, before the engine grows
        hdet.detect_boxes_batch(imgs[:2], [[(10, 10, 40, 40)], [(20, 20, 20, 50)]], [['left'], ['right']])
    assert hdet._cap == 1
    ok = (10, 10, 40, 40, 0)
    with pytest.raises(native.PmxError, match='box 1') as e:
        hdet.engine.keypoints_boxes_images(imgs, [ok + (0,), (20, 20, 50, 19, 0, 1)], 0.1)
    assert e.value.code == 1
    for bad in (5, -1):
        with pytest.raises(native.PmxError, match='box 2') as e:         # an image index out of range names the box
            hdet.engine.keypoints_boxes_images(imgs, [ok + (0,), ok + (4,), ok + (bad,)], 0.1)
        assert e.value.code == 1 and 'image index %d' % bad in str(e.value)
    with pytest.raises(native.PmxError, match='image 3') as e:           # an image that a box refers to is missing
        hdet.engine.keypoints_boxes_images(imgs[:3] + [None, imgs[4]], [ok + (4,), ok + (3,)], 0.1)
    assert e.value.code == 1
    with pytest.raises(native.PmxError) as e:                            # no image at all
        hdet.engine.keypoints_boxes_images([], [ok + (0,)], 0.1)
    assert e.value.code == 1
    with pytest.raises(native.PmxError, match='flip') as e:
        hdet.engine.keypoints_boxes_images(imgs, [(10, 10, 40, 40, 2, 0)], 0.1)
    assert e.value.code == 1
    with pytest.raises(native.PmxError) as e:                            # more boxes than the batch in the forward-only entry
        hdet.engine.forward_u8_boxes_images(imgs, [ok + (0,), ok + (1,)])
    assert e.value.code == 5
    # an image that no box refers to need not exist
    crop = imgs[2][20:90, 30:120]
    fresh = _detectors(native, 'handnet', 7)
    want = fresh(crop, hand_type='left')
    got = hdet.engine.keypoints_boxes_images([None, None, imgs[2]], [(30, 20, 120, 90, 1, 2)], 0.1)
    assert pkg('face_hand_detector')._keypoint_list(got[0]) == want
    assert hdet(crop, hand_type='left') == want                          # after the failing calls: still what a fresh detector returns
    # a posenet context
    pose = native.Engine(0, max_batch=1, max_h=SIZE, max_w=SIZE)
    for call in (lambda: pose.keypoints_boxes_images(imgs, [ok + (0,)], 0.1), lambda: pose.forward_u8_boxes_images(imgs, [ok + (0,)])):
        with pytest.raises(native.PmxError) as e:
            call()
        assert e.value.code == 6
    pose.close()
    # 40 boxes over 5 images on a max_batch = 16 detector
    per = [[(i + k, i, 60 + 3 * i + k, 70 + 2 * i) for i in range(8)] for k in range(5)]
    out = hdet.detect_boxes_batch(imgs, per, [['left'] * 8] * 5)
    assert [len(o) for o in out] == [8] * 5 and all(len(kp) == 21 for o in out for kp in o)
    assert hdet._cap == 16 and hdet.engine.max_batch == 16
    assert hdet(crop, hand_type='left') == want                          # after growth
    _close(hdet, fresh)


def test_device_images_through_torch_tensors(native):
    """on_device != 0: the images are torch uint8 tensors on the context's device; the same rows as from the host arrays"""
    import torch
    imgs = _images(19)
    boxes6 = [b for b in _interleaved(imgs) if (b[2] - b[0]) * (b[3] - b[1]) < 400 * 400][:6]
    det = _detectors(native, 'handnet', 8, max_batch=4)
    det._grow(4)
    want = det.engine.keypoints_boxes_images(imgs, boxes6, 0.05)
    dev = [torch.from_numpy(im).to('cuda:0') for im in imgs]
    torch.cuda.synchronize()                                             # (the context's stream is not torch's)
    got = det.engine.keypoints_boxes_images(dev, boxes6, 0.05)
    assert np.array_equal(got, want)
    with pytest.raises(ValueError):
        det.engine.keypoints_boxes_images([dev[0], imgs[1], imgs[2]], boxes6, 0.05)
    del dev
    det.engine.close()
