"""CPU: the box helpers of the batched face / hand path (PoseDetector.face_bbox / hand_bboxes), the C ABI of the box entries and the
demo command's arguments."""
import os

import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

from conftest import GOLDEN, pkg


class _Host(object):
    """PoseDetector's host helpers without a device context"""
    def __new__(cls):
        return object.__new__(pkg('pose_detector').PoseDetector)


def _check_pose(det, img, pose):
    pose = np.array(pose, copy=True)
    unit = det.get_unit_length(pose)
    if not np.isfinite(unit):
        return
    before = pose.copy()
    fb = det.face_bbox(pose, unit)
    hb = det.hand_bboxes(pose, unit)
    assert np.array_equal(pose, before)                    # the helpers leave the pose alone
    _, bbox = det.crop_face(img, pose.copy(), unit)
    assert fb == (None if bbox is None else tuple(bbox))
    hands = det.crop_hands(img, pose.copy(), unit)          # (crop_hands moves the wrists of the pose it gets)
    for side in ('left', 'right'):
        assert hb[side] == (None if hands[side] is None else tuple(hands[side]['bbox']))


def test_box_helpers_on_the_dinner_poses():
    z = np.load(os.path.join(GOLDEN, 'demo_chain_dinner.npz'))
    det = _Host()
    img = np.zeros((40, 50, 3), np.uint8)
    poses = z['poses']
    assert len(poses) >= 3
    for pose in poses:
        _check_pose(det, img, pose)


@settings(max_examples=200, deadline=None)
@given(st.lists(st.tuples(st.floats(-50, 700, allow_nan=False), st.floats(-50, 500, allow_nan=False), st.sampled_from([0.0, 2.0])),
                min_size=18, max_size=18))
def test_box_helpers_on_random_poses(joints):
    pose = np.array(joints, dtype=np.float64)
    pose[:, :2] = np.where(pose[:, 2:] > 0, np.round(pose[:, :2]), 0)
    with np.errstate(all='ignore'):
        _check_pose(_Host(), np.zeros((30, 30, 3), np.uint8), pose)


def test_box_entries_declared_and_exported():
    native = pkg('native')
    syms = native.header_symbols()
    for s in ('pmx_forward_u8_boxes', 'pmx_keypoints_images', 'pmx_keypoints_boxes'):
        assert s in syms
    if native.needs_build():
        native.build()
    lib = native.load()
    for s in ('pmx_forward_u8_boxes', 'pmx_keypoints_images', 'pmx_keypoints_boxes'):
        assert getattr(lib, s) is not None and s in lib._pmx_sig


def test_demo_parses_its_arguments():
    demo = pkg('demo')
    a = demo.parse_args(['--img', 'x.png', '--gpu', '1', '--out', 'r.png', '--pose-weights', 'p.npz', '--face-weights', 'f.npz',
                         '--hand-weights', 'h.npz'])
    assert (a.img, a.gpu, a.out, a.pose_weights, a.face_weights, a.hand_weights) == ('x.png', 1, 'r.png', 'p.npz', 'f.npz', 'h.npz')
    d = demo.parse_args(['--img', 'y.jpg'])
    assert d.gpu == -1 and d.out == 'result.png'
    with pytest.raises(SystemExit):
        demo.parse_args([])


def test_demo_canvas_helpers():
    demo = pkg('demo')
    a = np.array([[[0, 100, 255]]], np.uint8)
    b = np.array([[[255, 101, 255]]], np.uint8)
    out = demo.add_weighted(a, 0.6, b, 0.4, 0)
    assert out.tolist() == [[[102, 100, 255]]]
    img = np.zeros((6, 7, 3), np.uint8)
    demo.draw_rectangle(img, (1, 1), (4, 3), (255, 255, 255))
    m = img[:, :, 0] > 0
    assert m.sum() == 2 * 4 + 2 * 1 and m[1, 1:5].all() and m[3, 1:5].all() and m[2, 1] and m[2, 4]
