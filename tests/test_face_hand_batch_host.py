"""CPU: the C ABI of the many-image box entries (pmx_forward_u8_boxes_images / pmx_keypoints_boxes_images, pmx_box_image) and
detect_people_parts' host half (boxes, owners, error order) with recording stub detectors."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import pkg
from test_reference_network import load_e2e

NEW = ('pmx_forward_u8_boxes_images', 'pmx_keypoints_boxes_images')
E2E = ('e2e_person', 'e2e_people', 'e2e_dinner')


def _host():
    """PoseDetector's host helpers without a device context (test_face_hand_boxes_host.py::_Host)"""
    return object.__new__(pkg('pose_detector').PoseDetector)


class _Stub(object):
    """a detector that records its detect_boxes_batch calls and answers one marker per box"""
    def __init__(self, hand):
        self.hand, self.calls = hand, []

    def detect_boxes_batch(self, imgs, bboxes_per_image, *hand_types):
        assert len(hand_types) == (1 if self.hand else 0)
        self.calls.append((list(imgs), [list(b) for b in bboxes_per_image]) + tuple([list(t) for t in h] for h in hand_types))
        return [[('kp', self.hand, i, k) for k in range(len(b))] for i, b in enumerate(bboxes_per_image)]

    def detect_boxes(self, img, bboxes, *hand_types):        # (what detect_person_parts calls)
        return [('kp', self.hand, None, k) for k in range(len(bboxes))]


def test_new_entries_declared_exported_and_bound():
    native = pkg('native')
    syms = native.header_symbols()
    for s in NEW:
        assert s in syms
    if native.needs_build():
        native.build()
    lib = native.load()
    for s in NEW:
        assert getattr(lib, s) is not None and s in lib._pmx_sig
    assert len(lib._pmx_sig['pmx_forward_u8_boxes_images'][1]) == 6 and len(lib._pmx_sig['pmx_keypoints_boxes_images'][1]) == 8


def test_box_image_structure_matches_the_header():
    native = pkg('native')
    txt = open(native.HEADER).read()
    m = re.search(r'typedef\s+struct\s+pmx_box_image\s*\{([^}]*)\}\s*pmx_box_image\s*;', txt)
    assert m, 'pmx_box_image is not declared'
    names = [n.split()[-1].strip('*') for decl in m.group(1).split(';') if decl.strip() for n in decl.split(',')]
    assert names == ['bgr', 'h', 'w']
    assert [f[0] for f in native.PmxBoxImage._fields_] == names
    assert [f[1] for f in native.PmxBoxImage._fields_] == [C.c_void_p, C.c_int, C.c_int]

    class Want(C.Structure):          # const uint8_t*; int, int with the C compiler's padding
        _fields_ = [('bgr', C.POINTER(C.c_uint8)), ('h', C.c_int), ('w', C.c_int)]
    assert C.sizeof(native.PmxBoxImage) == C.sizeof(Want) == 16
    assert (native.PmxBoxImage.h.offset, native.PmxBoxImage.w.offset) == (8, 12)


def _expected(det, poses):
    """per image: unit lengths, face boxes + owners, hand boxes + types + owners, from the host helpers"""
    units, fb, fo, hb, ht, ho = [], [], [], [], [], []
    for p, pose in enumerate(np.array(poses, copy=True)):
        unit = det.get_unit_length(pose)
        units.append(unit)
        b = det.face_bbox(pose, unit)
        if b is not None:
            fb.append(b); fo.append(p)
        h = det.hand_bboxes(pose, unit)
        for side in ('left', 'right'):
            if h[side] is not None:
                hb.append(h[side]); ht.append(side); ho.append((p, side))
    return units, fb, fo, hb, ht, ho


def test_detect_people_parts_host_half_with_stub_detectors():
    FH = pkg('face_hand_detector')
    det = _host()
    gs = [load_e2e(n) for n in E2E]
    imgs, poses = [g['img'] for g in gs], [np.array(g['poses'], copy=True) for g in gs]
    before = [p.copy() for p in poses]
    fstub, hstub = _Stub(False), _Stub(True)
    out = FH.detect_people_parts(det, fstub, hstub, imgs, poses)
    assert len(fstub.calls) == 1 and len(hstub.calls) == 1               # ONE call per detector for the whole list
    assert all(np.array_equal(a, b) for a, b in zip(poses, before))      # the input poses are untouched
    assert len(out) == len(imgs)
    n_face = n_hand = 0
    for i, (img, p) in enumerate(zip(imgs, poses)):
        units, fb, fo, hb, ht, ho = _expected(det, p)
        assert fstub.calls[0][0][i] is img and hstub.calls[0][0][i] is img
        assert fstub.calls[0][1][i] == fb
        assert hstub.calls[0][1][i] == hb and hstub.calls[0][2][i] == ht
        assert len(out[i]) == len(p)
        assert [rec['unit_length'] for rec in out[i]] == units
        for k, rec in enumerate(out[i]):
            assert set(rec) == {'unit_length', 'face', 'left', 'right'}
            want = {'bbox': fb[fo.index(k)], 'keypoints': ('kp', False, i, fo.index(k))} if k in fo else None
            assert rec['face'] == want
            for side in ('left', 'right'):
                j = ho.index((k, side)) if (k, side) in ho else None
                assert rec[side] == (None if j is None else {'bbox': hb[j], 'keypoints': ('kp', True, i, j)})
        n_face += len(fb); n_hand += len(hb)
        # the per-image function computes the same boxes
        one = FH.detect_person_parts(det, _Stub(False), _Stub(True), img, p)
        assert [(r['unit_length'], r['face'] and r['face']['bbox'], r['left'] and r['left']['bbox'], r['right'] and r['right']['bbox'])
                for r in one] == \
               [(r['unit_length'], r['face'] and r['face']['bbox'], r['left'] and r['left']['bbox'], r['right'] and r['right']['bbox'])
                for r in out[i]]
    assert (n_face, n_hand) == (12, 4)


def test_detect_people_parts_raises_the_serial_error_before_any_detector_call():
    FH = pkg('face_hand_detector')
    det = _host()
    gs = [load_e2e(n) for n in E2E]
    imgs, poses = [g['img'] for g in gs], [np.array(g['poses'], copy=True) for g in gs]
    bad = np.zeros((18, 3), poses[1].dtype)
    bad[:, :2] = 50                                       # every joint at one point: no limb to measure, the unit length is 0 / 0
    bad[0, 2] = 2                                         # a visible nose: face_bbox meets int(nan)
    poses[1] = np.concatenate([poses[1][:1], bad[None], poses[1][1:]])
    with np.errstate(all='ignore'):
        with pytest.raises(Exception) as serial:
            FH.detect_person_parts(det, _Stub(False), _Stub(True), imgs[1], poses[1])
        fstub, hstub = _Stub(False), _Stub(True)
        with pytest.raises(type(serial.value)) as batch:
            FH.detect_people_parts(det, fstub, hstub, imgs, poses)
    assert type(batch.value) is type(serial.value) and str(batch.value) == str(serial.value)
    assert fstub.calls == [] and hstub.calls == []
    # several errors: the first in (image, person, ...) order -- an empty face box in image 0 comes before the nan of image 1
    tiny = np.zeros((18, 3), poses[0].dtype)
    tiny[:, :2] = 40.3
    tiny[0] = (40.5, 40.5, 2)                             # the nose 0.28 px from all other joints: a unit length that rounds the box to nothing
    unit = det.get_unit_length(tiny.copy())
    fb = det.face_bbox(tiny, unit)
    assert np.isfinite(unit) and (fb[2] == fb[0] or fb[3] == fb[1])
    poses[0] = np.concatenate([poses[0], tiny[None]])
    with pytest.raises(Exception) as serial0:
        FH.detect_person_parts(det, _Stub(False), _Stub(True), imgs[0], poses[0])
    assert type(serial0.value) is not type(serial.value)
    with np.errstate(all='ignore'):
        with pytest.raises(type(serial0.value)):
            FH.detect_people_parts(det, fstub, hstub, imgs, poses)
    assert fstub.calls == [] and hstub.calls == []
    with pytest.raises(ValueError):
        FH.detect_people_parts(det, fstub, hstub, imgs, poses[:2])
