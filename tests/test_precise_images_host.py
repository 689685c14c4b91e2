"""CPU: detect_precise for lists of images of different sizes (include/pose_mi355x.h::pmx_detect_precise_images) -- the C ABI is declared and
exported with matching ctypes signatures, and PoseDetector.detect_precise_batch routes, chunks and orders a mixed list correctly (stub
engine: no GPU)."""
import ctypes
import math

import numpy as np
import pytest

from conftest import pkg

ENTRIES = ('pmx_detect_precise_images', 'pmx_get_precise_image_maps', 'pmx_precise_images_table_bytes')


def test_precise_images_entries_declared_and_exported():
    native = pkg('native')
    syms = native.header_symbols()
    for s in ENTRIES:
        assert s in syms
    if native.needs_build():
        native.build()
    lib = native.load()
    for s in ENTRIES:
        assert getattr(lib, s) is not None and s in lib._pmx_sig
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert lib._pmx_sig['pmx_detect_precise_images'] == (ci, [vp, vp, ci])
    assert lib._pmx_sig['pmx_get_precise_image_maps'] == (ci, [vp, ci, vp, vp, ci, ci])
    res, args = lib._pmx_sig['pmx_precise_images_table_bytes']
    assert res is ci and args[0] is vp and args[1]._type_ is ctypes.c_size_t
    # the descriptor mirrors the header's struct: pointer, orig_h, orig_w, n_scales, 16 ints
    d = native.PmxPreciseImage
    assert [f[0] for f in d._fields_] == ['bgr', 'orig_h', 'orig_w', 'n_scales', 'scaled_hw']
    assert ctypes.sizeof(d) == ctypes.sizeof(ctypes.c_void_p) + 19 * 4 + (4 if ctypes.sizeof(ctypes.c_void_p) == 8 else 0)
    assert 'pmx_precise_images.hip' in [s for s, _ in native.SOURCES]


class StubEngine(object):
    """records the calls a detector makes; results: one record per image whose n_people encodes the image's height"""

    def __init__(self, raise_for=()):
        self.calls = []
        self.raise_for = set(raise_for)
        self._last = []

    def detect_precise_images(self, imgs, sizes):
        self.calls.append(('detect_precise_images', [im.shape for im in imgs], [[list(x) for x in s] for s in sizes]))
        self._last = imgs

    def precise_image_maps(self, k):
        h, w = self._last[k].shape[:2]
        return np.full((38, h, w), h, np.float32), np.full((19, h, w), w, np.float32)

    def results(self):
        native = pkg('native')
        rec = np.zeros(len(self._last), dtype=native.result_dtype(4))
        for k, im in enumerate(self._last):
            rec[k]['n_peaks'] = 5
            rec[k]['n_people'] = 1
            rec[k]['scores'][0] = float(im.shape[0])
            if im.shape[:2] in self.raise_for:
                rec[k]['status'] = native.IMG_TRIPLE_MATCH
        return rec

    # the same-size sequence
    def precise_begin(self, h, w, n):
        self.calls.append(('precise_begin', h, w, n))

    def precise_add_scale(self, batch, sh, sw, slot=None):
        self.calls.append(('precise_add_scale', sh, sw, slot))

    def precise_finish(self):
        self.calls.append(('precise_finish',))

    def postprocess(self, h, w, img_len, scale_xy=None):
        self.calls.append(('postprocess', h, w, img_len))
        self._last = [np.zeros((h, w, 3), np.uint8)] * self._n


def _detector(cap=(8, 368, 368), raise_for=()):
    PD = pkg('pose_detector')
    det = PD.PoseDetector.__new__(PD.PoseDetector)
    det.model = None
    det._weights = {'x': 1}
    det.engine = StubEngine(raise_for)
    det._cap = cap
    grown = []

    def make_engine(mb, mh, mw):
        grown.append((mb, mh, mw))
        det._cap = (mb, mh, mw)
    det._make_engine = make_engine
    det._grown = grown
    return det


def _imgs(shapes):
    return [np.zeros(s + (3,), np.uint8) for s in shapes]


def _ref_sizes(h, w):
    """reference pose_detector.py:441-443"""
    out = []
    for scale in (0.5, 1.0, 1.5, 2.0):
        m = scale * 368 / min(h, w)
        out.append([math.ceil(h * m), math.ceil(w * m)])
    return out


def test_mixed_list_runs_the_new_path_with_the_reference_scaled_sizes():
    det = _detector()
    shapes = [(480, 640), (640, 480), (375, 500)]
    res = det.detect_precise_batch(_imgs(shapes))
    kinds = [c[0] for c in det.engine.calls]
    assert kinds == ['detect_precise_images']                       # (no ValueError, no precise_* sequence)
    _, got_shapes, got_sizes = det.engine.calls[0]
    assert [s[:2] for s in got_shapes] == shapes
    assert got_sizes == [_ref_sizes(h, w) for h, w in shapes]
    assert [float(r[1][0]) for r in res] == [480.0, 640.0, 375.0]
    assert det.all_peaks is None


def test_chunks_respect_the_pixel_budget_and_results_keep_the_callers_order():
    PD = pkg('pose_detector')
    assert PD.precise_chunks([5, 5, 5, 5], 10, 8) == [[0, 1], [2, 3]]
    assert PD.precise_chunks([5, 20, 5], 10, 8) == [[0], [1], [2]]       # (an image over the budget alone: the library refuses it)
    assert PD.precise_chunks([1] * 5, 100, 2) == [[0, 1], [2, 3], [4]]
    det = _detector()
    det.precise_images_per_call = 2
    shapes = [(480, 640), (640, 480), (375, 500), (500, 375), (427, 640)]
    res = det.detect_precise_batch(_imgs(shapes), fetch_maps=True)
    px = [sum(-(-h // 8) * 8 * (-(-w // 8) * 8) for h, w in _ref_sizes(*s)) for s in shapes]
    assert len(det._grown) == 1                                           # grown ONCE, for the two largest images
    mb, mh, mw = det._cap
    assert mb * mh * mw >= sum(sorted(px)[-2:])
    calls = det.engine.calls
    assert len(calls) >= 2
    seen = []
    for _, cs, _ in calls:
        idx = [shapes.index(s[:2]) for s in cs]
        assert sum(px[i] for i in idx) <= mb * mh * mw and len(idx) <= mb
        seen += idx
    assert seen == list(range(len(shapes)))
    assert [float(r[1][0]) for r in res] == [float(h) for h, _ in shapes]
    assert isinstance(det.pafs, list) and [p.shape[1:] for p in det.pafs] == shapes
    assert all(float(p[0, 0, 0]) == h for p, (h, _) in zip(det.pafs, shapes))


def test_return_exceptions_behaves_as_for_a_same_size_batch():
    shapes = [(480, 640), (640, 480), (375, 500)]
    det = _detector(raise_for=[(640, 480)])
    with pytest.raises(IndexError):
        det.detect_precise_batch(_imgs(shapes))
    det = _detector(raise_for=[(640, 480)])
    res = det.detect_precise_batch(_imgs(shapes), return_exceptions=True)
    assert isinstance(res[1], IndexError) and float(res[0][1][0]) == 480.0 and float(res[2][1][0]) == 375.0


def test_same_size_list_keeps_the_sequence_path():
    det = _detector()
    det.engine._n = 2
    det.detect_precise_batch(_imgs([(480, 640), (480, 640)]))
    kinds = [c[0] for c in det.engine.calls]
    assert kinds == ['precise_begin'] + ['precise_add_scale'] * 4 + ['precise_finish', 'postprocess']
    assert det.engine.calls[0] == ('precise_begin', 480, 640, 2)
    assert sorted((c[1], c[2]) for c in det.engine.calls[1:5]) == sorted(tuple(s) for s in _ref_sizes(480, 640))
