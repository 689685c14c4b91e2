"""GPU: the consumers of the post-process table sets (csrc/pp_tables.h) on ONE context, in turn and back again -- the uniform entry's own
set, the per-size cache of the mixed-size entry, the per-call staging of the precise image list -- and pmx_keypoints against the box
entry on one-pixel axes (the num == 1 branch of the grid), with and without the left / right mirror."""
import math

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

NET = 24                                              # context capacity 4 x 24 x 24: every call below fits


@pytest.fixture(scope='module')
def weights(native):
    """synthetic weights whose last stage is rescaled on one 64 x 64 image, so that peaks pass the threshold"""
    W = pkg('weights')
    raw = W.synthetic_weights(3)
    eng = native.Engine(0, max_batch=1, max_h=64, max_w=64)
    eng.set_weights(raw)
    eng.forward_u8(np.random.default_rng(5).integers(0, 256, (1, 64, 64, 3), dtype=np.uint8))
    paf, heat = eng.get_maps()
    eng.close()
    return W.calibrate_head(raw, paf[0], heat[0], heat_s=0.3, heat_t=0.0, paf_s=1.2)


def _engine(native, weights):
    eng = native.Engine(0, max_batch=4, max_h=NET, max_w=NET)
    eng.set_weights(weights)
    return eng


def _image_bytes(eng, i, rec):
    """peaks, connections, subsets and the defined part of the result record of image i, as bytes"""
    n = int(rec['n_people'])
    head = [int(rec[k]) for k in ('n_people', 'n_peaks', 'status', 'n_subsets_raw')]
    return (eng.peaks(i).tobytes(), eng.connections(i).tobytes(), eng.subsets(i).tobytes(), head, rec['scores'][:n].tobytes(),
            rec['poses'][:n].tobytes())


def _all_images(eng, n):
    recs = eng.results()
    return [_image_bytes(eng, i, recs[i]) for i in range(n)]


def test_table_consumers_in_turn_on_one_context(native, weights):
    rng = np.random.default_rng(11)
    paf = (rng.standard_normal((1, 38, 5, 7)) * 0.8).astype(np.float32)
    heat = (rng.standard_normal((1, 19, 5, 7)) * 0.3).astype(np.float32)
    mixed = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((20, 31), (33, 18), (15, 22))]
    net_hw, map_hw = [(16, 24), (24, 16), (16, 24)], [(21, 30), (31, 19), (18, 27)]
    precise = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((17, 23), (23, 17))]
    scaled = [[(math.ceil(im.shape[0] * s), math.ceil(im.shape[1] * s)) for s in (0.5, 1)] for im in precise]

    def a(eng):
        eng.set_maps(paf, heat)
        eng.postprocess(23, 31, img_len=31)
        return _all_images(eng, 1)

    def b(eng):
        eng.detect_images(mixed, net_hw, map_hw)
        return _all_images(eng, 3)

    def c(eng):
        eng.detect_precise_images(precise, scaled)
        return _all_images(eng, 2)

    eng = _engine(native, weights)
    a0 = a(eng)
    b0 = b(eng)
    a1 = a(eng)          # (the mixed call used to leave the context's own set clobbered)
    c0 = c(eng)
    a2 = a(eng)
    eng.close()
    assert a1 == a0 and a2 == a0
    for run, got in ((b, b0), (c, c0)):
        fresh = _engine(native, weights)
        want = run(fresh)
        fresh.close()
        assert got == want
    # (a) has something to compare: its maps are random with a spread of 0.3, every joint type has a smoothed maximum above the threshold
    counts = [[len(x[0]) // 40 for x in r] for r in (a0, b0, c0)]
    print('peaks per image (a, b, c):', counts, 'connections of (a):', len(a0[0][1]) // 32)
    assert counts[0][0] >= 18


@pytest.mark.parametrize('hw', [(9, 1), (1, 9)])
def test_keypoints_equal_the_box_entry_on_one_pixel_axes(native, hw):
    """pmx_keypoints with "kp_flip_x" and the box entry build their tables at different places (the context's own set, the call's
    staging): the same crop with the same flip gives the same rows"""
    FHW = pkg('weights')
    h, w = hw
    eng = native.Engine(0, max_batch=1, max_h=64, max_w=64, arch='handnet')
    eng.set_weights(FHW.synthetic_weights(9, 'handnet'))
    img = np.random.default_rng(13).integers(0, 256, (40, 50, 3), dtype=np.uint8)
    for flip in (0, 1):
        box = (7, 5, 7 + w, 5 + h, flip)
        got = eng.keypoints_boxes(img, [box], -1e30)[0]
        eng.forward_u8_boxes(img, [box])
        eng.set_option('kp_flip_x', flip)
        want = eng.keypoints(h, w, -1e30)[0]
        assert got.shape == (21, 4) and np.array_equal(got, want), (hw, flip, np.argwhere(got != want)[:5])
        assert got[:, 3].all()
    eng.close()
