"""GPU: detect_precise for a LIST of images of different sizes (include/pose_mi355x.h: pmx_detect_precise_images; csrc/pmx_precise_images.hip).
Every (image, scale) pair is a segment of one network forward on one stream; three segment-aware kernels do the u8 cubic resize + pad,
the x8 up-sampling and the crop + resize to the original size + ordered average.  Bars:
  * fp32: per image, the averaged maps, peaks, connections, subsets, poses and scores equal the begin / add_scale / finish sequence of that
    image alone, bit for bit, with the options that pin the plain kernels a segmented forward runs ("precise_plain" 1, "conv1_wino" 2);
  * f16 mode: the same against the DEFAULT f16 sequence (the f16 kernels are batch- and layout-invariant);
  * a permuted list permutes the results; the context handles many sizes, capacity growth and a refused oversized call."""
import sys

import numpy as np
import pytest

from conftest import ROOT, forward_plan, pkg

pytestmark = pytest.mark.gpu

# landscape, portrait, square, two equal sizes, one whose scale 1.0 is its original size (short side = inference_img_size)
SHAPES = [(72, 120), (130, 84), (96, 96), (72, 120), (368, 400)]


def _calibrated(native):
    W = pkg('weights')
    weights = W.synthetic_weights(0)
    eng = native.Engine(0, max_batch=1, max_h=368, max_w=368)
    eng.set_weights(weights)
    eng.forward_u8(np.random.default_rng(1234).integers(0, 256, (1, 368, 368, 3), dtype=np.uint8))
    paf, heat = eng.get_maps()
    eng.close()
    return W.calibrate_head(weights, paf[0], heat[0], heat_s=0.2, heat_t=-0.2, paf_s=1.2)      # (bench.precise_mode's crowd-like load)


def _images(shapes, seed=21):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in shapes]


def _sizes(det, imgs):
    return [det.precise_scaled_sizes(im.shape) for im in imgs]


def _padded_px(sizes):
    return sum((-(-h // 8) * 8) * (-(-w // 8) * 8) for h, w in sizes)


def _list_engine(native, weights, sizes, precision=0):
    """an engine whose pixel budget holds every pair of the list in one call"""
    n = len(sizes)
    px = sum(_padded_px(s) for s in sizes)
    eng = native.Engine(0, max_batch=n, max_h=368, max_w=-(-px // (n * 368 * 8)) * 8)
    eng.set_weights(weights)
    if precision:
        eng.set_option('precision', precision)
    return eng


def _outputs(eng, i):
    return dict(peaks=eng.peaks(i), connections=eng.connections(i), subsets=eng.subsets(i))


def _sequence(native, weights, img, sizes, precision=0, plain=True):
    """the existing device path for ONE image: begin / add_scale (largest first, as PoseDetector does) / finish + full-size post-process"""
    h, w = img.shape[:2]
    big = max(_padded_px([s]) for s in sizes)
    eng = native.Engine(0, max_batch=1, max_h=8, max_w=-(-big // 64) * 8)
    eng.set_weights(weights)
    if precision:
        eng.set_option('precision', precision)
    if plain:
        eng.set_option('precise_plain', 1)
        eng.set_option('conv1_wino', 2)
    try:
        eng.precise_begin(h, w, 1)
        for slot in sorted(range(len(sizes)), key=lambda k: -sizes[k][0] * sizes[k][1]):
            eng.precise_add_scale(img[None], sizes[slot][0], sizes[slot][1], slot=slot)
        eng.precise_finish()
        paf, heat = eng.get_maps()
        eng.postprocess(h, w, img_len=w)
        rec = eng.results()[0]
        return dict(paf=paf[0], heat=heat[0], rec=rec, **_outputs(eng, 0))
    finally:
        eng.close()


def _same_record(a, b):
    n = int(a['n_people'])
    assert int(b['n_people']) == n and int(a['n_peaks']) == int(b['n_peaks']) and int(a['status']) == int(b['status'])
    assert np.array_equal(a['poses'][:n], b['poses'][:n]) and np.array_equal(a['scores'][:n], b['scores'][:n])


def _assert_image_equal(eng, i, rec, ref):
    paf, heat = eng.precise_image_maps(i)
    assert np.array_equal(paf.view(np.uint32), ref['paf'].view(np.uint32)), (i, np.abs(paf - ref['paf']).max())
    assert np.array_equal(heat.view(np.uint32), ref['heat'].view(np.uint32)), (i, np.abs(heat - ref['heat']).max())
    _same_record(rec, ref['rec'])
    got = _outputs(eng, i)
    for k in ('peaks', 'connections', 'subsets'):
        assert np.array_equal(got[k], ref[k]), (i, k)


@pytest.fixture(scope='module')
def weights(native):
    return _calibrated(native)


@pytest.fixture(scope='module')
def fp32_refs(native, weights):
    PD = pkg('pose_detector')
    det = PD.PoseDetector.__new__(PD.PoseDetector)
    imgs = _images(SHAPES)
    sizes = _sizes(det, imgs)
    assert sizes[4][1] == (368, 400)                       # scale 1.0 of the last image IS its original size (the copy branch)
    return imgs, sizes, [_sequence(native, weights, im, s) for im, s in zip(imgs, sizes)]


def test_fp32_list_equals_the_plain_sequence_per_image_bit_for_bit(native, weights, fp32_refs):
    imgs, sizes, refs = fp32_refs
    eng = _list_engine(native, weights, sizes)
    plan, wino, _ = forward_plan(eng, lambda: eng.detect_precise_images(imgs, sizes), with_wino=True)
    assert not plan and not plan.wino_units and not plan.wino_tails        # no split-K, no unit mode: plain launches only
    assert {'conv1_2', 'conv2_1', 'conv4_4_CPM', 'Mconv1_stage2', 'Mconv5_stage6'} <= wino, wino
    rec = eng.results()
    assert len(rec) == len(imgs)
    people = peaks = 0
    for i in range(len(imgs)):
        _assert_image_equal(eng, i, rec[i], refs[i])
        people += int(rec[i]['n_people'])
        peaks += int(rec[i]['n_peaks'])
    assert people >= 3 and peaks >= 50, ('the fixture should find people', people, peaks)
    # the per-call tables: no per-size cache of the sequence path is touched
    assert eng.precise_table_stats()[0] == 0
    eng.close()


def test_permuted_list_and_single_image(native, weights, fp32_refs):
    imgs, sizes, refs = fp32_refs
    perm = [3, 0, 4, 2, 1]
    eng = _list_engine(native, weights, sizes)
    eng.detect_precise_images([imgs[i] for i in perm], [sizes[i] for i in perm])
    rec = eng.results()
    for k, i in enumerate(perm):
        _assert_image_equal(eng, k, rec[k], refs[i])
    # one image through the new entry point
    eng.detect_precise_images([imgs[1]], [sizes[1]])
    _assert_image_equal(eng, 0, eng.results()[0], refs[1])
    eng.close()


def test_f16_list_equals_the_default_f16_sequence(native, weights):
    PD = pkg('pose_detector')
    det = PD.PoseDetector.__new__(PD.PoseDetector)
    imgs = _images(SHAPES[:4], seed=22)
    sizes = _sizes(det, imgs)
    refs = [_sequence(native, weights, im, s, precision=2, plain=False) for im, s in zip(imgs, sizes)]
    eng = _list_engine(native, weights, sizes, precision=2)
    eng.detect_precise_images(imgs, sizes)
    rec = eng.results()
    for i in range(len(imgs)):
        _assert_image_equal(eng, i, rec[i], refs[i])
    eng.close()


def test_detector_mixed_list_equals_per_image_detect_precise(native, weights, fp32_refs):
    """PoseDetector.detect_precise_batch on a mixed list: chunks, caller's order, maps as lists"""
    PD = pkg('pose_detector')
    imgs, sizes, refs = fp32_refs
    det = PD.PoseDetector(weights=weights, device=0)
    det.precise_images_per_call = 2                        # three calls for five images
    res = det.detect_precise_batch(imgs, fetch_maps=True, return_exceptions=True)
    assert isinstance(det.pafs, list) and len(det.pafs) == len(imgs)
    for i in range(len(imgs)):
        assert np.array_equal(det.pafs[i], refs[i]['paf']) and np.array_equal(det.heatmaps[i], refs[i]['heat']), i
        n = int(refs[i]['rec']['n_people'])
        if n:
            assert np.array_equal(np.asarray(res[i][0]), refs[i]['rec']['poses'][:n]), i
            assert np.array_equal(np.asarray(res[i][1]), refs[i]['rec']['scores'][:n]), i
    det.engine.close()


def test_config5_frame_inside_a_mixed_list_vs_precise_ref(native):
    """the 482 x 642 frame of bench.precise_mode (its calibrated head) inside a mixed list, through the new path in fp32, against
    oracle/precise_ref with the bounds of test_config5_precise_482x642_native_network_vs_precise_ref"""
    sys.path.insert(0, ROOT)
    import bench
    PD, W = pkg('pose_detector'), pkg('weights')
    H, Wd = 482, 642
    img = np.random.default_rng(55).integers(0, 256, (H, Wd, 3), dtype=np.uint8)
    wts = W.synthetic_weights(0)
    det = PD.PoseDetector(weights=wts, device=0, max_size=(744, 984))
    cal = PD.resize_cubic_u8(img, int(np.ceil(Wd * 368 / min(H, Wd))), int(np.ceil(H * 368 / min(H, Wd))))
    cal, _ = det.pad_image(cal, 8, (104, 117, 123))
    det.engine.forward_u8(cal[None])
    paf0, heat0 = det.engine.get_maps()
    wts = W.calibrate_head(wts, paf0[0], heat0[0], heat_s=0.2, heat_t=-0.2, paf_s=1.2)
    det._weights = wts
    det.engine.set_weights({k: wts[k] for k in ('Mconv7_stage6_L1', 'Mconv7_stage6_L2')})
    others = _images([(200, 300), (300, 220)], seed=7)
    res = det.detect_precise_batch([others[0], img, others[1]], fetch_maps=True, return_exceptions=True)
    assert not isinstance(res[1], Exception), res[1]
    poses, scores = res[1]
    det.pafs, det.heatmaps = det.pafs[1], det.heatmaps[1]
    # precise_match reads the frame's peaks from det.all_peaks: the frame alone through the same entry point gives them
    det.engine.detect_precise_images([img], [det.precise_scaled_sizes(img.shape)])
    det.all_peaks = det.engine.peaks(0)
    m = bench.precise_match(det, img, wts, poses, scores)
    print('\n[precise 482x642 in a mixed list] %d people; vs precise_ref: %s' % (len(scores), m))
    assert 'error' not in m and 'oracle_raised' not in m, m
    assert len(det.all_peaks) >= 300 and len(scores) >= 10
    assert m['max_abs_diff_averaged_maps_over_scale'] <= 2e-5
    assert m['all_mismatches_are_near_ties'] and m['max_margin_of_a_mismatch'] <= 1e-5
    assert m['max_abs_peak_score_diff'] <= 1e-4 and m['max_abs_score_diff_matched_people'] <= 1e-4
    assert m['matched_people'] >= 0.9 * m['people_cpu']
    det.engine.close()


def test_many_sizes_through_one_context(native, weights):
    """>= 40 distinct original sizes, several calls in a row on one context: every call equals a fresh context, and the table memory the
    context holds is bounded by the largest call, not by the sizes seen"""
    PD = pkg('pose_detector')
    det = PD.PoseDetector.__new__(PD.PoseDetector)
    rng = np.random.default_rng(40)
    shapes = []
    while len(shapes) < 42:                                 # (aspect ratios up to 4:3: the 2.0 scale stays near 736 x 984)
        h = int(rng.integers(64, 112))
        s = (h, int(rng.integers(-(-h * 3 // 4), h * 4 // 3 + 1)))
        if s not in shapes:
            shapes.append(s)
    imgs = _images(shapes, seed=41)
    sizes = _sizes(det, imgs)
    calls = [list(range(k, k + 6)) for k in range(0, 42, 6)]
    eng = _list_engine(native, weights, [max(sizes, key=_padded_px)] * 6)
    table_bytes = []
    for ci, call in enumerate(calls):
        eng.detect_precise_images([imgs[i] for i in call], [sizes[i] for i in call])
        rec = eng.results()
        table_bytes.append(eng.precise_images_table_bytes())
        if ci in (0, 3, len(calls) - 1):
            fresh = _list_engine(native, weights, [sizes[i] for i in call])
            fresh.detect_precise_images([imgs[i] for i in call], [sizes[i] for i in call])
            frec = fresh.results()
            for k in range(len(call)):
                _same_record(rec[k], frec[k])
                a, b = eng.precise_image_maps(k), fresh.precise_image_maps(k)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (ci, k)
                for key, v in _outputs(fresh, k).items():
                    assert np.array_equal(_outputs(eng, k)[key], v), (ci, k, key)
            fresh.close()
    assert max(table_bytes) <= 2 * min(table_bytes), table_bytes             # (per call, grown to the largest call; no per-size growth)
    assert eng.precise_table_stats()[0] == 0
    eng.close()


def test_capacity_growth_reruns_the_postprocess_with_live_tables(native, weights, fp32_refs):
    imgs, sizes, refs = fp32_refs
    eng = _list_engine(native, weights, sizes)
    eng.set_capacities(peaks_per_joint=2, subsets=2, people=1)
    eng.detect_precise_images(imgs, sizes)
    rec = eng.results()                                     # grows, re-runs every post-process call on the per-call tables
    caps = eng.capacities()
    assert caps['peaks_per_joint'] > 2 and caps['subsets'] > 2
    for i in range(len(imgs)):
        _same_record(rec[i], refs[i]['rec'])
        got = _outputs(eng, i)
        for k in ('peaks', 'connections', 'subsets'):
            assert np.array_equal(got[k], refs[i][k]), (i, k)
    eng.close()


def test_level3_capacity_refused_before_any_launch(native, weights, fp32_refs):
    imgs, sizes, refs = fp32_refs
    px = _padded_px(sizes[0])
    small = native.Engine(0, max_batch=len(imgs), max_h=8, max_w=-(-px // (len(imgs) * 64)) * 8)     # pixels for the first image only
    small.set_weights(weights)
    small.profile_reset()
    small.profile_enable(True)
    with pytest.raises(native.PmxError) as e:
        small.detect_precise_images(imgs, sizes)
    assert e.value.code == 5 and 'pixels' in str(e.value)
    assert small.profile() == []                            # nothing was launched
    small.profile_enable(False)
    small.detect_precise_images(imgs[:1], sizes[:1])        # the context still works
    _assert_image_equal(small, 0, small.results()[0], refs[0])
    small.close()
