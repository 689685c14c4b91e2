"""GPU: COCO key-point evaluation per image on the device (pmx_coco_eval; native.Engine.coco_eval, PoseDetector.evaluate_batch,
coco.evaluate) against the package's NumPy contract (coco.oks_matrix, coco.evaluate_image): the tables equal, the OKS values within 1e-13
(both sides take exp within about an ulp of terms <= 1 and add at most 17 of them in the same order: below 1e-14; the tolerance leaves a
factor of ten).  The images come from tests/coco_eval_cases.py; tests/test_coco_eval_host.py asserts the margins that make the equality
of the tables independent of those ulps.  Shapes: 0 / 1 / 2 / 20 / 21 / 25 detections (the cut at 20), 0 .. PMX_EVAL_MAX_GT ground truths,
1 / 3 / 70 images with empty ones first, in the middle and last."""
import json
import os

import numpy as np
import pytest

import coco_eval_cases as CS
from conftest import GOLDEN, pkg

pytestmark = pytest.mark.gpu

INVALID, CAPACITY, STATE = 1, 5, 6
KEYS = ('order', 'scores', 'areas', 'dt_match', 'dt_ig', 'gt_ig')
HEAD = ('Mconv7_stage6_L1', 'Mconv7_stage6_L2')


@pytest.fixture(scope='module', autouse=True)
def _torch_runtime_first():
    """torch brings its own HIP runtime; it initialises only while the library's has not opened the device yet in this process."""
    import torch
    torch.cuda.init()


@pytest.fixture(scope='module')
def coco():
    return pkg('coco')


@pytest.fixture(scope='module')
def eng(native):
    e = native.Engine(0, max_batch=1, max_h=64, max_w=64, arch='handnet')          # any kind of context, no weights
    yield e
    e.close()


@pytest.fixture(scope='module')
def want(coco):
    """the contract on every generated batch, computed once: name -> per image (result of evaluate_image, oks matrix)"""
    out = {}
    for name, images in CS.batches().items():
        rows = []
        for poses, scores, anns in images:
            d = coco.detections(poses, scores)
            oks = coco.oks_matrix(d, anns)
            rows.append((coco.evaluate_image(d, anns, oks=oks), oks))
        out[name] = rows
    return out


def _golden(name):
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    return z, z['poses'].reshape(tuple(z['poses_shape']))


@pytest.fixture(scope='module')
def det():
    """a detector that finds the eight people of the golden image e2e_people"""
    z, _ = _golden('e2e_people')
    w = pkg('weights').synthetic_weights(int(z['seed']))
    w[HEAD[0]], w[HEAD[1]] = (z['head_W1'], z['head_b1']), (z['head_W2'], z['head_b2'])
    d = pkg('pose_detector').PoseDetector(weights=w, device=0, max_batch=2, max_size=(368, 368))
    yield d
    d.engine.close()


def _annotations_of(poses, rng, extra_crowd=True):
    """annotation dictionaries near a detector's poses: the COCO points moved by less than a pixel and rounded"""
    anns = []
    for p in poses:
        rows = np.array([p[j] for j in CS.JOINT_OF_COCO], dtype=np.float64)
        lab = rows[:, 2] != 0
        rows[:, :2] = np.round(rows[:, :2] + rng.normal(0, 0.3, (17, 2))) * lab[:, None]
        rows[:, 2] = 2 * lab
        x, y = rows[lab, 0], rows[lab, 1]
        bbox = [float(x.min()), float(y.min()), float(x.max() - x.min()), float(y.max() - y.min())]
        anns.append(CS.annotation(rows, max(bbox[2] * bbox[3] * 0.5, 2000.0), bbox=bbox))
    if extra_crowd and anns:
        anns.append(dict(anns[0], iscrowd=1))
    return anns


def _same(got, ref, what, oks=None):
    if ref is None:
        assert got is None, what
        return
    assert got is not None, what
    for k in KEYS:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, (what, k, got[k].shape, got[k].dtype, ref[k].shape, ref[k].dtype)
        assert np.array_equal(got[k], ref[k]), (what, k, got[k], ref[k])
    if oks is not None:
        assert got['oks'].shape == oks.shape, (what, got['oks'].shape, oks.shape)
        if oks.size:
            err = np.abs(got['oks'] - oks).max()
            assert err <= 1e-13, (what, err)


def _run(engine, images, oks=True):
    return engine.coco_eval([im[2] for im in images], [im[0] for im in images], [im[1] for im in images], oks=oks)


def _bytes(results):
    return [None if e is None else {k: np.asarray(v).tobytes() for k, v in e.items()} for e in results]


@pytest.mark.parametrize('name', ['one', 'three', 'three_empty_last', 'seventy'])
def test_generated_batches_equal_the_contract_and_repeat(eng, want, name):
    images = CS.batches()[name]
    got = _run(eng, images)
    assert len(got) == len(images)
    for k, (e, (ref, oks)) in enumerate(zip(got, want[name])):
        _same(e, ref, '%s[%d]: %d detections, %d ground truths' % (name, k, len(images[k][1]), len(images[k][2])), oks)
    assert _bytes(_run(eng, images)) == _bytes(got)          # two runs, the same bytes (the OKS included)


def test_every_shape_is_in_the_batches(want):
    seen = {(len(im[1]), len(im[2])) for images in CS.batches().values() for im in images}
    assert set(CS.shape_list()) <= seen and {d for d, _ in seen} >= set(CS.DETS) and {g for _, g in seen} >= set(CS.GTS)
    # ... and the walks had work to do: matches, ignored matches and unmatched detections all occur
    m = np.concatenate([e['dt_match'].reshape(-1) for e, _ in want['seventy'] if e is not None])
    ig = np.concatenate([e['dt_ig'].reshape(-1) for e, _ in want['seventy'] if e is not None])
    assert (m >= 0).sum() > 100 and (m < 0).sum() > 100 and ig[m >= 0].any() and (~ig[m >= 0]).any() and ig[m < 0].any()


@pytest.mark.parametrize('name', sorted(CS.hand_cases()))
def test_hand_built_matching_cases_on_the_device(eng, name):
    poses, scores, anns, expected = CS.hand_cases()[name]
    CS.check_expected(eng.coco_eval([anns], [poses], [scores])[0], expected, name)


def test_all_hand_built_cases_in_one_call_and_an_image_with_neither(eng, coco):
    cases = sorted(CS.hand_cases().items())
    images = [(c[0], c[1], c[2]) for _, c in cases]
    images.insert(3, (np.zeros((0, 18, 3)), np.zeros(0), []))
    got = _run(eng, images, oks=False)
    assert got[3] is None and 'oks' not in got[0]
    for (name, c), e in zip(cases, got[:3] + got[4:]):
        CS.check_expected(e, c[3], name)
        _same(e, coco.evaluate_image(coco.detections(c[0], c[1]), c[2]), name)


# ---- the raw entry: outputs one by one, unused slots, error codes ---------------------------------------------------------------------
def _tables(native, coco, images):
    gts = [coco.ground_truths(im[2]) for im in images]
    counts = np.array([len(g['area']) for g in gts])
    tab = np.zeros((len(images), 2), np.int32)
    tab[:, 0], tab[:, 1] = np.cumsum(counts) - counts, counts
    rows = np.zeros(max(1, counts.sum()), coco.EVAL_GT_DTYPE)
    for g, off in zip(gts, tab[:, 0]):
        for key in coco.EVAL_GT_DTYPE.names:
            rows[key][off:off + len(g['area'])] = g[key]
    poses = np.ascontiguousarray(np.concatenate([np.asarray(im[0], np.float64).reshape(-1, 18, 3) for im in images] + [np.zeros((1, 18, 3))]))
    scores = np.ascontiguousarray(np.concatenate([np.asarray(im[1], np.float64).reshape(-1) for im in images] + [np.zeros(1)]))
    n_people = np.array([len(im[1]) for im in images], np.int32)
    return dict(images=tab, gts=rows, n_gts=int(counts.sum()), consts=coco.eval_consts(), poses=poses, scores=scores, n_people=n_people)


OUTS = ('det_count', 'det_order', 'det_scores', 'det_areas', 'dt_match', 'dt_ig', 'gt_ig', 'oks')


def _buffers(n, total, fill):
    shape = dict(det_count=((n,), np.int32), det_order=((n, 20), np.int32), det_scores=((n, 20), np.float64), det_areas=((n, 20), np.float64),
                 dt_match=((n, 3, 10, 20), np.int32), dt_ig=((n, 3, 10, 20), np.uint8), gt_ig=((max(total, 1), 3), np.uint8),
                 oks=((max(total, 1) * 20,), np.float64))
    out = {}
    for k, (s, t) in shape.items():
        out[k] = np.frombuffer(bytes([fill]) * (int(np.prod(s)) * np.dtype(t).itemsize), dtype=t).reshape(s).copy()
    return out


def _raw(native, engine, t, bufs, null=(), n_images=None, n_gts=None, in_place=False):
    P = native._ptr
    arg = lambda k: None if k in null else P(t[k])
    det = (None, None, None) if in_place else (arg('poses'), arg('scores'), arg('n_people'))
    rc = engine.lib.pmx_coco_eval(engine._ctx, arg('images'), len(t['images']) if n_images is None else n_images, arg('gts'),
                                  t['n_gts'] if n_gts is None else n_gts, arg('consts'), det[0], det[1], det[2],
                                  *[None if (k in null or k not in bufs) else P(bufs[k]) for k in OUTS])
    assert rc == 0 or engine.lib.pmx_last_error().decode().strip()
    return rc


def test_raw_outputs_alone_unused_slots_and_identical_bytes(native, eng, coco, want):
    images = CS.batches()['three']
    t = _tables(native, coco, images)
    n, total = len(images), t['n_gts']
    a, b = _buffers(n, total, 0x00), _buffers(n, total, 0xff)
    assert _raw(native, eng, t, a) == 0 and _raw(native, eng, t, b) == 0
    for k in OUTS:
        assert a[k].tobytes() == b[k].tobytes(), k          # every slot is written, and written the same
    assert list(a['det_count']) == [0, 20, 20]
    assert (a['det_order'][0] == -1).all() and (a['dt_match'][0] == -1).all() and not a['dt_ig'][0].any() and not a['det_scores'][0].any()
    ref = want['three'][1][0]
    assert np.array_equal(a['det_order'][1], ref['order']) and np.array_equal(a['dt_match'][1], ref['dt_match'])
    assert np.array_equal(a['gt_ig'][:64].T.astype(bool), ref['gt_ig'])
    for k in OUTS:                                           # each output alone
        one = _buffers(n, total, 0x55)
        assert _raw(native, eng, t, {k: one[k]}) == 0
        assert one[k].tobytes() == a[k].tobytes(), k


def test_error_codes_leave_the_context_usable(native, eng, coco, want):
    images = CS.batches()['three']
    n, good = len(images), _tables(native, coco, images)
    out = _buffers(n, good['n_gts'], 0x07)
    untouched = {k: v.tobytes() for k, v in out.items()}

    def changed(**kw):
        t = dict(good)
        for k, v in kw.items():
            t[k] = v(good[k].copy())
        return t

    def put(field, index, value):
        def f(arr):
            a = arr if field is None else arr[field]          # (a field is a strided view: no reshape)
            a[np.unravel_index(index, a.shape)] = value
            return arr
        return f

    bad = [
        dict(t=good, null=('images',)), dict(t=good, null=('gts',)), dict(t=good, null=('consts',)),
        dict(t=good, null=('scores',)), dict(t=good, null=('n_people',)), dict(t=good, null=OUTS),
        dict(t=good, n_images=0), dict(t=good, n_images=-1), dict(t=good, n_gts=-1),
        dict(t=good, n_gts=good['n_gts'] - 1),                                          # the last image's range ends past the table
        dict(t=changed(images=put(None, 2, -1))),                                        # gt0 < 0
        dict(t=changed(images=put(None, 3, -2))),                                        # a negative count of ground truths
        dict(t=changed(n_people=put(None, 1, -1))),                                      # ... of people
        dict(t=changed(gts=put('keypoints', 7, float('nan')))), dict(t=changed(gts=put('keypoints', 52, float('inf')))),
        dict(t=changed(gts=put('area', 3, float('nan')))), dict(t=changed(gts=put('bbox', 5, float('-inf')))),
        dict(t=changed(poses=put(None, 100, float('nan')))), dict(t=changed(poses=put(None, 54 * 30 + 1, float('inf')))),
        dict(t=changed(scores=put(None, 4, float('nan')))), dict(t=changed(scores=put(None, 44, float('inf')))),
        dict(t=changed(consts=put('joint', 2, 18))), dict(t=changed(consts=put('vars', 0, float('nan')))),
    ]
    for kw in bad:
        assert _raw(native, eng, bufs=out, **kw) == INVALID, {k: v for k, v in kw.items() if k != 't'}
        assert all(out[k].tobytes() == untouched[k] for k in out)                       # nothing was enqueued
    # one ground truth too many in one image: refused whole, and the context goes on
    P = CS.grid_points(100, 100)
    many = [(CS.pose_of(P)[None], np.ones(1), [CS.annotation(P + [k % 7, k // 7], 5000.0) for k in range(coco.EVAL_MAX_GT + 1)])]
    t = _tables(native, coco, many)
    assert _raw(native, eng, t, _buffers(1, t['n_gts'], 0)) == CAPACITY
    with pytest.raises(native.PmxError) as err:
        _run(eng, many)
    assert err.value.code == CAPACITY and 'PMX_EVAL_MAX_GT' in str(err.value)
    with pytest.raises(ValueError):
        eng.coco_eval([[], []], [np.zeros((0, 18, 3))], [np.zeros(0)])
    with pytest.raises(ValueError):
        eng.coco_eval([])
    # the in-place form before any post-process
    assert _raw(native, eng, good, out, in_place=True) == STATE
    assert all(out[k].tobytes() == untouched[k] for k in out)
    got = _run(eng, images)
    for e, (ref, oks) in zip(got, want['three']):
        _same(e, ref, 'after the errors', oks)
    full = [(im[0], im[1], im[2][:coco.EVAL_MAX_GT]) for im in many]          # exactly PMX_EVAL_MAX_GT is taken
    _same(_run(eng, full, oks=False)[0], coco.evaluate_image(coco.detections(*full[0][:2]), full[0][2]), 'PMX_EVAL_MAX_GT ground truths')


def test_a_facenet_context_and_the_callers_stream(native, want):
    import torch
    images = CS.batches()['three']
    e = native.Engine(0, max_batch=1, max_h=64, max_w=64, arch='facenet')
    try:
        for got, (ref, oks) in zip(_run(e, images), want['three']):
            _same(got, ref, 'facenet', oks)
        stream = torch.cuda.Stream()
        assert stream.cuda_stream != 0
        e.set_stream(stream.cuda_stream)
        try:
            for got, (ref, oks) in zip(_run(e, images), want['three']):
                _same(got, ref, 'side stream', oks)
        finally:
            e.set_stream(0)
    finally:
        e.close()


# ---- detections where the post-process left them ---------------------------------------------------------------------------------------
def test_records_in_place_equal_caller_arrays_and_nothing_else_moves(native, det, coco):
    PD = pkg('pose_detector')
    z, golden_poses = _golden('e2e_people')
    img = z['img']
    res = det.detect_batch([img, img[::-1].copy()])
    assert len(res[0][1]) == len(golden_poses) == 8
    rng = np.random.default_rng(11)
    gts = [_annotations_of(res[0][0], rng), _annotations_of(res[0][0][:3], rng, extra_crowd=False)]
    eng = det.engine
    maps = [m.copy() for m in eng.get_maps()]
    rec = eng.results().tobytes()
    in_place = eng.coco_eval(gts, oks=True)
    fetched = PD.unpack_results(eng.results())
    arrays = eng.coco_eval(gts, [r[0] for r in fetched], [r[1] for r in fetched], oks=True)
    assert _bytes(in_place) == _bytes(arrays)
    for k in range(2):
        _same(in_place[k], coco.evaluate_image(coco.detections(*res[k]), gts[k]), 'image %d' % k, coco.oks_matrix(coco.detections(*res[k]), gts[k]))
    assert (in_place[0]['dt_match'][0, 0] >= 0).sum() == 8          # every person finds its annotation at OKS 0.5
    assert eng.results().tobytes() == rec and all(np.array_equal(a, b) for a, b in zip(eng.get_maps(), maps))
    # the first image alone: fewer images than records is allowed, more is a state error
    assert _bytes(eng.coco_eval(gts[:1], oks=True)) == _bytes(in_place[:1])
    with pytest.raises(native.PmxError) as err:
        eng.coco_eval(gts + gts[:1])
    assert err.value.code == STATE
    # evaluate_batch is the two steps in one
    ev, poses, scores = det.evaluate_batch([img, img[::-1].copy()], gts)
    assert _bytes(ev) == _bytes([{k: e[k] for k in KEYS} for e in in_place])
    assert all(np.array_equal(p, r[0]) and np.array_equal(s, r[1]) for p, s, r in zip(poses, scores, res))


def test_evaluate_over_an_annotation_file_equals_the_host_pipeline(native, det, coco, tmp_path):
    PD = pkg('pose_detector')
    rng = np.random.default_rng(13)
    pixels = {7: _golden('e2e_people')[0]['img'], 4: _golden('e2e_person')[0]['img'], 9: rng.integers(0, 256, (48, 48, 3), dtype=np.uint8),
              2: rng.integers(0, 256, (48, 48, 3), dtype=np.uint8)}
    alone = {k: det.detect_batch([im])[0] for k, im in pixels.items()}
    assert len(alone[7][1]) == 8
    data = {'images': [], 'annotations': [], 'categories': [{'id': 1, 'name': 'person'}]}
    P = CS.grid_points(5, 5, step=8.0)
    anns_of = {7: _annotations_of(alone[7][0], rng), 4: _annotations_of(_golden('e2e_person')[1], rng),
               9: [CS.annotation(P + [k % 5, k // 100], 900.0) for k in range(coco.EVAL_MAX_GT + 1)],          # too many for the device entry
               2: []}                                                                                          # an image without annotations
    for img_id, im in pixels.items():
        data['images'].append({'id': img_id, 'file_name': 'im%d.png' % img_id, 'height': im.shape[0], 'width': im.shape[1]})
        PD.imwrite_bgr(str(tmp_path / ('im%d.png' % img_id)), im)
        for a in anns_of[img_id]:
            data['annotations'].append(dict(a, id=len(data['annotations']) + 1, image_id=img_id, segmentation=[]))
    (tmp_path / 'ann.json').write_text(json.dumps(data))
    ds = coco.CocoKeypoints(str(tmp_path / 'ann.json'), mode='eval')
    assert ds.img_ids == [4, 7, 9] and sorted(ds.images) == [2, 4, 7, 9]
    seen = []
    out = coco.evaluate(ds, det, str(tmp_path), batch=3, on_batch=lambda done, total: seen.append((done, total)))
    assert seen == [(3, 4), (4, 4)]
    ids = [2, 4, 7, 9]
    per_image = [coco.evaluate_image(coco.detections(*alone[k]), ds.annotations(k)) for k in ids]
    precision, recall = coco.accumulate(per_image)
    summary = coco.summarize(precision, recall)
    assert list(out)[:10] == list(coco.SUMMARY_KEYS) and all(out[k] == summary[k] for k in summary), (summary, {k: out[k] for k in summary})
    assert np.array_equal(out['precision'], precision) and np.array_equal(out['recall'], recall)
    assert out['results'] == coco.results(ids, [alone[k][0] for k in ids], [alone[k][1] for k in ids])
    for e, ref, k in zip(out['per_image'], per_image, ids):
        _same(e, ref, 'image id %d' % k)
    assert 0 < out['AP'] <= 1 and out['AR'] > 0
    # a chosen subset, one image per call
    sub = coco.evaluate(ds, det, str(tmp_path), batch=1, img_ids=[7])
    one = coco.summarize(*coco.accumulate([per_image[2]]))
    assert all(sub[k] == one[k] for k in one) and sub['AP50'] > 0.9
    # detect_precise's records (post-processed at the original size) are evaluated in place just the same
    ev, poses, scores = det.evaluate_batch([pixels[9]], [ds.annotations(9)[:40]], precise=True)
    p, s = det.detect_precise_batch([pixels[9]])[0]
    assert np.array_equal(poses[0], p) and np.array_equal(scores[0], s)
    _same(ev[0], coco.evaluate_image(coco.detections(p, s), ds.annotations(9)[:40]), 'precise')
