"""Deterministic call scripts, one per kind of context, for the stream and thread tests (test_gpu_streams.py, test_gpu_threads.py,
threads_child.py).  A script takes an open engine, runs a fixed sequence of calls on fixed inputs and returns {name: array}; run serially
in the main thread it is the reference that every other run -- on a caller's stream, in a thread, in a fresh process -- must equal bit for
bit.  The shapes are the smallest the suite uses for whole pipelines (test_gpu_context_lifetime.py)."""
import hashlib
import importlib

import numpy as np

PKG = 'chainer_realtime_multi-person_pose_estimation_amd'
POSE = dict(max_batch=4, max_h=96, max_w=128)
FACE = dict(max_batch=2, max_h=64, max_w=64, arch='facenet')
RENDER = dict(max_batch=1, max_h=64, max_w=64)
PRECISE_SCALES = [(24, 32), (48, 64), (72, 96), (96, 128)]
FACE_BOXES = [(5, 5, 60, 70, 0), (30, 20, 110, 90, 1), (-10, 40, 50, 120, 0)]          # three boxes at max_batch 2: two chunks


def _pkg(sub):
    return importlib.import_module(PKG + '.' + sub)


def u8(seed, *shape):
    return np.random.default_rng(seed).integers(0, 256, shape + (3,), dtype=np.uint8)


def pose_weights(native):
    """Synthetic weights whose last layers are calibrated on one fixed image (weights.calibrate_head), so that the post-process finds peaks
    and people: records that differ between inputs.  Deterministic: the calibration forward is itself bit-reproducible."""
    W = _pkg('weights')
    w = W.synthetic_weights(0)
    eng = native.Engine(0, max_batch=1, max_h=96, max_w=128)
    try:
        eng.set_weights(w)
        eng.forward_u8(u8(0, 1, 96, 128))
        paf, heat = eng.get_maps()
    finally:
        eng.close()
    return W.calibrate_head(w, paf[0], heat[0])


def face_weights():
    return _pkg('weights').synthetic_weights(0, 'facenet')


def records(res):
    """The result records without their capacity-dependent padding: per image the info words and the n_people live rows."""
    out = {}
    for i, r in enumerate(res):
        n = int(r['n_people'])
        out['%d.info' % i] = np.array([r['n_people'], r['n_peaks'], r['status'], r['n_subsets_raw']], np.int32)
        out['%d.scores' % i] = np.array(r['scores'][:n], np.float64)
        out['%d.poses' % i] = np.array(r['poses'][:n], np.float64)
    return out


def _put(out, prefix, d):
    for k, v in d.items():
        out[prefix + '.' + k] = v


def precise_sequence(eng, img, scales=PRECISE_SCALES):
    """detect_precise as a sequence, the largest scale first: with four scales, the four lanes"""
    h, w = img.shape[:2]
    eng.precise_begin(h, w, 1)
    for slot, (sh, sw) in sorted(enumerate(scales), key=lambda t: -t[1][0]):
        eng.precise_add_scale(img[None], sh, sw, slot=slot)
    eng.precise_finish()
    eng.postprocess(h, w, img_len=w)


def pose_script(eng):
    """detect_batch at batch 1 and 2, a mixed detect_images (two size classes, one of them twice and not consecutive), the four-lane
    precise sequence and a post-process that outgrows tiny capacities."""
    out = {}
    for B in (1, 2):
        eng.detect_batch(u8(10 + B, B, 96, 128), map_h=80, map_w=112)
        _put(out, 'batch%d' % B, records(eng.results()))
        paf, heat = eng.get_maps()
        out['batch%d.paf' % B], out['batch%d.heat' % B] = paf, heat
    if eng.max_batch >= 3:          # (a batch-2 context runs the script without its three-image call)
        eng.detect_images([u8(21, 60, 90), u8(22, 96, 128), u8(23, 50, 70)], [(64, 96), (96, 128), (64, 96)], [(60, 90), (96, 128), (50, 70)])
        _put(out, 'mixed', records(eng.results()))
        for i in range(3):
            out['mixed.paf%d' % i], out['mixed.heat%d' % i] = eng.image_maps(i)
    precise_sequence(eng, u8(31, 48, 64))
    _put(out, 'precise', records(eng.results()))
    out['precise.peaks'] = np.asarray(eng.peaks(0))
    rng = np.random.default_rng(41)
    eng.set_capacities(peaks_per_joint=2, subsets=2, people=1)
    eng.set_maps((rng.standard_normal((1, 38, 12, 16)) * 0.5).astype('f'), (rng.random((1, 19, 12, 16)) * 0.5).astype('f'))
    eng.postprocess(80, 112, img_len=112)
    _put(out, 'grown', records(eng.results()))
    out['grown.peaks'] = np.asarray(eng.peaks(0))
    assert eng.capacities()['peaks_per_joint'] > 2
    return out


def face_script(eng):
    """keypoints_boxes with three boxes on a batch-2 context: two chunks"""
    return {'face.kp': eng.keypoints_boxes(u8(51, 100, 120), FACE_BOXES, 0.05)}


def render_inputs(seed=61):
    """two images of about 100 x 120 with people, one face part on the first: what render_script draws"""
    rng = np.random.default_rng(seed)
    imgs = [u8(seed + 1, 100, 120), u8(seed + 2, 90, 110)]
    poses = []
    for n, im in zip((2, 1), imgs):
        p = np.zeros((n, 18, 3))
        p[:, :, 0] = rng.uniform(-5, im.shape[1] + 5, (n, 18))
        p[:, :, 1] = rng.uniform(-5, im.shape[0] + 5, (n, 18))
        p[:, :, 2] = np.where(rng.random((n, 18)) < 0.25, 0, 2)
        poses.append(p)
    box = (30, 10, 75, 55)
    kps = [[float(rng.uniform(0, 45)), float(rng.uniform(0, 45)), float(rng.random())] for _ in range(70)]
    kps[3] = kps[40] = None
    return imgs, poses, [[('face', box, kps)], []]


def render_script(eng):
    """render host -> host with the blend and one face part; needs no weights"""
    imgs, poses, parts = render_inputs()
    return {'render.%d' % i: c for i, c in enumerate(eng.render(imgs, poses, parts, blend=True))}


def same(got, want):
    """None, or a description of the first difference between two script results"""
    if sorted(got) != sorted(want):
        return 'keys differ: %r vs %r' % (sorted(got), sorted(want))
    for k in sorted(want):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if g.shape != w.shape or g.dtype != w.dtype or g.tobytes() != w.tobytes():
            return '%s differs (%s %r vs %s %r)' % (k, g.dtype, g.shape, w.dtype, w.shape)
    return None


def digests(result):
    """{name: SHA-256 of the array's dtype, shape and bytes}"""
    out = {}
    for k, v in result.items():
        a = np.ascontiguousarray(v)
        out[k] = hashlib.sha256(('%s %r ' % (a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()
    return out
