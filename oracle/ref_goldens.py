"""TEST INFRASTRUCTURE -- what the verbatim reference returned for the inputs of tests/test_oracle_vs_reference.py and the
reference checks of tests/test_reference_network.py, recorded once so that those tests run wherever the repository is checked out.

    python -m oracle.ref_goldens          (authoring container only: needs the reference, oracle/_refimport.py)
        -> tests/golden/ref_checks.npz    arrays (maps, peaks, poses, scores, label maps)
           tests/golden/ref_checks.json   everything else (layer tables, helper results, crop boxes; crops as digests)

The inputs are regenerated from the same seeds by the tests; only the reference's answers are stored.  Networks run on the torch-CPU
conv with ONE thread here and in the tests (oneDNN's summation order depends on the thread count), so that the bit-for-bit checks
compare like with like.  Crops are stored as SHA-256 digests of their values (`digest`), which only equal arrays reproduce.
"""
import hashlib
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPZ = os.path.join(ROOT, 'tests', 'golden', 'ref_checks.npz')
JSON = os.path.join(ROOT, 'tests', 'golden', 'ref_checks.json')
PP_CASES = [(11, 2, 0.0), (12, 7, 0.02), (13, 10, 0.03)]
KP_CASES = [('facenet', None), ('handnet', 'right'), ('handnet', 'left')]


def digest(a):
    """SHA-256 over the shape and the float64 values of an array: equal digests <=> np.array_equal (for the integer / float data here)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return hashlib.sha256(repr(a.shape).encode() + a.tobytes()).hexdigest()


def plain(v):
    """NumPy scalars / tuples / arrays -> JSON types (ints stay ints, floats round-trip exactly)."""
    if isinstance(v, dict):
        return {str(k): plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple, np.ndarray)):
        return [plain(x) for x in v]
    if isinstance(v, (bool, np.bool_)):
        return bool(v)
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        return float(v)
    return v


_loaded = None


def load():
    """(arrays, json) of the committed recording."""
    global _loaded
    if _loaded is None:
        z = np.load(NPZ)
        _loaded = ({k: z[k] for k in z.files}, json.load(open(JSON)))
    return _loaded


def one_thread():
    """Set torch to one CPU thread; returns the previous count."""
    import torch
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    return n


# ---- the recording (reference side of each test, same inputs and rng streams as the tests) ----------------------------------------
def main():
    import contextlib
    import importlib
    import io
    import sys
    import tempfile
    sys.path.insert(0, ROOT)
    from oracle import _refimport as R
    from oracle import fixtures as Fx
    from oracle import network_ref as N
    from oracle import postprocess_ref as P
    from oracle import precise_ref, resize_ref
    W = importlib.import_module('chainer_realtime_multi-person_pose_estimation_amd.weights')
    assert R.reference_available(), 'the reference is needed to record its answers'
    one_thread()
    arr, js = {}, {}

    # test_oracle_vs_reference.py::test_postprocess_matches_verbatim_reference
    for seed, n, noise in PP_CASES:
        heat, paf, _ = Fx.synthetic_maps(seed, n, 46, 46, 1.0, 0.9, noise=noise, height_range=(0.3, 0.7), drop_prob=0.15)
        ref = R.ref_postprocess(P.resize_images_ref(heat, 320, 320), P.resize_images_ref(paf, 320, 320), 320, orig_w=640, orig_h=480)
        arr['pp%d_all_peaks' % seed] = np.asarray(ref['all_peaks'], np.float64)
        for l, c in enumerate(ref['connections']):
            arr['pp%d_conn%02d' % (seed, l)] = np.asarray(c, np.float64)
        arr['pp%d_poses' % seed] = np.asarray(ref['poses'], np.float64)
        arr['pp%d_scores' % seed] = np.asarray(ref['scores'], np.float64)

    # ::test_label_renderer_matches_reference_generator
    _, _, det, gen = R.import_reference()
    _, _, poses = Fx.synthetic_maps(5, 4, 40, 52, 1.2, 1.0)
    img = np.zeros((40, 52, 3), 'uint8')
    arr['gen_heat'] = gen.generate_heatmaps(img, poses, 1.2)
    arr['gen_paf'] = gen.generate_pafs(img, poses, 1.0)

    # ::test_host_helpers_match_reference
    rng = np.random.default_rng(0)
    sizes = []
    for _ in range(50):
        h, w = int(rng.integers(20, 2000)), int(rng.integers(20, 2000))
        for t in (368, 320):
            rw, rh = det.compute_optimal_size(np.zeros((h, w, 3), 'uint8'), t)
            sizes.append([h, w, t, int(rw), int(rh)])
    js['optimal_sizes'] = sizes
    arr['preprocess'] = det.preprocess(rng.integers(0, 256, (9, 13, 3), dtype=np.uint8))

    # ::test_demo_chain_helpers_match_reference
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (200, 300, 3), dtype=np.uint8)
    rows = []
    for _ in range(300):
        pose = np.zeros((18, 3))
        pose[:, :2] = rng.uniform(-20, 320, (18, 2))
        pose[:, 2] = (rng.random(18) > 0.3) * 2
        ul = det.get_unit_length(pose.copy())
        u = ul if np.isfinite(ul) and ul > 1 else 20.0
        row = {'unit_length': None if np.isnan(ul) else float(ul)}
        try:
            fr = det.crop_face(img, pose.copy(), u)
            hr = det.crop_hands(img, pose.copy(), 25.0)
        except ValueError:
            row['raised'] = True
            rows.append(row)
            continue
        row['face'] = [None if fr[0] is None else digest(fr[0]), plain(fr[1])]
        row['hands'] = {side: None if hr[side] is None else {'bbox': plain(hr[side]['bbox']), 'img': digest(hr[side]['img'])}
                        for side in ('left', 'right')}
        rows.append(row)
    js['demo_chain'] = rows

    # ::test_crop_person_and_rect_crop_face_match_reference
    m = R.import_reference_modules()
    m['pose_detector'].sys = sys
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (240, 320, 3), dtype=np.uint8)
    rows = []
    for _ in range(400):
        pose = np.zeros((18, 3))
        pose[:, :2] = rng.uniform(5, 300, (18, 2))
        pose[:, 2] = (rng.random(18) > rng.choice([0.2, 0.6, 0.9])) * 2
        u = np.float64(rng.uniform(5, 40))
        try:
            r = det.crop_person(img, pose.copy(), u)
        except (IndexError, ValueError, AttributeError):
            rows.append(None)
            continue
        rows.append({'bbox': [int(v) for v in r[1]], 'img': digest(r[0])})
    js['crop_person'] = rows
    rows = []
    for _ in range(200):
        rect = (int(rng.integers(0, 300)), int(rng.integers(0, 220)), int(rng.integers(4, 120)), int(rng.integers(4, 120)))
        try:
            a = m['face_detector'].crop_face(img, rect)
        except ValueError:
            rows.append(None)
            continue
        rows.append({'bbox': plain(a[1]), 'img': digest(a[0])})
    js['rect_crop_face'] = rows
    js['entity'] = {k: plain(m['entity'].params[k]) for k in ('face_crop_scale', 'fingers_indices', 'face_line_indices', 'coco_joint_indices')}

    # test_reference_network.py: layer tables, networks (all stages), PoseDetector call, detect_precise, keypoint detectors
    js['layer_tables'] = {arch: plain(R.ref_layer_table(arch)) for arch in ('posenet', 'facenet', 'handnet')}

    def x_of(arch, seed, h, w):
        im = np.random.default_rng(seed + 1000).integers(0, 256, (1, h, w, 3), dtype=np.uint8)
        div = 255.0 if arch == 'posenet' else 256.0
        return (im.astype(np.float32) / np.float32(div) - np.float32(0.5)).transpose(0, 3, 1, 2)
    rp, rh = R.ref_network_forward('posenet', W.synthetic_weights(0), x_of('posenet', 7, 64, 96), all_stages=True)
    for s in range(6):
        arr['net_posenet_stage%d_paf' % s], arr['net_posenet_stage%d_heat' % s] = rp[s], rh[s]
    for arch in ('facenet', 'handnet'):
        for s, h in enumerate(R.ref_network_forward(arch, W.synthetic_weights(1, arch), x_of(arch, 8, 56, 72), all_stages=True)):
            arr['net_%s_stage%d_heat' % (arch, s)] = h

    w = W.synthetic_weights(3)
    img = np.random.default_rng(5).integers(0, 256, (70, 90, 3), dtype=np.uint8)
    in_w, in_h = P.compute_optimal_size(70, 90, 368)
    small = resize_ref.resize_linear_u8(img, in_w, in_h)
    paf, heat = N.forward(w, P.preprocess(small))
    w = W.calibrate_head(w, paf[0], heat[0])
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, 'coco_posenet.npz')
        W.save_npz(path, w)
        det_w = R.ref_pose_detector(weights_file=path)
    poses, scores = R.ref_call(det_w, img)
    arr['call_poses'], arr['call_scores'] = np.asarray(poses, np.float64), np.asarray(scores, np.float64)

    w = W.synthetic_weights(2)
    img = np.random.default_rng(6).integers(0, 256, (40, 56, 3), dtype=np.uint8)
    paf, heat = N.forward(w, P.preprocess(resize_ref.resize_linear_u8(img, 368 * 56 // 40 // 8 * 8, 368)))
    w = W.calibrate_head(w, paf[0], heat[0], heat_s=0.2, heat_t=-0.2, paf_s=1.2)
    det_p = R.ref_pose_detector(w, precise=True)
    poses, _ = R.ref_call(det_p, img)
    arr['precise_pafs'], arr['precise_heats'] = det_p.pafs, det_p.heatmaps
    arr['precise_poses'] = np.asarray(poses, np.float64).reshape(-1, 18, 3)

    kp = {}
    for arch, hand_type in KP_CASES:
        w = W.synthetic_weights(4, arch)
        img = np.random.default_rng(9).integers(0, 256, (60, 52, 3), dtype=np.uint8)
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, 'w.npz')
            W.save_npz(path, w)
            with contextlib.redirect_stdout(io.StringIO()):
                d = (m['face_detector'].FaceDetector if arch == 'facenet' else m['hand_detector'].HandDetector)(arch, path, device=-1)
        key = 'face_inference_img_size' if arch == 'facenet' else 'hand_inference_img_size'
        old = m['entity'].params[key]
        m['entity'].params[key] = 64
        try:
            ref = d(img) if hand_type is None else d(img, hand_type=hand_type)
        finally:
            m['entity'].params[key] = old
        kp['%s-%s' % (arch, hand_type)] = [None if a is None else plain(a[:3]) for a in ref]
    js['keypoints'] = kp
    js['keypoint_thresh'] = {arch: float(m['entity'].params['face_heatmap_peak_thresh' if arch == 'facenet' else 'hand_heatmap_peak_thresh'])
                             for arch in ('facenet', 'handnet')}

    np.savez_compressed(NPZ, **{k: np.asarray(v) for k, v in arr.items()})
    with open(JSON, 'w') as f:
        json.dump(js, f, separators=(',', ':'))
    print('wrote', NPZ, os.path.getsize(NPZ), JSON, os.path.getsize(JSON))


if __name__ == '__main__':
    main()
