"""TEST INFRASTRUCTURE -- what the verbatim reference returned on the post-process edge cases of tests/postprocess_edge_cases.py
(non-finite maps, exact ties at radius 0, other Gaussian radii, tiny maps, down-sampling), recorded once so that
tests/test_postprocess_edges_host.py can pin the NumPy oracle to it wherever the repository is checked out.

    python -m oracle.ref_edge_goldens     (authoring container only: needs the reference, oracle/_refimport.py)
        -> tests/golden/ref_pp_edges.npz  per pose case: all_peaks, connections as (limb, a, b, score) rows, poses, scores
                                          per key-point case: (channels, 4) rows (x, y, confidence, valid)

The inputs are regenerated from the case table by the tests; only the reference's answers are stored.  The reference reads its Gaussian
sigma from `entity.params['gaussian_sigma']`: the recorder sets it for the call and puts it back, as oracle/ref_goldens.py does with
`face_inference_img_size`.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPZ = os.path.join(ROOT, 'tests', 'golden', 'ref_pp_edges.npz')

_loaded = None


def load():
    """{key: array} of the committed recording."""
    global _loaded
    if _loaded is None:
        z = np.load(NPZ)
        _loaded = {k: z[k] for k in z.files}
    return _loaded


def flat_connections(conns):
    """list of 19 (k, 3) arrays -> (n, 4) float64 rows (limb, a, b, score)"""
    rows = [np.hstack([np.full((len(c), 1), float(l)), np.asarray(c, np.float64).reshape(-1, 3)]) for l, c in enumerate(conns)]
    return np.vstack(rows).reshape(-1, 4)


def keypoint_rows(kps):
    """list of [x, y, conf] | None -> (n, 4) float64 rows (x, y, confidence, valid); zeros where None"""
    return np.array([[0, 0, 0, 0] if k is None else [k[0], k[1], float(k[2]), 1] for k in kps], np.float64).reshape(-1, 4)


def kp_key(arch, size, flip):
    return 'kp_%s_%dx%d_flip%d' % (arch, size[0], size[1], flip)


def main():
    import warnings
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import postprocess_edge_cases as E
    from oracle import _refimport as R
    from oracle import postprocess_ref as P
    assert R.reference_available(), 'the reference is needed to record its answers'
    m = R.import_reference_modules()
    params = m['entity'].params
    assert m['pose_detector'].params is params and m['hand_detector'].params is params
    arr = {}

    for name, c in E.recorded_cases().items():
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')           # (0 x inf in the resize of the planted maps)
            heat = P.resize_images_ref(c['heat'], c['map_h'], c['map_w'])
            paf = P.resize_images_ref(c['paf'], c['map_h'], c['map_w'])
        old = params['gaussian_sigma']
        params['gaussian_sigma'] = c['sigma']
        try:
            ref = R.ref_postprocess(heat, paf, c['map_w'])
        finally:
            params['gaussian_sigma'] = old
        arr[name + '/all_peaks'] = np.asarray(ref['all_peaks'], np.float64).reshape(-1, 5)
        arr[name + '/connections'] = flat_connections(ref['connections'])
        arr[name + '/poses'] = np.asarray(ref['poses'], np.float64).reshape(-1, 18, 3)
        arr[name + '/scores'] = np.asarray(ref['scores'], np.float64).reshape(-1)

    for arch, n_maps, cls in (('handnet', 22, m['hand_detector'].HandDetector), ('facenet', 71, m['face_detector'].FaceDetector)):
        det = cls.__new__(cls)                    # compute_peaks_from_heatmaps reads `params` only
        for size in E.KP_SIZES:
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                up = P.resize_images_ref(E.keypoint_maps(n_maps), size[0], size[1])
                for flip in (0, 1):
                    maps = np.ascontiguousarray(up[:, :, ::-1]) if flip else up
                    arr[kp_key(arch, size, flip)] = keypoint_rows(det.compute_peaks_from_heatmaps(maps))

    np.savez_compressed(NPZ, **arr)
    print('wrote', NPZ, os.path.getsize(NPZ), 'bytes,', len(arr), 'arrays')


if __name__ == '__main__':
    main()
