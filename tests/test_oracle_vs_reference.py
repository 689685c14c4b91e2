"""CPU: the oracle against what the VERBATIM reference functions returned on the same inputs -- recorded by
oracle/ref_goldens.py (tests/golden/ref_checks.*, through oracle/_refimport.py where the reference exists), so that these
checks run everywhere.  Crops are compared through their value digests (oracle/ref_goldens.py::digest)."""
import numpy as np
import pytest

from oracle import postprocess_ref as P
from oracle import fixtures as Fx
from oracle import ref_goldens as G


@pytest.mark.parametrize('seed,n,noise', [(11, 2, 0.0), (12, 7, 0.02), (13, 10, 0.03)])
def test_postprocess_matches_verbatim_reference(seed, n, noise):
    heat, paf, _ = Fx.synthetic_maps(seed, n, 46, 46, 1.0, 0.9, noise=noise, height_range=(0.3, 0.7), drop_prob=0.15)
    up_h = P.resize_images_ref(heat, 320, 320)
    up_p = P.resize_images_ref(paf, 320, 320)
    arr, _ = G.load()
    ref = {'all_peaks': arr['pp%d_all_peaks' % seed], 'connections': [arr['pp%d_conn%02d' % (seed, l)] for l in range(19)],
           'poses': arr['pp%d_poses' % seed], 'scores': arr['pp%d_scores' % seed]}
    mine = P.postprocess(up_h, up_p, 320, orig_w=640, orig_h=480)
    assert np.array_equal(ref['all_peaks'], mine['all_peaks'])
    for a, b in zip(ref['connections'], mine['connections']):
        assert a.shape == np.asarray(b).reshape(-1, 3).shape
        if len(a):
            assert np.array_equal(a[:, :2], b[:, :2]) and np.allclose(a[:, 2], b[:, 2], rtol=0, atol=1e-12)
    assert np.array_equal(np.asarray(ref['poses']), np.asarray(mine['poses']))
    assert np.allclose(ref['scores'], mine['scores'], rtol=0, atol=1e-12)


def test_label_renderer_matches_reference_generator():
    arr, _ = G.load()
    heat, paf, poses = Fx.synthetic_maps(5, 4, 40, 52, 1.2, 1.0)
    assert np.array_equal(heat, arr['gen_heat'])
    assert np.array_equal(paf, arr['gen_paf'])


def test_host_helpers_match_reference():
    arr, js = G.load()
    sizes = iter(js['optimal_sizes'])
    rng = np.random.default_rng(0)
    for _ in range(50):
        h, w = int(rng.integers(20, 2000)), int(rng.integers(20, 2000))
        for t in (368, 320):
            rh_, rw_, rt, rw, rh = next(sizes)
            assert (rh_, rw_, rt) == (h, w, t)
            assert (int(rw), int(rh)) == P.compute_optimal_size(h, w, t)
    img = rng.integers(0, 256, (9, 13, 3), dtype=np.uint8)
    assert np.array_equal(arr['preprocess'], P.preprocess(img))


def test_demo_chain_helpers_match_reference():
    """get_unit_length / crop_face / crop_hands (pose_detector.py:267-424) of the product class vs the verbatim reference
    on random poses.  The reference raises ValueError when a crop box lies entirely outside the image (negative slice
    sizes at :423); the mirror returns the all-zero crop there -- those cases are skipped."""
    from conftest import pkg
    _, js = G.load()
    rows = js['demo_chain']
    assert len(rows) == 300
    PD = pkg('pose_detector')
    mine = PD.PoseDetector.__new__(PD.PoseDetector)
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (200, 300, 3), dtype=np.uint8)
    compared = 0
    for row in rows:
        pose = np.zeros((18, 3))
        pose[:, :2] = rng.uniform(-20, 320, (18, 2))
        pose[:, 2] = (rng.random(18) > 0.3) * 2
        ul_r, ul_m = row['unit_length'], mine.get_unit_length(pose.copy())
        assert ul_r == ul_m or (ul_r is None and np.isnan(ul_m))
        u = ul_r if ul_r is not None and np.isfinite(ul_r) and ul_r > 1 else 20.0
        if row.get('raised'):
            continue
        fr, hr = row['face'], row['hands']
        fm = mine.crop_face(img, pose.copy(), u)
        hm = mine.crop_hands(img, pose.copy(), 25.0)
        assert fr[1] == G.plain(fm[1]) and ((fr[0] is None and fm[0] is None) or (fm[0] is not None and fr[0] == G.digest(fm[0])))
        for side in ('left', 'right'):
            assert (hr[side] is None) == (hm[side] is None)
            if hr[side] is not None:
                assert hr[side]['bbox'] == G.plain(hm[side]['bbox']) and hr[side]['img'] == G.digest(hm[side]['img'])
        compared += 1
    assert compared > 100


def test_crop_person_and_rect_crop_face_match_reference():
    """PoseDetector.crop_person (pose_detector.py:311-352) and face_detector.crop_face(img, rect) (:99-114) vs the verbatim
    reference.  The reference's crop_person uses `sys.maxsize` without importing sys (NameError as shipped): the module got
    `sys` injected for the recording so that its logic can be compared."""
    from conftest import pkg
    _, js = G.load()
    PD, FH = pkg('pose_detector'), pkg('face_hand_detector')
    mine = PD.PoseDetector.__new__(PD.PoseDetector)
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (240, 320, 3), dtype=np.uint8)
    compared = 0
    assert len(js['crop_person']) == 400 and len(js['rect_crop_face']) == 200
    for r in js['crop_person']:
        pose = np.zeros((18, 3))
        pose[:, :2] = rng.uniform(5, 300, (18, 2))
        pose[:, 2] = (rng.random(18) > rng.choice([0.2, 0.6, 0.9])) * 2
        u = np.float64(rng.uniform(5, 40))
        if r is None:
            continue          # fewer than two usable joints / box outside the image: the reference fails in its own ways
        g = mine.crop_person(img, pose.copy(), u)
        assert tuple(r['bbox']) == tuple(g[1]) and r['img'] == G.digest(g[0])
        compared += 1
    assert compared > 200
    for a in js['rect_crop_face']:
        rect = (int(rng.integers(0, 300)), int(rng.integers(0, 220)), int(rng.integers(4, 120)), int(rng.integers(4, 120)))
        if a is None:
            continue
        b = FH.crop_face(img, rect)
        assert a['bbox'] == G.plain(b[1]) and a['img'] == G.digest(b[0])
    # constants of the face / hand drawing helpers
    ent, ref_ent = pkg('entity'), js['entity']
    for k in ('face_crop_scale', 'fingers_indices'):
        assert G.plain(ent.params[k]) == ref_ent[k]
    assert [list(map(int, v)) for v in ent.params['face_line_indices']] == [list(map(int, v)) for v in ref_ent['face_line_indices']]
    assert [int(v) for v in ent.params['coco_joint_indices']] == [int(v) for v in ref_ent['coco_joint_indices']]
