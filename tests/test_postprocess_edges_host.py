"""CPU: the oracle on the post-process edge cases (tests/postprocess_edge_cases.py).  Two things are shown here so that the device
tests (tests/test_gpu_postprocess_edges.py), which compare with the oracle alone, mean something:

  * the NumPy oracle equals what the VERBATIM reference returned on every case (tests/golden/ref_pp_edges.npz, recorded by
    oracle/ref_edge_goldens.py): peaks, connection ids, poses bit for bit, scores within 1e-9, key points exactly;
  * every case does what it was built for (a planted value changes the result, a threshold sits between two cases, a tile really takes
    the un-patched branch): conditions on the oracle alone.

Two observations differ from what the cases were first expected to do; both are what the reference itself returns, and are asserted:
  * +inf at low-resolution pixel (0, 0) of every joint channel leaves all 89 peaks of the base in place (no blob lies within a filter
    radius of that corner), so the case `heat_pinf_blob` plants +inf two pixels from the strongest neck blob as well: that one goes;
  * under sigma 2.5 a spike at (y 63, x 64) of a 65 x 65 map gives its one peak at (64, 64): reflected at the border, the smoothed row 64
    (taps g1 + g2) exceeds row 63 (g0 + g3).  All other listed pixels keep their peak where the spike is.
"""
import warnings

import numpy as np
import pytest

import postprocess_edge_cases as E
from oracle import face_hand_ref as FH
from oracle import postprocess_ref as P
from oracle import ref_edge_goldens as G

SCORE_TOL = 1e-9
CASES = E.recorded_cases()
_memo = {}


def oracle(name):
    if name not in _memo:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')               # 0 x inf, inf - inf: the planted values
            _memo[name] = E.oracle(CASES[name])
    return _memo[name]


def close(a, b):
    """within SCORE_TOL; equal infinities count as equal (np.isclose), NaN equals nothing"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all(np.isclose(a, b, rtol=0, atol=SCORE_TOL)))


@pytest.mark.parametrize('name', sorted(CASES))
def test_oracle_equals_recorded_reference(name):
    ref, got = G.load(), oracle(name)
    assert np.array_equal(got['all_peaks'].reshape(-1, 5), ref[name + '/all_peaks']), 'peaks (type, x, y, score, id)'
    conns, rconns = G.flat_connections(got['connections']), ref[name + '/connections']
    assert conns.shape == rconns.shape and np.array_equal(conns[:, :3], rconns[:, :3]), 'connection (limb, a, b)'
    assert close(conns[:, 3], rconns[:, 3]), 'connection scores'
    assert np.array_equal(np.asarray(got['poses'], np.float64).reshape(-1, 18, 3), ref[name + '/poses']), 'poses'
    assert close(got['scores'], ref[name + '/scores']), 'person scores'


@pytest.mark.parametrize('arch,n_maps', [('handnet', 22), ('facenet', 71)])
@pytest.mark.parametrize('size', E.KP_SIZES)
@pytest.mark.parametrize('flip', [0, 1])
def test_keypoint_oracle_equals_recorded_reference(arch, n_maps, size, flip):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        up = P.resize_images_ref(E.keypoint_maps(n_maps), size[0], size[1])
        if flip:
            up = np.ascontiguousarray(up[:, :, ::-1])
        got = G.keypoint_rows(FH.compute_keypoints(up, E.KP_THRESH))
    ref = G.load()[G.kp_key(arch, size, flip)]
    assert got.shape == ref.shape == (n_maps - 1, 4)
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:5]
    # what the channels were built for: the plain spike is a key point, one NaN anywhere or a NaN channel gives None, so does the small spike
    valid = dict(zip(E.KP_CHANNELS, ref[:6, 3]))
    assert valid['spike'] == 1 and valid['spike_nan'] == 0 and valid['all_nan'] == 0 and valid['below'] == 0
    if size == (70, 50):
        assert valid['spike_ninf'] == 1 and np.array_equal(ref[3], ref[0]), '-inf far from the spike changes nothing'
        assert valid['spike_pinf'] == 1 and ref[2, 2] == np.inf
    else:                                             # (at in == out the zero weight next to the infinity gives a NaN: None)
        assert valid['spike_pinf'] == 0 and valid['spike_ninf'] == 0
    assert not ref[6:, 3].any()


# ---- 1. non-finite maps -------------------------------------------------------------------------------------------------------------
def test_nonfinite_cases_are_not_vacuous():
    clean = oracle('nf_clean')
    assert len(clean['all_peaks']) == 89 and len(clean['subsets']) == 5
    for n in E.NONFINITE_HEAT_SINGLE:
        r = oracle('nf_' + n)
        same = r['all_peaks'].shape == clean['all_peaks'].shape and np.array_equal(r['all_peaks'], clean['all_peaks'])
        assert not same, n
        assert len(r['all_peaks']) >= 50 and len(r['subsets']) >= 1, n
    assert np.array_equal(oracle('nf_heat_pinf')['all_peaks'], clean['all_peaks'])        # (module docstring)
    assert len(oracle('nf_heat_nan')['all_peaks']) == 88 and len(oracle('nf_heat_pinf_blob')['all_peaks']) == 87
    chan = oracle('nf_heat_chan_nan')['all_peaks']
    assert not (chan[:, 0] == E.NF_JOINT).any() and len(chan) == 89 - int((clean['all_peaks'][:, 0] == E.NF_JOINT).sum())
    r = oracle('nf_all_nan')
    assert len(r['all_peaks']) == 0 and len(r['subsets']) == 0
    inf_scores = [n for n in E.NONFINITE_PAF if np.isinf(oracle('nf_' + n)['scores']).any()]
    both = [n for n in inf_scores if np.isfinite(oracle('nf_' + n)['scores']).any()]
    assert 'paf_pinf' in inf_scores and 'paf_ninf' in inf_scores and both, (inf_scores, both)
    assert not any(np.isnan(oracle('nf_' + n)['scores']).any() for n in E.NONFINITE)
    # what the device's candidate store has to hold: more than 4 and at most 16 accepted pairs per limb, infinite scores among them
    for n in ('paf_pinf', 'paf_ninf'):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            most, n_inf = E.candidate_counts(CASES['nf_' + n], E.oracle(CASES['nf_' + n], with_maps=True))
        assert 4 < most <= 16 and n_inf >= 10, (n, most, n_inf)
    # the two in == out cases: the zero bilinear weight next to the infinity gives NaN in the resized maps
    for n, key in (('same_heat_pinf', 'heat'), ('same_paf_pinf', 'paf')):
        c = CASES['nf_' + n]
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            up = P.resize_images_ref(c[key], c['map_h'], c['map_w'])
        assert np.isnan(up).any() and np.isinf(up).any() and not np.isnan(c[key]).any(), n
        assert len(oracle('nf_' + n)['all_peaks']) >= 1


# ---- 3. lattice cases at radius 0 ---------------------------------------------------------------------------------------------------
def test_identity_filter_and_resize():
    a = np.random.default_rng(0).standard_normal((3, 65, 65)).astype(np.float32)
    assert len(P.gaussian_kernel1d(0.1)) == 1
    assert np.array_equal(P.gaussian_filter_ref(a[0], 0.1), a[0])
    assert np.array_equal(P.resize_images_ref(a, 65, 65), a)


def _peaks_of(r, joint):
    p = r['all_peaks']
    return [(int(y), int(x)) for _, x, y, _, _ in p[p[:, 0] == joint]]


def test_lattice_peaks_are_as_listed():
    r = oracle('lat_lattice_peaks')
    assert _peaks_of(r, 0) == [] and _peaks_of(r, 1) == [(20, 20)]                    # the float32 threshold
    assert r['all_peaks'][r['all_peaks'][:, 0] == 1][0, 3] == float(np.nextafter(E.T, np.float32(1)))
    assert _peaks_of(r, 2) == [] and _peaks_of(r, 3) == [(20, 20), (21, 21)] and _peaks_of(r, 4) == []
    for i, yx in enumerate(E.SPIKES):
        assert _peaks_of(r, 5 + i) == [yx], (i, yx)
    assert len(r['all_peaks']) == 3 + len(E.SPIKES)


def test_border_spikes_under_the_real_filter():
    r = oracle('lat_border_spikes_s2.5')
    for i, yx in enumerate(E.SPIKES):
        want = (64, 64) if yx == (63, 64) else yx                                     # (module docstring)
        assert _peaks_of(r, 5 + i) == [want], (i, yx, _peaks_of(r, 5 + i))
    assert len(r['all_peaks']) == len(E.SPIKES)


def _limb0(r):
    return np.asarray(r['connections'][0], np.float64).reshape(-1, 3)


def test_limb_thresholds_are_as_listed():
    c = _limb0(oracle('lat_limb_at_thresh'))
    assert c.shape == (1, 3) and c[0, 2] == 0.05000000074505806                       # the float64 comparison of pose_detector.py:155
    assert _limb0(oracle('lat_limb_below_thresh')).shape == (0, 3)
    c = _limb0(oracle('lat_limb_9_of_10'))
    assert c.shape == (1, 3) and c[0, 2] == 0.9
    assert _limb0(oracle('lat_limb_8_of_10')).shape == (0, 3)                          # n_valid > 8
    for n in ('limb_at_thresh', 'limb_below_thresh', 'limb_9_of_10', 'limb_8_of_10'):
        assert len(oracle('lat_' + n)['all_peaks']) == 2


def test_zero_length_pair_and_person_size():
    r = oracle('lat_zero_length')
    p = r['all_peaks']
    assert len(p) == 3 and [tuple(v) for v in p[:, :3]] == [(1, 10, 40), (8, 10, 40), (8, 19, 40)]
    c = _limb0(r)
    assert c.shape == (1, 3) and tuple(c[0, :2]) == (0, 2)                            # to the SECOND joint-8 peak, not the one underneath
    r = oracle('lat_person_size')
    assert len(r['all_peaks']) == 5 and len(_limb0(r)) == 2 and len(r['connections'][1]) == 1
    assert len(r['subsets']) == 1 and r['subsets'][0, 19] == 3                        # the two-part subset is dropped
    assert (np.asarray(r['poses'])[0][:, 2] == 2).sum() == 3


# ---- 4. other radii, tiny maps, down-sampling ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('sigma', [1.0, 2.5, 4.0])
@pytest.mark.parametrize('hw', [(97, 121), (5, 7), (3, 3), (1, 40), (40, 1), (1, 1)])
def test_filter_equals_scipy_at_other_radii_and_narrow_maps(sigma, hw):
    """Maps narrower than the radius reflect more than once; SciPy is the reference's filter."""
    ndi = pytest.importorskip('scipy.ndimage')
    a = (np.random.default_rng(hw[0] * 100 + hw[1]).random(hw) * 3).astype(np.float32)
    assert np.array_equal(P.gaussian_filter_ref(a, sigma), ndi.gaussian_filter(a, sigma=sigma))


def test_radius_cases_have_peaks_and_people():
    assert [len(P.gaussian_kernel1d(s)) // 2 for s in E.SIGMAS] == [0, 4, 16]
    assert len(P.gaussian_kernel1d(4.2)) // 2 == 17
    for s in E.SIGMAS:
        r = oracle('radius_s%g' % s)
        assert len(r['all_peaks']) >= 20, (s, len(r['all_peaks']))
    assert len(oracle('radius_s1')['subsets']) >= 1


@pytest.mark.parametrize('sigma', E.NARROW_SIGMAS)
@pytest.mark.parametrize('hw', E.NARROW)
def test_narrow_maps_have_peaks(hw, sigma):
    r = oracle('narrow_%dx%d_%dx%d_s%g' % (hw + (sigma,)))
    if hw[:2] != (1, 1):
        assert len(r['all_peaks']) >= 1
    assert min(hw[2:]) < int(4 * sigma + 0.5) or hw == (5, 7, 23, 31)


@pytest.mark.parametrize('hw', E.DOWN)
def test_down_sampled_tiles_take_the_unpatched_branch(hw):
    """A 54-pixel tile (32 + 2 + 2 x 10, reflected at the borders) of the fast peak kernel stages its low-resolution patch in LDS only
    if the patch fits 56 x 56; here the first tile's span exceeds 56 on the intended axes and fits on the other."""
    h, w, map_h, map_w = hw

    def span(n_in, n_out):
        i0, i1, _, _ = P.resize_grid(n_in, n_out)
        idx = np.arange(-11, 43)                          # tile 0: pixels -1 - R .. 32 + R
        idx = np.where(idx < 0, -idx - 1, idx)            # 'reflect'
        idx = np.where(idx >= n_out, 2 * n_out - 1 - idx, idx)
        return int(i1[idx].max() - i0[idx].min() + 1)
    assert (span(h, map_h) > 56) == (h > map_h) and (span(w, map_w) > 56) == (w > map_w), (span(h, map_h), span(w, map_w))
    assert h > map_h or w > map_w
    r = oracle('down_%dx%d_%dx%d' % hw)
    assert len(r['all_peaks']) >= 10 and len(r['subsets']) >= 1
