"""GPU: the HIP post-process at its edges against the NumPy oracle (pinned to the verbatim reference on exactly these inputs by
tests/test_postprocess_edges_host.py): non-finite maps through the pose path and the key-point arg-max, exact ties and thresholds at
radius 0, Gaussian radii 0 / 4 / 16, maps narrower than the radius, down-sampling (the un-patched tile of the fast peak kernel).

Contract (include/pose_mi355x.h): peaks, connection ids, subset ids, poses and smoothed maps bit-equal (NaN at the same places), scores
within 1e-9 with equal infinities equal, status 0; a key-point channel holding a NaN gives no key point and a NaN confidence.
"""
import warnings

import numpy as np
import pytest

import postprocess_edge_cases as E
from conftest import conns_by_limb, pkg
from oracle import face_hand_ref as FH
from oracle import postprocess_ref as P

pytestmark = pytest.mark.gpu
SCORE_TOL = 1e-9
_memo = {}


def oracle(key, c):
    """the oracle's answer for a pose case, computed once per module run and left unchanged"""
    if key not in _memo:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')               # 0 x inf, inf - inf: the planted values
            _memo[key] = E.oracle(c, with_maps=True)
    return _memo[key]


def close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all(np.isclose(a, b, rtol=0, atol=SCORE_TOL)))


def same_bits(a, b):
    """bit-equal where finite or infinite, NaN exactly where the oracle has NaN"""
    nan = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), nan) and np.array_equal(a[~nan], b[~nan])


def check(e, image, ref, rec, what):
    peaks = e.peaks(image)
    rp = ref['all_peaks'].reshape(-1, 5)
    assert peaks.shape == rp.shape, (what, 'peak count', peaks.shape, rp.shape)
    assert np.array_equal(peaks, rp), (what, 'peaks (type, x, y, score, id)', np.argwhere(peaks != rp)[:5])
    conns = conns_by_limb(e.connections(image))
    for l in range(19):
        r = np.asarray(ref['connections'][l], np.float64).reshape(-1, 3)
        assert conns[l].shape == r.shape, (what, 'limb %d' % l, conns[l], r)
        assert np.array_equal(conns[l][:, :2], r[:, :2]), (what, 'limb %d ids' % l)
        assert close(conns[l][:, 2], r[:, 2]), (what, 'limb %d scores' % l, conns[l][:, 2], r[:, 2])
    subsets = e.subsets(image)
    rs = ref['subsets']
    assert subsets.shape == rs.shape, (what, 'subsets', subsets.shape, rs.shape)
    assert np.array_equal(subsets[:, :18], rs[:, :18]), (what, 'subset ids')
    assert close(subsets[:, 18:], rs[:, 18:]), (what, 'subset score / count', subsets[:, 18:], rs[:, 18:])
    n = int(rec['n_people'])
    assert rec['status'] == 0, (what, int(rec['status']))
    assert n == len(rs) and rec['n_peaks'] == len(rp), (what, n, len(rs))
    if n:
        assert np.array_equal(rec['poses'][:n], np.asarray(ref['poses'], np.float64)), (what, 'poses')
        assert close(rec['scores'][:n], ref['scores']), (what, 'person scores', rec['scores'][:n], ref['scores'])


def run(e, c, key, what, generic=0, keep=0, slices=-1, batch=None):
    """one case through one form of the post-process; options are put back whatever happens"""
    ref = oracle(key, c)
    try:
        e.set_option('pp_generic', generic)
        e.set_option('keep_smoothed', keep)
        e.set_option('pp_limbs_slices', slices)
        paf, heat = (c['paf'][None], c['heat'][None]) if batch is None else batch
        e.set_maps(paf, heat)
        e.postprocess(c['map_h'], c['map_w'], img_len=c['map_w'])
        if keep:
            for j in range(18):
                sm = e.smoothed(0, j)
                assert same_bits(sm, ref['smoothed'][j]), (what, 'smoothed channel %d' % j)
        rec = e.results()[0]
        check(e, 0, ref, rec, what)
    finally:
        e.set_option('pp_generic', 0)
        e.set_option('keep_smoothed', 0)
        e.set_option('pp_limbs_slices', -1)
    return ref


@pytest.fixture(scope='module')
def engines(native):
    """one fresh context per Gaussian sigma, made on first use"""
    made = {}

    def get(sigma):
        if sigma not in made:
            made[sigma] = native.Engine(0, max_batch=2, max_h=368, max_w=368, gaussian_sigma=sigma)
        return made[sigma]
    yield get
    for e in made.values():
        e.close()


# ---- 1. non-finite maps through the pose post-process -------------------------------------------------------------------------------
FORMS = [dict(generic=0, keep=0), dict(generic=1, keep=0), dict(generic=0, keep=1), dict(generic=1, keep=1),
         dict(slices=0), dict(slices=3), dict(slices=8)]


@pytest.mark.parametrize('name', E.NONFINITE)
def test_nonfinite_maps_every_form(engines, name):
    """Both peak kernels, with the pruning exit (keep_smoothed 0) and with the smoothed channels compared (1; the planted channel
    included), and the candidate scan in one block, three and eight slices."""
    c = E.nonfinite_case(name)
    for form in FORMS:
        run(engines(2.5), c, 'nf_' + name, (name, form), **form)


@pytest.mark.parametrize('candidates', [16, 4])
@pytest.mark.parametrize('name', ['clean', 'paf_pinf', 'paf_ninf', 'same_paf_pinf'])
def test_nonfinite_scores_in_the_device_memory_candidate_store(native, name, candidates):
    """A context whose candidate store lies in device memory: 16 entries hold the at most 12 accepted pairs of a limb of these maps,
    the infinite scores among them (the host test counts them); 4 entries do not, so the growth loop runs on infinite scores too."""
    c = E.nonfinite_case(name)
    most, _ = E.candidate_counts(c, oracle('nf_' + name, c))
    for slices in (-1, 0):
        e = native.Engine(0, max_batch=2, max_h=368, max_w=368)
        e.set_capacities(candidates=candidates)
        try:
            run(e, c, 'nf_' + name, (name, candidates, slices), slices=slices)
            assert e.capacities()['candidates'] >= max(most, candidates)
        finally:
            e.close()


def test_nonfinite_maps_grow_tiny_capacities(native):
    e = native.Engine(0, max_batch=2, max_h=368, max_w=368)
    e.set_capacities(peaks_per_joint=4, subsets=2, people=1)
    try:
        ref = run(e, E.nonfinite_case('paf_pinf'), 'nf_paf_pinf', 'tiny capacities')
        caps = e.capacities()
        assert caps['peaks_per_joint'] > 4 and caps['subsets'] > 2 and caps['people'] >= len(ref['subsets']) > 1
    finally:
        e.close()


def _image_bytes(e, i, rec):
    n = int(rec['n_people'])
    head = [int(rec[k]) for k in ('n_people', 'n_peaks', 'status', 'n_subsets_raw')]
    return (e.peaks(i).tobytes(), e.connections(i).tobytes(), e.subsets(i).tobytes(), head, rec['scores'][:n].tobytes(),
            rec['poses'][:n].tobytes())


@pytest.mark.parametrize('name', ['paf_pinf', 'heat_chan_nan', 'all_nan'])
def test_a_planted_image_leaves_its_neighbour_alone(engines, name):
    e = engines(2.5)
    clean, planted = E.nonfinite_case('clean'), E.nonfinite_case(name)
    e.set_maps(clean['paf'][None], clean['heat'][None])
    e.postprocess(120, 120, img_len=120)
    alone = _image_bytes(e, 0, e.results()[0])
    e.set_maps(np.stack([planted['paf'], clean['paf']]), np.stack([planted['heat'], clean['heat']]))
    e.postprocess(120, 120, img_len=120)
    recs = e.results()
    assert _image_bytes(e, 1, recs[1]) == alone
    check(e, 0, oracle('nf_' + name, planted), recs[0], name)
    check(e, 1, oracle('nf_clean', clean), recs[1], 'clean beside ' + name)


def test_nan_bias_in_the_last_stage_on_the_product_path(native):
    """detect_batch on a 64 x 64 image (the NHWC maps of the forward): one NaN bias of the last heat layer makes that joint's map NaN
    (forward contract); that joint type then has no peaks, the other types keep theirs, and everything equals the oracle on get_maps()."""
    W = pkg('weights')
    raw = W.synthetic_weights(3)
    img = np.random.default_rng(5).integers(0, 256, (1, 64, 64, 3), dtype=np.uint8)
    e = native.Engine(0, max_batch=1, max_h=64, max_w=64)
    try:
        e.set_weights(raw)
        e.forward_u8(img)
        paf, heat = e.get_maps()
        good = W.calibrate_head(raw, paf[0], heat[0], heat_s=0.3, heat_t=0.0, paf_s=1.2)      # as tests/test_gpu_pp_tables.py
        e.set_weights(good)
        e.detect_batch(img, map_h=64, map_w=64)
        clean = e.peaks(0)
        assert e.results()[0]['status'] == 0 and len(clean) >= 2
        joint = int(clean[0, 0])
        Wl, b = good['Mconv7_stage6_L2']
        b = np.array(b, np.float32)
        b[joint] = np.nan
        e.set_layer('Mconv7_stage6_L2', Wl, b)
        e.detect_batch(img, map_h=64, map_w=64)
        rec = e.results()[0]
        paf, heat = e.get_maps()
        assert np.isnan(heat[0, joint]).all() and not np.isnan(np.delete(heat[0], joint, 0)).any() and not np.isnan(paf).any()
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            ref = P.postprocess_from_net_output(paf[0], heat[0], 64, 64)
        check(e, 0, ref, rec, 'NaN bias, joint %d' % joint)
        got = e.peaks(0)
        assert not (got[:, 0] == joint).any()
        assert np.array_equal(got[:, :4], clean[clean[:, 0] != joint][:, :4])
    finally:
        e.close()


# ---- 2. non-finite maps through the key-point arg-max -------------------------------------------------------------------------------
N_MAPS = {'handnet': 22, 'facenet': 71}


def kp_oracle(maps, size, flip):
    """(channels, 4) rows (x, y, confidence, valid) of the oracle; the confidence is the smoothed maximum (`max_value`) also where the
    reference appends None, which is what the library writes there"""
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        up = P.resize_images_ref(maps, size[0], size[1])
        if flip:
            up = np.ascontiguousarray(up[:, :, ::-1])         # hand_detector.py:46-47
        kps = FH.compute_keypoints(up, E.KP_THRESH)
        rows = np.zeros((len(kps), 4))
        for i, k in enumerate(kps):
            rows[i] = [0, 0, P.gaussian_filter_ref(up[i]).max() if i < 6 else 0.0, 0] if k is None else [k[0], k[1], k[2], 1]
    return rows


def kp_check(got, ref, what):
    assert got.shape == ref.shape
    for ch in range(len(ref)):
        name = (what, E.KP_CHANNELS[ch] if ch < 6 else ch, got[ch], ref[ch])
        assert got[ch, 3] == ref[ch, 3], ('None-ness',) + name
        if ref[ch, 3]:
            assert got[ch, 0] == ref[ch, 0] and got[ch, 1] == ref[ch, 1], ('x, y',) + name
        if np.isnan(ref[ch, 2]):
            assert np.isnan(got[ch, 2]), ('confidence',) + name
        else:
            assert got[ch, 2] == ref[ch, 2], ('confidence',) + name


@pytest.fixture(scope='module')
def kp_engines(native):
    made = {arch: native.Engine(0, max_batch=2, max_h=368, max_w=368, arch=arch) for arch in N_MAPS}
    yield made
    for e in made.values():
        e.close()


@pytest.mark.parametrize('arch', sorted(N_MAPS))
@pytest.mark.parametrize('size', E.KP_SIZES)
@pytest.mark.parametrize('generic', [0, 1])
@pytest.mark.parametrize('flip', [0, 1])
def test_keypoints_on_nonfinite_maps(kp_engines, arch, size, generic, flip):
    e = kp_engines[arch]
    maps = E.keypoint_maps(N_MAPS[arch])
    ref = kp_oracle(maps, size, flip)
    try:
        e.set_option('pp_generic', generic)
        e.set_option('kp_flip_x', flip)
        e.set_heat(maps[None])
        got = e.keypoints(size[0], size[1], E.KP_THRESH)[0]
    finally:
        e.set_option('pp_generic', 0)
        e.set_option('kp_flip_x', 0)
    kp_check(got, ref, (arch, size, generic, flip))


@pytest.mark.parametrize('arch', sorted(N_MAPS))
def test_keypoints_images_on_nonfinite_maps(kp_engines, arch):
    """Per-tile records merged by kp_merge_kernel: the 70 x 50 crop has 3 x 2 tiles, the NaN sits in another tile than the spike."""
    e = kp_engines[arch]
    maps = E.keypoint_maps(N_MAPS[arch])
    e.set_heat(np.stack([maps, maps]))
    got = e.keypoints_images([(70, 50, 0), (70, 50, 1)], E.KP_THRESH)
    for i, flip in enumerate((0, 1)):
        kp_check(got[i], kp_oracle(maps, (70, 50), flip), (arch, 'keypoints_images', flip))
    e.set_heat(maps[None])
    got = e.keypoints_images([(40, 40, 0)], E.KP_THRESH)
    kp_check(got[0], kp_oracle(maps, (40, 40), 0), (arch, 'keypoints_images', '40 x 40'))


@pytest.mark.parametrize('hand_type', ['right', 'left'])
def test_hand_detector_on_nonfinite_maps(native, hand_type):
    D = pkg('face_hand_detector')
    maps = E.keypoint_maps(22)
    det = D.HandDetector('handnet', model=lambda x: [maps[None]], device=0)
    try:
        img = np.zeros((70, 50, 3), np.uint8)
        got = det(img, hand_type=hand_type)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            ref, _ = FH.detect(lambda x: maps[None], img, E.KP_THRESH, hand_type=hand_type)
        assert len(got) == len(ref) == 21
        for ch, (g, r) in enumerate(zip(got, ref)):
            assert (g is None) == (r is None), (ch, g, r)
            if r is not None:
                assert g[0] == r[0] and g[1] == r[1] and g[2] == r[2], (ch, g, r)
        assert ref[0] is not None and ref[1] is None and ref[2] is not None and ref[4] is None
    finally:
        det.engine.close()


@pytest.mark.parametrize('hw', [(9, 1), (1, 9)])
def test_keypoints_equal_the_oracle_on_one_pixel_axes(native, hw):
    """The crops of tests/test_gpu_pp_tables.py (there: the two entries against each other), here against the oracle: a one-pixel axis
    is the num == 1 branch of the resize grid and reflects ten times under the radius-10 filter."""
    FHW = pkg('weights')
    h, w = hw
    e = native.Engine(0, max_batch=1, max_h=64, max_w=64, arch='handnet')
    try:
        e.set_weights(FHW.synthetic_weights(9, 'handnet'))
        img = np.random.default_rng(13).integers(0, 256, (40, 50, 3), dtype=np.uint8)
        for flip in (0, 1):
            e.forward_u8_boxes(img, [(7, 5, 7 + w, 5 + h, flip)])
            heat = e.get_maps()[0]
            e.set_option('kp_flip_x', flip)
            got = e.keypoints(h, w, -1e30)[0]
            up = P.resize_images_ref(heat, h, w)
            ref = FH.compute_keypoints(np.ascontiguousarray(up[:, :, ::-1]) if flip else up, -1e30)
            assert got[:, 3].all() and all(r is not None for r in ref)
            want = np.array([[r[0], r[1], r[2], 1] for r in ref], np.float64)
            assert np.array_equal(got, want), (hw, flip, np.argwhere(got != want)[:5])
    finally:
        e.close()


# ---- 3. lattice cases at radius 0 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('slices', [0, 8])
@pytest.mark.parametrize('name', E.LATTICE_CASES)
def test_lattice_cases_at_radius_0(engines, name, slices):
    """sigma 0.1: the filter is the identity, and so is the resize at in == out, so the planted float32 values reach the NMS and the
    limb scoring unchanged (what each case must give is asserted on the oracle in tests/test_postprocess_edges_host.py)."""
    run(engines(0.1), E.lattice_case(name), 'lat_' + name, (name, slices), slices=slices)


@pytest.mark.parametrize('generic', [0, 1])
def test_border_and_seam_spikes_under_the_real_filter(engines, generic):
    run(engines(2.5), E.lattice_case('border_spikes', 2.5), 'lat_border_spikes_s2.5', ('border_spikes', generic), generic=generic, keep=1)


# ---- 4. other radii, tiny maps, down-sampling ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('sigma', E.SIGMAS)
def test_other_gaussian_radii(engines, sigma):
    """radius 0, 4 and 16 on maps that are no multiple of the 32-pixel tile: the generic peak kernel at the radii it is never run at"""
    for keep in (1, 0):
        run(engines(sigma), E.radius_case(sigma), 'radius_s%g' % sigma, (sigma, keep), keep=keep)


def test_radius_17_is_refused(native):
    with pytest.raises(native.PmxError) as err:
        native.Engine(0, max_batch=1, max_h=64, max_w=64, gaussian_sigma=4.2)
    assert err.value.code == 1                            # PMX_ERR_INVALID


@pytest.mark.parametrize('sigma,generic', [(2.5, 0), (2.5, 1), (4.0, 0)])
@pytest.mark.parametrize('hw', E.NARROW)
def test_maps_narrower_than_the_radius(engines, hw, sigma, generic):
    key = 'narrow_%dx%d_%dx%d_s%g' % (hw + (sigma,))
    for keep in (1, 0):
        run(engines(sigma), E.narrow_case(hw, sigma), key, (hw, sigma, generic, keep), generic=generic, keep=keep)


@pytest.mark.parametrize('generic', [0, 1])
@pytest.mark.parametrize('hw', E.DOWN)
def test_down_sampled_maps(engines, hw, generic):
    """maps smaller than the network output: the fast kernel's tile reads the map itself instead of an LDS patch, on both axes, on rows
    only and on columns only"""
    for keep in (1, 0):
        run(engines(2.5), E.down_case(hw), 'down_%dx%d_%dx%d' % hw, (hw, generic, keep), generic=generic, keep=keep)
