"""The case table of the post-process edge tests (tests/test_postprocess_edges_host.py on the CPU, tests/test_gpu_postprocess_edges.py on
the device, oracle/ref_edge_goldens.py for the recording of the verbatim reference's answers): non-finite maps, exact ties and
thresholds at radius 0, other Gaussian radii, maps narrower than the radius, down-sampling.  Pure NumPy: every input is regenerated
from this table, only the reference's answers are stored (tests/golden/ref_pp_edges.npz).

A pose case is a dict {sigma, paf, heat, map_h, map_w}: low-resolution maps (38 | 19, h, w) float32, post-processed at map_h x map_w
with img_len = map_w.  A key-point case is {maps (n_maps, 40, 40), out_h, out_w}.
"""
import numpy as np

from oracle import fixtures as Fx
from oracle import postprocess_ref as P

NAN, INF = np.float32(np.nan), np.float32(np.inf)
T = np.float32(0.05)                                  # heatmap_peak_thresh and inner-product threshold as float32
LATTICE = 65                                          # radius-0 cases: map == maps == 65 x 65 (two tile seams, three tiles per axis)
SPIKES = [(0, 0), (0, 64), (64, 0), (64, 64), (31, 31), (32, 32), (31, 32), (0, 32), (32, 0), (63, 64)]     # (y, x), channel 5 + i


def case(sigma, paf, heat, map_h, map_w):
    return dict(sigma=sigma, paf=np.ascontiguousarray(paf, np.float32), heat=np.ascontiguousarray(heat, np.float32),
                map_h=int(map_h), map_w=int(map_w))


def oracle(c, with_maps=False):
    """The NumPy oracle's answer for a pose case."""
    if with_maps:
        return P.postprocess_from_net_output(c['paf'], c['heat'], c['map_h'], c['map_w'], sigma=c['sigma'])
    heat = P.resize_images_ref(c['heat'], c['map_h'], c['map_w'])
    paf = P.resize_images_ref(c['paf'], c['map_h'], c['map_w'])
    return P.postprocess(heat, paf, c['map_w'], sigma=c['sigma'])


def candidate_counts(c, ref):
    """(most accepted candidate pairs of one limb, infinite candidate scores over all limbs) of oracle(c, with_maps=True): what the
    candidate store of the device has to hold"""
    pk, most, n_inf = ref['all_peaks'], 0, 0
    for l, (ja, jb) in enumerate(P.LIMBS_POINT):
        a, b = pk[pk[:, 0] == ja][:, 1:], pk[pk[:, 0] == jb][:, 1:]
        if len(a) and len(b):
            with np.errstate(invalid='ignore'):               # inf - inf, 0 x inf: the planted values
                cands = P.compute_candidate_connections(ref['pafs'][[2 * l, 2 * l + 1]], a, b, c['map_w'])
            most = max(most, len(cands))
            n_inf += sum(bool(np.isinf(s)) for _, _, s in cands)
    return most, n_inf


# ---- 1. non-finite maps -------------------------------------------------------------------------------------------------------------
NONFINITE_HEAT_SINGLE = ['heat_nan', 'heat_pinf_blob', 'heat_ninf']        # each changes at least one peak of the clean result
NONFINITE_PAF = ['paf_nan', 'paf_pinf', 'paf_ninf', 'same_paf_pinf']
NONFINITE = ['clean', 'heat_pinf'] + NONFINITE_HEAT_SINGLE + ['paf_nan', 'paf_pinf', 'paf_ninf', 'heat_chan_nan', 'all_nan', 'same_heat_pinf',
                                                 'same_paf_pinf']
NF_JOINT = 1                                          # the heat channel that takes the planted values (neck: it starts 5 of the 19 limbs)


def _nonfinite_base():
    heat, paf, _ = Fx.synthetic_maps(2, 6, 30, 30, 1.0, 0.9, noise=0.02, height_range=(0.3, 0.7), drop_prob=0.1)
    return heat, paf


def nonfinite_case(name):
    """30 x 30 maps of six synthetic people at map 120 x 120 (`same_*`: at 30 x 30, where the resize is the identity up to 0 x inf)."""
    heat, paf = _nonfinite_base()
    heat, paf = heat.copy(), paf.copy()
    size = 30 if name.startswith('same_') else 120
    by, bx = np.unravel_index(int(np.argmax(heat[NF_JOINT])), heat[NF_JOINT].shape)      # the strongest neck blob: an interior pixel
    assert 2 <= by < 28 and 2 <= bx < 28
    if name == 'heat_nan':
        heat[NF_JOINT, by, bx] = NAN
    elif name == 'heat_pinf':
        heat[:18, 0, 0] = INF                         # low-resolution pixel (0, 0) of every joint channel
    elif name == 'same_heat_pinf':
        heat[:18, 15, 15] = INF                       # interior: the pixels left of and above it get 0 x inf = NaN from the resize
    elif name == 'heat_pinf_blob':
        heat[NF_JOINT, by + 2, bx] = INF              # two pixels from the strongest neck blob: its peak goes
    elif name == 'heat_ninf':
        heat[:18, 29, :] = -INF                       # the last row
    elif name == 'paf_nan':
        paf[:, by, bx] = NAN                          # one pixel of every channel, under a limb
    elif name in ('paf_pinf', 'same_paf_pinf'):
        paf[:, by - 2:by + 3, bx - 2:bx + 3] = INF
    elif name == 'paf_ninf':
        paf[:, by - 2:by + 3, bx - 2:bx + 3] = -INF
    elif name == 'heat_chan_nan':
        heat[NF_JOINT] = NAN
    elif name == 'all_nan':
        heat[:] = NAN
        paf[:] = NAN
    else:
        assert name == 'clean', name
    return case(2.5, paf, heat, size, size)


# ---- 2. key-point maps --------------------------------------------------------------------------------------------------------------
KP_CHANNELS = ['spike', 'spike_nan', 'spike_pinf', 'spike_ninf', 'all_nan', 'below']
KP_SIZES = [(40, 40), (70, 50)]                       # in == out; up-sampled to more than one 32 x 32 tile per axis
KP_THRESH = 0.1


def keypoint_maps(n_maps):
    """(n_maps, 40, 40): channels 0..5 as KP_CHANNELS, the rest zero.  The spike sits at (y 8, x 9), the planted value at (30, 29):
    further apart than two Gaussian radii at both sizes, so the spike's neighbourhood stays finite."""
    m = np.zeros((n_maps, 40, 40), np.float32)
    m[0:4, 8, 9] = 4.0
    m[1, 30, 29] = NAN
    m[2, 30, 29] = INF
    m[3, 30, 29] = -INF
    m[4] = NAN
    m[5, 8, 9] = 0.5
    return m


# ---- 3. lattice cases at radius 0 ---------------------------------------------------------------------------------------------------
LATTICE_CASES = ['lattice_peaks', 'limb_at_thresh', 'limb_below_thresh', 'limb_9_of_10', 'limb_8_of_10', 'zero_length', 'person_size']


def _blank():
    return np.zeros((38, LATTICE, LATTICE), np.float32), np.zeros((19, LATTICE, LATTICE), np.float32)


def lattice_case(name, sigma=0.1):
    paf, heat = _blank()
    if name == 'lattice_peaks':
        heat[0, 20, 20] = T                                       # a lone threshold value: no peak (float32 '>')
        heat[1, 20, 20] = np.nextafter(T, np.float32(1))          # one ulp above: a peak
        heat[2, 20, 20] = heat[2, 20, 21] = 0.5                   # equal horizontal neighbours: none
        heat[3, 20, 20] = heat[3, 21, 21] = 0.5                   # equal diagonal pixels: both
        heat[4, 19:22, 19:22] = 0.5                               # 3 x 3 plateau: none
        for i, (y, x) in enumerate(SPIKES):
            heat[5 + i, y, x] = 0.5
    elif name == 'border_spikes':                                 # the same pixels under a real filter (sigma 2.5: smoothed peak ~ 0.1)
        for i, (y, x) in enumerate(SPIKES):
            heat[5 + i, y, x] = 4.0
    elif name.startswith('limb_'):                                # limb 0 = joint 1 -> joint 8; the 10 samples fall on x = 10..19 of row 40
        heat[1, 40, 10] = heat[8, 40, 19] = 0.5
        if name == 'limb_at_thresh':
            paf[0, 40, 10:20] = T                                 # float64(float32(0.05)) > 0.05: accepted
        elif name == 'limb_below_thresh':
            paf[0, 40, 10:20] = np.nextafter(T, np.float32(0))
        elif name == 'limb_9_of_10':
            paf[0, 40, 10:20] = 1.0
            paf[0, 40, 14] = 0.0
        else:
            assert name == 'limb_8_of_10', name
            paf[0, 40, 10:20] = 1.0
            paf[0, 40, 14] = paf[0, 40, 17] = 0.0                 # n_valid == 8 is not '> 8'
    elif name == 'zero_length':
        heat[1, 40, 10] = heat[8, 40, 10] = heat[8, 40, 19] = 0.5
        paf[0] = 1.0
    elif name == 'person_size':
        heat[1, 20, 10] = heat[8, 20, 19] = 0.5                   # two parts: dropped
        heat[1, 40, 10] = heat[8, 40, 19] = heat[9, 40, 28] = 0.5  # three parts: kept
        paf[0] = 1.0                                              # limb 0 (1 -> 8), x component
        paf[2] = 1.0                                              # limb 1 (8 -> 9)
    else:
        raise KeyError(name)
    return case(sigma, paf, heat, LATTICE, LATTICE)


# ---- 4. other radii, tiny maps, down-sampling ---------------------------------------------------------------------------------------
SIGMAS = [0.1, 1.0, 4.0]                              # radius 0, 4 and 16 (the largest the library takes)


def radius_case(sigma):
    heat, paf, _ = Fx.synthetic_maps(4, 4, 24, 30, 1.0, 0.9, noise=0.02, height_range=(0.3, 0.7), drop_prob=0.1)
    return case(sigma, paf, heat, 97, 121)


NARROW = [(5, 7, 5, 7), (3, 3, 3, 3), (1, 40, 1, 40), (40, 1, 40, 1), (1, 1, 1, 1), (5, 7, 23, 31)]     # (h, w, map_h, map_w)
NARROW_SIGMAS = [2.5, 4.0]


def narrow_case(hw, sigma):
    h, w, map_h, map_w = hw
    rng = np.random.default_rng(1000 * h + w)
    heat = (rng.random((19, h, w)) * 3).astype(np.float32)
    paf = (rng.standard_normal((38, h, w)) * 0.8).astype(np.float32)
    return case(sigma, paf, heat, map_h, map_w)


DOWN = [(120, 120, 60, 60), (120, 40, 60, 40), (40, 120, 40, 60)]      # the un-patched tile on both axes, on rows only, on columns only


def down_case(hw):
    h, w, map_h, map_w = hw
    heat, paf, _ = Fx.synthetic_maps(6, 5, h, w, 5.0, 4.0, noise=0.02, height_range=(0.3, 0.7), drop_prob=0.1)
    return case(2.5, paf, heat, map_h, map_w)


def recorded_cases():
    """{name: pose case} of everything the verbatim reference is recorded on."""
    out = {}
    for n in NONFINITE:
        out['nf_' + n] = nonfinite_case(n)
    for n in LATTICE_CASES:
        out['lat_' + n] = lattice_case(n)
    out['lat_border_spikes_s2.5'] = lattice_case('border_spikes', 2.5)
    for s in SIGMAS:
        out['radius_s%g' % s] = radius_case(s)
    for hw in NARROW:
        for s in NARROW_SIGMAS:
            out['narrow_%dx%d_%dx%d_s%g' % (hw + (s,))] = narrow_case(hw, s)
    for hw in DOWN:
        out['down_%dx%d_%dx%d' % hw] = down_case(hw)
    return out
