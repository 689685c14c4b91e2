"""pmx_detect_batch as two half-batch chains on two streams (option "batch_chains"; csrc/pmx_api.hip: detect_batch_chains): every layer is
planned once for the whole batch and launched per half, so maps and records are the bits of the one-chain call -- whatever the split, the
order of calls, the capacities -- and what the caller enqueues behind the call sees all B records.

Shapes: 48 x 368 is the smallest input whose 1/8 map (6 x 46 = 69 Winograd tiles: two full blocks of 32 + 5) takes the run geometry with a
unit-mode tail; conv_algo 2 (with wino_tail 1) puts small batches on the Winograd forms, batch_chains 1 forces the two chains wherever the
plans allow."""
import re

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu
H, W = 48, 368


@pytest.fixture(scope='module')
def weights(native):
    Wt = pkg('weights')
    w = Wt.synthetic_weights(0)
    eng = native.Engine(0, max_batch=1, max_h=H, max_w=W)
    eng.set_weights(w)
    eng.forward_u8(np.random.default_rng(1234).integers(0, 256, (1, H, W, 3), dtype=np.uint8))
    paf, heat = eng.get_maps()
    eng.close()
    return Wt.calibrate_head(w, paf[0], heat[0])


@pytest.fixture(scope='module')
def small(native, weights):
    """batch <= 5 of 48 x 368 with every eligible layer on the Winograd forms"""
    eng = native.Engine(0, max_batch=5, max_h=H, max_w=W)
    eng.set_weights(weights)
    eng.set_option('conv_algo', 2)
    eng.set_option('wino_tail', 1)       # (under conv_algo 2 the tails run in unit mode only when asked for)
    yield eng
    eng.close()


def images(B, h=H, w=W, seed=5):
    return np.random.default_rng(seed).integers(0, 256, (B, h, w, 3), dtype=np.uint8)


def detect(eng, imgs, chains, profile=False):
    """-> (paf, heat, records, profile) of one detect_batch with batch_chains = chains"""
    eng.set_option('batch_chains', chains)
    prof = None
    if profile:
        eng.profile_reset(); eng.profile_enable(profile)      # (True / 1: every launch; 2: the 7x7 layers only)
    try:
        eng.detect_batch(imgs, imgs.shape[1], imgs.shape[2])
        rec = eng.results()
        if profile:
            prof = eng.profile()
    finally:
        if profile:
            eng.profile_enable(False); eng.profile_reset()
        eng.set_option('batch_chains', 0)
    paf, heat = eng.get_maps()
    return paf, heat, rec, prof


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2].dtype == b[2].dtype and a[2].tobytes() == b[2].tobytes()


def halves(prof):
    return sorted({m.group(0) for p in prof for m in [re.search(r'@\d+\+\d+$', p['kernel'])] if m})


@pytest.mark.parametrize('B', [2, 4, 5])
def test_two_chains_bit_identical_to_one(small, B):
    """maps and records of B = 2, 4 and 5 (2 + 3) images: two chains == one chain, bit for bit; and the two chains did run"""
    imgs = images(B, seed=B)
    one = detect(small, imgs, 0)
    two = detect(small, imgs, 1, profile=True)
    assert halves(two[3]) == sorted(['@0+%d' % (B // 2), '@%d+%d' % (B // 2, B - B // 2)]), halves(two[3])
    assert int(one[2]['n_peaks'].sum()) > 0
    assert same(one, two)


def test_two_chains_bit_identical_at_368_default_algo(native, weights):
    """four 368 x 368 frames under the default conv_algo (the forms of the batch path: merged tails of two images per half)"""
    eng = native.Engine(0, max_batch=4, max_h=368, max_w=368)
    eng.set_weights(weights)
    imgs = images(4, 368, 368, seed=9)
    one = detect(eng, imgs, 0)
    two = detect(eng, imgs, 1, profile=True)
    print('halves at 368 x 368, B = 4:', halves(two[3]))
    auto = detect(eng, imgs, -1, profile=2)
    eng.close()
    assert same(one, two) and same(one, auto)
    assert not halves(auto[3])       # 4 frames are 128 blocks per 7x7 launch: no whole rounds of the CUs, the automatic rule keeps one chain


def test_automatic_rule_takes_two_chains_at_batch_16(native, weights):
    """sixteen 368 x 368 frames under the default options: 16 full blocks x 8 images x 2 groups = 256 = one round of the CUs per half, so
    the automatic rule (the default) runs two chains of 8 -- same bits as one chain; under the per-launch profiler it keeps one chain"""
    eng = native.Engine(0, max_batch=16, max_h=368, max_w=368)
    eng.set_weights(weights)
    imgs = images(16, 368, 368, seed=16)
    one = detect(eng, imgs, 0)
    auto = detect(eng, imgs, -1, profile=2)
    per_launch = detect(eng, imgs, -1, profile=1)
    eng.close()
    assert same(one, auto) and same(one, per_launch)
    assert not halves(per_launch[3])
    assert halves(auto[3]) == ['@0+8', '@8+8'], halves(auto[3])          # (the 256 CUs of an MI355X)


def test_no_stale_scratch_between_calls(small):
    """two calls in a row, then off / on / off, with another batch in between: the second chain's slabs carry nothing over"""
    a, b = images(4, seed=1), images(4, seed=2)
    ref_a, ref_b = detect(small, a, 0), detect(small, b, 0)
    assert not same(ref_a, ref_b)
    for imgs, ref, chains in [(a, ref_a, 1), (a, ref_a, 1), (b, ref_b, 1), (a, ref_a, 0), (a, ref_a, 1), (b, ref_b, 0), (a, ref_a, 1), (a, ref_a, 0)]:
        assert same(detect(small, imgs, chains), ref), chains


def test_profile_labels_of_the_halves(small):
    """every launch of the one-chain profile appears twice, "@0+2" and "@2+3", under the same form label, and the FLOP, issued FLOP and
    bytes of the two halves (the one-chain figures scaled by 2/5 and 3/5 in double: a few ulps) add up to the one-chain figures"""
    imgs = images(5, seed=3)
    p0 = detect(small, imgs, 0, profile=True)[3]
    p1 = detect(small, imgs, 1, profile=True)[3]
    assert not halves(p0) and len(p0) >= 40
    got = {(p['layer'], p['kernel']): p for p in p1}
    assert len(got) == 2 * len(p0)
    for p in p0:
        parts = [got.get((p['layer'], p['kernel'] + suffix)) for suffix in ('@0+2', '@2+3')]
        for q in parts:
            assert q is not None and q['launches'] == p['launches'], (p['layer'], p['kernel'])
        for key in ('flop_per_launch', 'issued_flop_per_launch', 'bytes_per_launch'):
            total = parts[0][key] + parts[1][key]
            assert abs(total - p[key]) <= 1e-9 * abs(p[key]), (p['layer'], p['kernel'], key, parts[0][key], parts[1][key], p[key])
    kernels = {p['layer']: p['kernel'] for p in p0}
    assert 'conv1_1+conv1_2' in kernels and any('conv1x1_pair' in kn for kn in kernels.values())
    # the run geometry with a unit-mode tail is among them, with its three entries
    tails = [kn for kn in (p['kernel'] for p in p0) if 'r/t' in kn]
    assert tails and any(kn.endswith(':units') for kn in tails) and any(kn.endswith(':combine') for kn in tails) and any(':' not in kn for kn in tails)


def _hip():
    """the HIP runtime the library has loaded, for a device buffer of the test's own"""
    import ctypes as C
    with open('/proc/self/maps') as f:
        path = next(line.split()[-1] for line in f if 'libamdhip64.so' in line)
    hip = C.CDLL(path)
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    return hip


def test_snapshot_behind_the_call_sees_all_records(native, small):
    """results_snapshot enqueued directly after detect_batch, no host synchronisation in between: the records of both halves"""
    import ctypes as C
    hip = _hip()
    imgs = images(5, seed=4)
    snaps = []
    for chains in (0, 1):
        nbytes = 5 * native.result_dtype(small.capacities()['people']).itemsize
        dev = C.c_void_p()
        assert hip.hipMalloc(C.byref(dev), nbytes) == 0
        small.set_option('batch_chains', chains)
        small.detect_batch(imgs, H, W)
        small.results_snapshot(chains, dev.value, nbytes)
        small.set_option('batch_chains', 0)
        nb, cap, rb, ov = small.snapshot_wait(chains)
        assert (nb, ov) == (5, False) and rb * nb == nbytes
        host = np.empty(nbytes, np.uint8)
        assert hip.hipMemcpy(host.ctypes.data, dev, nbytes, 2) == 0          # (device to host)
        assert hip.hipFree(dev) == 0
        snaps.append(host.tobytes())
    assert snaps[0] == snaps[1] and snaps[1] == small.results().tobytes()
    assert int(small.results()['n_peaks'][3:].sum()) > 0       # (the second chain's images have something to report)


def test_capacity_growth_ends_in_the_same_records(native):
    """capacities too small for the images: the growth (after the join, one chain) ends in the records of a context that was large enough.
    (Four 368 x 368 frames with the head calibrated at that size: 48 x 368 frames have a dozen peaks each, too few to overflow anything.)"""
    Wt = pkg('weights')
    w = Wt.synthetic_weights(0)
    big = native.Engine(0, max_batch=4, max_h=368, max_w=368)
    big.set_weights(w)
    big.forward_u8(images(1, 368, 368, seed=1234))
    paf, heat = big.get_maps()
    w = Wt.calibrate_head(w, paf[0], heat[0])
    big.set_weights({k: w[k] for k in ('Mconv7_stage6_L1', 'Mconv7_stage6_L2')})
    imgs = images(4, 368, 368, seed=6)
    ref = detect(big, imgs, 0)[2]
    big.close()
    print('peaks per image', ref['n_peaks'], 'people', ref['n_people'])
    eng = native.Engine(0, max_batch=4, max_h=368, max_w=368)
    eng.set_weights(w)
    eng.set_capacities(peaks_per_joint=2, subsets=2, people=1)
    got, prof = detect(eng, imgs, 1, profile=True)[2:]
    caps = eng.capacities()
    eng.close()
    assert halves(prof) == ['@0+2', '@2+2']
    assert caps['peaks_per_joint'] > 2
    n = ref['n_people']
    assert np.array_equal(got['n_people'], n) and np.array_equal(got['n_peaks'], ref['n_peaks']) and np.array_equal(got['status'], ref['status'])
    for i in range(4):
        assert np.array_equal(got['poses'][i, :n[i]], ref['poses'][i, :n[i]]) and np.array_equal(got['scores'][i, :n[i]], ref['scores'][i, :n[i]])


def test_mixed_and_precise_calls_are_untouched(native, weights):
    """a mixed-size call and a detect_precise sequence: same results and the same launches with the option at 1 as at 0"""
    rng = np.random.default_rng(8)
    mixed = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in [(48, 368), (64, 96), (48, 368)]]
    net = [im.shape[:2] for im in mixed]
    img = rng.integers(0, 256, (64, 96, 3), dtype=np.uint8)
    eng = native.Engine(0, max_batch=3, max_h=96, max_w=368)
    eng.set_weights(weights)
    out = []
    for chains in (0, 1):
        eng.set_option('batch_chains', chains)
        eng.profile_reset(); eng.profile_enable(True)
        eng.detect_images(mixed, net, net)
        rec = eng.results()
        eng.precise_begin(64, 96)
        eng.precise_add_scale(img, 64, 96)
        eng.precise_add_scale(img, 96, 144)
        eng.precise_finish()
        paf, heat = eng.get_maps()
        prof = sorted((p['layer'], p['kernel'], p['launches']) for p in eng.profile())
        eng.profile_enable(False)
        out.append((rec.tobytes(), paf, heat, prof))
    eng.close()
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    assert out[0][3] == out[1][3] and sum(p[2] for p in out[0][3]) > 100
