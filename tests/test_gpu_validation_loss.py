"""GPU: the validation loss on the device (include/pose_mi355x.h: pmx_loss_* / pmx_validate_batch / pmx_get_labels) against the reference's
own recorded labels and compute_loss values (tests/golden/loss_ref.npz) and against the CPU restatement tests/loss_ref.py."""
import os

import numpy as np
import pytest

import loss_ref
from conftest import GOLDEN, pkg
from test_validation_loss_host import LOSS_CASES, MASKS, mask_of

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23          # one float32 ulp below 1: the device's and glibc's float64 exp may differ in the last bit before the float32 cast


@pytest.fixture(scope='module')
def rec():
    z = np.load(os.path.join(GOLDEN, 'loss_ref.npz'))
    d = {k: z[k] for k in z.files}
    d['sigma'], d['width'] = [float(v) for v in d['sigma_width']]
    return d


@pytest.fixture(scope='module')
def stages():
    z = np.load(os.path.join(GOLDEN, 'ref_checks.npz'))
    return [(z['net_posenet_stage%d_paf' % s], z['net_posenet_stage%d_heat' % s]) for s in range(6)]


@pytest.fixture(scope='module')
def golden_img():
    return np.random.default_rng(1007).integers(0, 256, (1, 64, 96, 3), dtype=np.uint8)      # the input of the net_posenet_stage* goldens


@pytest.fixture(scope='module')
def eng(native):
    e = native.Engine(0, max_batch=2, max_h=64, max_w=96)
    e.set_weights(pkg('weights').synthetic_weights(0))
    yield e
    e.close()


@pytest.fixture(scope='module')
def ref_targets(rec):
    """loss_ref.targets of the recorded labels, per (case, mask): computed once, never modified"""
    out = {}
    for case in LOSS_CASES + ('odd',):
        h, w = [int(v) for v in rec[case + '_hw']]
        for m in MASKS:
            out[case, m] = loss_ref.targets(rec[case + '_paf'], rec[case + '_heat'], mask_of(m, h, w))
    return out


def _rel(a, b):
    return abs(a - b) / b if b else abs(a)


@pytest.mark.parametrize('case', ['generic3', 'axis2', 'empty', 'odd'])
def test_labels_match_the_recorded_reference_labels(native, rec, case):
    h, w = [int(v) for v in rec[case + '_hw']]
    e = native.Engine(0, max_batch=1, max_h=h, max_w=w)
    e.loss_set_poses([rec[case + '_poses']], h, w, None, rec['sigma'], rec['width'])
    paf, heat = e.labels(0)
    e.close()
    dh, dp = np.abs(heat - rec[case + '_heat']).max(), np.abs(paf - rec[case + '_paf']).max()
    print(case, 'heat', dh, 'paf', dp)
    assert dh <= ULP
    assert np.array_equal(paf != 0, rec[case + '_paf'] != 0)
    assert dp <= ULP
    if case == 'empty':
        assert not paf.any() and (heat[18] == 1).all()


@pytest.mark.parametrize('case', ['generic3', 'axis2', 'empty', 'odd'])
def test_targets_from_poses_and_from_maps(native, rec, ref_targets, case):
    h, w = [int(v) for v in rec[case + '_hw']]
    e = native.Engine(0, max_batch=1, max_h=h, max_w=w)
    for m in MASKS:
        mask = mask_of(m, h, w)
        want_p, want_h, want_m = ref_targets[case, m]
        e.loss_set_poses([rec[case + '_poses']], h, w, None if mask is None else mask[None], rec['sigma'], rec['width'])
        paf_t, heat_t, mask_t = e.loss_targets()
        dp, dh = np.abs(paf_t[0] - want_p).max(), np.abs(heat_t[0] - want_h).max()
        print(case, m, 'targets from poses: paf', dp, 'heat', dh)
        assert dp <= ULP and dh <= ULP
        assert np.array_equal(mask_t[0], want_m)
        # the recorded full-size labels, resized on the device: the same float32 operations in the same order
        e.loss_set_targets(rec[case + '_paf'][None], rec[case + '_heat'][None], h, w, None if mask is None else mask[None])
        paf_t, heat_t, mask_t = e.loss_targets()
        assert np.array_equal(paf_t[0], want_p) and np.array_equal(heat_t[0], want_h) and np.array_equal(mask_t[0], want_m)
        # maps already at h/8 x w/8 are taken as they are
        e.loss_set_targets(want_p[None], want_h[None], h, w, want_m[None])
        paf_t, heat_t, mask_t = e.loss_targets()
        assert np.array_equal(paf_t[0], want_p) and np.array_equal(heat_t[0], want_h) and np.array_equal(mask_t[0], want_m)
    e.close()


@pytest.mark.parametrize('case', LOSS_CASES)
@pytest.mark.parametrize('k', [0, 5])
def test_current_maps_loss_of_a_golden_stage(eng, rec, stages, ref_targets, case, k):
    yp, yh = stages[k]
    n_p, n_h = yp.size, yh.size
    for m in MASKS:
        mask = mask_of(m, 64, 96)
        t_p, t_h, t_m = ref_targets[case, m]
        eng.loss_set_targets(rec[case + '_paf'][None], rec[case + '_heat'][None], 64, 96, None if mask is None else mask[None])
        eng.set_maps(yp, yh)
        lp, lh = eng.loss_current_maps()
        rp, rh = loss_ref.stage_loss(yp, yh, t_p[None], t_h[None], t_m[None])
        want = rec['%s_%s_loss' % (case, m)]
        print(case, k, m, 'paf', lp, rp, want[1 + k], 'heat', lh, rh, want[7 + k])
        assert _rel(lp, rp) <= n_p * 2.0 ** -52 and _rel(lh, rh) <= n_h * 2.0 ** -52
        assert abs(lp - want[1 + k]) <= n_p * 2.0 ** -24 * want[1 + k] and abs(lh - want[7 + k]) <= n_h * 2.0 ** -24 * want[7 + k]
        if m == 'all':
            assert lp == 0.0 and lh == 0.0


def _check_validate_against_own_maps(eng, img, t_p, t_h, t_m, fp_tol):
    """pmx_validate_batch's stage-s entry = loss_ref.stage_loss of the maps a forward stopped after stage s returns for the same input"""
    total, paf, heat = eng.validate_batch(img)
    _, _, n = eng.loss_get()
    assert n == 6
    for s in range(1, 7):
        eng.set_option('stop_stage', s)
        try:
            ts, ps, hs = eng.validate_batch(img)
            p6, h6, ns = eng.loss_get()
            eng.forward_u8(img)
            yp, yh = eng.get_maps()
        finally:
            eng.set_option('stop_stage', 6)
        assert ns == s
        assert not ps[s:].any() and not hs[s:].any()
        assert np.array_equal(ps[:s], paf[:s]) and np.array_equal(hs[:s], heat[:s])
        rp, rh = loss_ref.stage_loss(yp, yh, t_p, t_h, t_m)
        print('stage', s, 'paf', paf[s - 1], rp, 'heat', heat[s - 1], rh)
        assert _rel(paf[s - 1], rp) <= yp.size * fp_tol and _rel(heat[s - 1], rh) <= yh.size * fp_tol
    assert total == sum(float(p) + float(h) for p, h in zip(paf, heat))
    return total, paf, heat


def test_validate_batch_on_the_golden_input(eng, rec, golden_img, ref_targets):
    case = 'generic3'
    t_p, t_h, t_m = ref_targets[case, 'none']
    eng.loss_set_poses([rec[case + '_poses']], 64, 96, None, rec['sigma'], rec['width'])
    tp, th, tm = eng.loss_targets()
    total, paf, heat = _check_validate_against_own_maps(eng, golden_img, tp, th, tm, 2.0 ** -52)
    # the reference's own six stages: its maps are reproduced within 1e-4 (test_gpu_reference_goldens.py), so a loss moves by
    # at most 2e-4 * sqrt(loss)
    want = rec[case + '_none_loss']
    for s in range(6):
        print('stage', s + 1, 'vs reference: paf', paf[s], want[1 + s], 'heat', heat[s], want[7 + s])
        assert abs(paf[s] - want[1 + s]) <= 2e-4 * np.sqrt(want[1 + s]) + 1e-8
        assert abs(heat[s] - want[7 + s]) <= 2e-4 * np.sqrt(want[7 + s]) + 1e-8
    again = eng.validate_batch(golden_img)
    assert again[0] == total and np.array_equal(again[1], paf) and np.array_equal(again[2], heat)          # the same bits


def test_batch_of_two_and_maps_unchanged_by_the_hook(eng, rec, golden_img):
    imgs = np.concatenate([golden_img, np.random.default_rng(5).integers(0, 256, (1, 64, 96, 3), dtype=np.uint8)])
    masks = np.zeros((2, 64, 96), bool)
    masks[1] = True
    eng.loss_set_poses([rec['axis2_poses'], np.zeros((0, 18, 3))], 64, 96, masks, rec['sigma'], rec['width'])
    t = [loss_ref.targets(*loss_ref.labels((64, 96), p, rec['sigma'], rec['width']), mask=m)
         for p, m in ((rec['axis2_poses'], masks[0]), (np.zeros((0, 18, 3)), masks[1]))]
    t_p, t_h, t_m = (np.stack([a[i] for a in t]) for i in range(3))
    tp, th, tm = eng.loss_targets()
    assert np.abs(tp - t_p).max() <= ULP and np.abs(th - t_h).max() <= ULP and np.array_equal(tm, t_m)
    assert tm[1].all() and not tm[0].any()
    # every stage of the batch against loss_ref on the maps a forward stopped there returns
    total, paf, heat = _check_validate_against_own_maps(eng, imgs, tp, th, tm, 2.0 ** -52)
    again = eng.validate_batch(imgs)
    assert again[0] == total and np.array_equal(again[1], paf) and np.array_equal(again[2], heat)
    hooked = eng.get_maps()
    eng.forward_u8(imgs)
    plain = eng.get_maps()
    assert np.array_equal(hooked[0], plain[0]) and np.array_equal(hooked[1], plain[1])
    rp, rh = loss_ref.stage_loss(plain[0], plain[1], tp, th, tm)
    print('batch of two: paf', paf[5], rp, 'heat', heat[5], rh)
    assert _rel(paf[5], rp) <= plain[0].size * 2.0 ** -52 and _rel(heat[5], rh) <= plain[1].size * 2.0 ** -52
    # the hook left on: a plain forward accumulates the same losses
    eng.loss_enable(True)
    try:
        eng.forward_u8(imgs)
        p6, h6, n = eng.loss_get()
    finally:
        eng.loss_enable(False)
    assert n == 6 and np.array_equal(p6, paf) and np.array_equal(h6, heat)


def test_validate_batch_in_f16_mode(native, rec, golden_img):
    e = native.Engine(0, max_batch=1, max_h=64, max_w=96)
    e.set_weights(pkg('weights').synthetic_weights(0))
    e.set_option('precision', 2)
    e.loss_set_poses([rec['generic3_poses']], 64, 96, None, rec['sigma'], rec['width'])
    tp, th, tm = e.loss_targets()
    _check_validate_against_own_maps(e, golden_img, tp, th, tm, 2.0 ** -52)
    e.close()


def test_errors_leave_the_context_usable(native, eng, rec, golden_img):
    def code(fn, *a, **k):
        with pytest.raises(native.PmxError) as ei:
            fn(*a, **k)
        assert str(ei.value).split(': ', 1)[1].strip(), 'no message'
        return ei.value.code
    INVALID, CAPACITY, STATE = 1, 5, 6
    eng.detect_batch(golden_img, 64, 96)
    before = eng.results().copy()
    poses = rec['generic3_poses']
    for arch in ('facenet', 'handnet'):
        f = native.Engine(0, max_batch=1, max_h=64, max_w=96, arch=arch)
        assert code(f.loss_enable, True) == STATE
        assert code(f.loss_set_poses, [poses], 64, 96) == STATE
        assert code(f.validate_batch, golden_img) == STATE
        f.close()
    fresh = native.Engine(0, max_batch=1, max_h=64, max_w=96)
    fresh.set_weights(pkg('weights').synthetic_weights(0))
    assert code(fresh.loss_get) == STATE                                   # no hooked forward yet
    assert code(fresh.validate_batch, golden_img) == STATE                 # no targets
    assert code(fresh.loss_current_maps) == STATE
    assert code(fresh.labels) == STATE and code(fresh.loss_targets) == STATE       # no poses / targets yet
    fresh.close()
    assert code(eng.loss_set_poses, [poses], 64, 96, None, 0.0, 8.0) == INVALID
    assert code(eng.loss_set_poses, [poses], 64, 96, None, 7.0, -1.0) == INVALID
    assert code(eng.loss_set_poses, [poses], 60, 96) == INVALID
    bad = poses.copy()
    bad[0, np.argmax(bad[0, :, 2] > 0), 0] = np.inf
    assert code(eng.loss_set_poses, [bad], 64, 96) == INVALID
    def raw(rc, word):
        assert rc == INVALID and word in eng.lib.pmx_last_error().decode(), (rc, eng.lib.pmx_last_error())
    n = np.array([-1], np.int32)
    raw(eng.lib.pmx_loss_set_poses(eng._ctx, native._ptr(poses), native._ptr(n), 1, 64, 96, None, 7.0, 8.0), 'n_people[0] = -1')
    raw(eng.lib.pmx_loss_set_poses(eng._ctx, native._ptr(poses), None, 1, 64, 96, None, 7.0, 8.0), 'null')
    one = np.array([1], np.int32)
    raw(eng.lib.pmx_loss_set_poses(eng._ctx, None, native._ptr(one), 1, 64, 96, None, 7.0, 8.0), 'null poses')
    raw(eng.lib.pmx_loss_get(eng._ctx, None, None, None), 'null')
    raw(eng.lib.pmx_loss_current_maps(eng._ctx, None, None), 'null')
    raw(eng.lib.pmx_validate_batch(eng._ctx, None, 1, 64, 96, 0, None), 'null')
    raw(eng.lib.pmx_loss_set_targets(eng._ctx, None, None, None, 1, 64, 96, 64, 96), 'null')
    assert code(eng.loss_set_poses, [poses] * 3, 64, 96) == CAPACITY
    assert code(eng.loss_set_poses, [poses], 64, 104) == CAPACITY
    assert code(eng.loss_set_targets, np.zeros((1, 38, 16, 24), 'f'), np.zeros((1, 19, 16, 24), 'f'), 64, 96) == INVALID
    eng.loss_set_poses([poses], 64, 96)
    eng.loss_enable(True)
    try:
        assert code(eng.forward_u8, np.concatenate([golden_img, golden_img])) == STATE          # targets of another batch
        assert code(eng.forward_u8, golden_img[:, :56]) == STATE                                # ... of another h
        assert code(eng.forward_u8, golden_img[:, :, :88]) == STATE                             # ... of another w
        assert code(eng.detect_batch, golden_img[:, :, :88], 64, 88) == STATE
        assert code(eng.forward_u8_images, [golden_img[0], golden_img[0, :56]]) == STATE
        assert code(eng.detect_images, [golden_img[0]], [(64, 96)], [(64, 96)]) == STATE
        assert code(eng.precise_begin, 64, 96) == STATE
        assert code(eng.detect_precise_images, [golden_img[0]], [[(64, 96)]]) == STATE
    finally:
        eng.loss_enable(False)
    eng.detect_batch(golden_img, 64, 96)
    assert eng.results().tobytes() == before.tobytes()


def test_detector_validation_loss_equals_the_engine(native, rec, golden_img):
    PD = pkg('pose_detector')
    det = PD.PoseDetector(weights=pkg('weights').synthetic_weights(0), device=0, max_batch=2, max_size=(64, 96))
    rng = np.random.default_rng(9)
    imgs = [golden_img[0]] + [rng.integers(0, 256, (64, 96, 3), dtype=np.uint8) for _ in range(2)]
    poses = [rec['generic3_poses'], rec['axis2_poses'], np.zeros((0, 18, 3))]
    masks = [mask_of(m, 64, 96) if m != 'none' else np.zeros((64, 96), bool) for m in ('none', 'left', 'px00')]
    got = det.validation_loss(imgs, poses, masks)                                  # chunks of 2 and 1
    eng = det.engine
    eng.loss_set_poses(poses[:2], 64, 96, np.stack(masks[:2]))
    a = eng.validate_batch(np.stack(imgs[:2]))
    eng.loss_set_poses(poses[2:], 64, 96, np.stack(masks[2:]))
    b = eng.validate_batch(np.stack(imgs[2:]))
    paf, heat = (2 * a[1] + b[1]) / 3, (2 * a[2] + b[2]) / 3
    assert got['paf_stages'] == [float(v) for v in paf] and got['heat_stages'] == [float(v) for v in heat]
    assert got['val/loss'] == float((2 * a[0] + b[0]) / 3) and got['val/paf'] == float(paf.sum()) and got['val/heat'] == float(heat.sum())
    one = det.validation_loss(imgs[:1], poses[:1])
    eng.loss_set_poses(poses[:1], 64, 96)
    assert one['val/loss'] == eng.validate_batch(np.stack(imgs[:1]))[0]
    paf_l, heat_l = det.generate_labels((64, 96), rec['axis2_poses'])
    assert np.abs(paf_l - rec['axis2_paf']).max() <= ULP and np.abs(heat_l - rec['axis2_heat']).max() <= ULP
