"""GPU: the opt-in f16 inference mode (engine option "precision" = 2, `precision='f16'` on the detectors) against its arithmetic
contract (tests/f16_emulation.py; include/pose_mi355x.h): single layers, saturation, whole-network maps,
invariance of an image's bits to the launch it is part of, the detectors' entry points, and the option's edges."""
import os

import numpy as np
import pytest

import f16_emulation as E
from conftest import GOLDEN, pkg
from test_reference_network import _x, load_e2e

pytestmark = pytest.mark.gpu

# Network maps (tests/golden/net_posenet_*: shapes and seeds).  Measured on CPU with f16_emulation: the emulation with fp32 sums against
# the one with float64 sums differs by 1.22e-3 / 1.45e-3 (paf / heat, 64 x 96) and 1.24e-3 / 2.02e-3 (184 x 248) relative to
# max(1, max |ref|): a summation-order difference moves an activation across an f16 rounding boundary of the next layer, and that
# travels.  The GPU's fp32 order is a third order: bound = 4 x the largest measured.
NET_EMU_BOUND = 8e-3
# f16 emulation against the fp32 reference (oracle/network_ref): 1.21e-3 / 1.35e-3 (64 x 96), 1.65e-3 / 2.12e-3 (184 x 248);
# GPU f16 against GPU f32 = that plus the order noise of both: bound = 4 x 2.12e-3 + the emulation bound's share, rounded up.
NET_F32_BOUND = 1.2e-2


def _f16(eng):
    eng.set_option('precision', 2)


def _f32(eng):
    eng.set_option('precision', 0)


LAYER_CASES = [
    # (ks, cin, cout, relu, pool, B, H, W)
    (3, 3, 64, True, False, 2, 46, 46),           # conv1_1's shape (cin 3 -> one 16-channel chunk)
    (3, 64, 64, True, True, 1, 46, 46),
    (3, 64, 128, False, False, 3, 23, 31),
    (3, 128, 256, True, True, 2, 22, 30),
    (3, 512, 128, True, False, 1, 11, 13),
    (3, 185, 128, True, False, 4, 9, 7),
    (7, 185, 128, True, False, 2, 46, 46),        # Mconv1's shape (the concat input)
    (7, 128, 128, True, False, 1, 23, 31),
    (7, 128, 512, False, False, 1, 13, 17),
    (7, 64, 256, True, True, 2, 10, 14),
    (7, 512, 64, True, False, 1, 5, 9),
]


@pytest.mark.parametrize('case', LAYER_CASES, ids=lambda c: 'k%d_ci%d_co%d_r%d_p%d_b%d_%dx%d' % tuple(int(v) for v in c))
def test_single_layer_matches_emulation(engine, case):
    ks, cin, cout, relu, pool, B, H, W = case
    rng = np.random.default_rng(ks * 1000 + cin + cout + H)
    x = rng.uniform(-1, 1, (B, cin, H, W)).astype(np.float32)
    Wt = (rng.standard_normal((cout, cin, ks, ks)) / np.sqrt(cin * ks * ks)).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, cout).astype(np.float32)
    ref = E.conv_f16(x, Wt, b, relu, pool)
    unrounded = E.conv_f16(x, Wt, b, relu, pool, rounded=False)
    tol = 2e-5 * max(1.0, float(np.abs(ref).max()))
    _f16(engine)
    try:
        y = engine.conv2d(x, Wt, b, relu=relu, pool=pool)
    finally:
        _f32(engine)
    assert y.shape == ref.shape and np.isfinite(y).all()
    err = float(np.abs(y - ref).max())
    assert err <= tol, (err, tol)
    # negative control: the rounding of the operands is visible, i.e. the f16 kernel ran
    assert float(np.abs(y - unrounded).max()) > 10 * tol


def test_saturation(engine):
    rng = np.random.default_rng(5)
    x = (rng.uniform(-1, 1, (1, 32, 16, 16)) * 1e5).astype(np.float32)       # many beyond +-65504
    x[0, 0, :4, :4] = 7e4
    Wt = (rng.standard_normal((64, 32, 3, 3)) * 0.05).astype(np.float32)
    Wt[0, 0, 0, 0] = 1e5
    b = np.zeros(64, np.float32)
    ref = E.conv_f16(x, Wt, b)
    _f16(engine)
    try:
        y = engine.conv2d(x, Wt, b)
    finally:
        _f32(engine)
    assert np.isfinite(y).all()
    assert float(np.abs(y - ref).max()) <= 2e-5 * float(np.abs(ref).max())


def _net_maps(native, seed, h, w, precision):
    img, x = _x('posenet', seed, h, w)
    eng = native.Engine(0, max_batch=1, max_h=h, max_w=w)
    eng.set_weights(pkg('weights').synthetic_weights(seed))
    eng.set_option('precision', precision)
    eng.forward_u8(img)
    paf, heat = eng.get_maps()
    eng.close()
    return paf, heat, x


@pytest.mark.parametrize('name', ['net_posenet_64x96', 'net_posenet_184x248'])
def test_network_maps(native, name):
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    seed = int(z['seed'])
    h, w = [int(v) for v in z['hw']]
    paf, heat, x = _net_maps(native, seed, h, w, 2)
    paf32, heat32, _ = _net_maps(native, seed, h, w, 0)
    epaf, eheat = E.forward_f16(pkg('weights').synthetic_weights(seed), x)
    e_emu = max(E.rel_err(paf, epaf), E.rel_err(heat, eheat))
    e_f32 = max(E.rel_err(paf, paf32), E.rel_err(heat, heat32))
    print('%s: f16 vs emulation %.3g, f16 vs f32 %.3g' % (name, e_emu, e_f32))
    assert e_emu <= NET_EMU_BOUND and e_f32 <= NET_F32_BOUND, (e_emu, e_f32)
    assert not np.array_equal(paf, paf32)


def test_invariance_and_determinism(native):
    seed = 0
    w = pkg('weights').synthetic_weights(seed)
    rng = np.random.default_rng(21)
    img = rng.integers(0, 256, (184, 248, 3), dtype=np.uint8)
    others = rng.integers(0, 256, (8, 184, 248, 3), dtype=np.uint8)
    eng = native.Engine(0, max_batch=8, max_h=368, max_w=368)
    eng.set_weights(w)
    eng.forward_u8(img[None])
    f32_before = eng.get_maps()
    _f16(eng)
    eng.forward_u8(img[None])
    alone = eng.get_maps()
    eng.forward_u8(img[None])
    again = eng.get_maps()
    assert all(np.array_equal(a, b) for a, b in zip(alone, again))
    assert not np.array_equal(alone[0], f32_before[0])
    for pos in (0, 5):
        batch = others.copy()
        batch[pos] = img
        eng.forward_u8(batch)
        paf, heat = eng.get_maps()
        assert np.array_equal(paf[pos], alone[0][0]) and np.array_equal(heat[pos], alone[1][0]), pos
    # inside a mixed-size batch (one launch per layer over all size classes)
    mixed = [rng.integers(0, 256, (240, 320, 3), dtype=np.uint8), img, rng.integers(0, 256, (368, 368, 3), dtype=np.uint8), img]
    eng.forward_u8_images(mixed)
    for i in (1, 3):
        paf, heat = eng.image_maps(i)
        assert np.array_equal(paf, alone[0][0]) and np.array_equal(heat, alone[1][0]), i
    # back to fp32: the f32 bits of before
    _f32(eng)
    eng.forward_u8(img[None])
    f32_after = eng.get_maps()
    assert all(np.array_equal(a, b) for a, b in zip(f32_before, f32_after))
    # set_layer after an f16 run takes effect in f16 mode (the f16 pack was dropped with the fp32 one)
    _f16(eng)
    W1, b1 = w['conv3_1']
    eng.set_layer('conv3_1', W1 * np.float32(0.5), b1)
    eng.forward_u8(img[None])
    changed = eng.get_maps()
    assert not np.array_equal(changed[0], alone[0])
    eng.set_layer('conv3_1', W1, b1)
    eng.forward_u8(img[None])
    restored = eng.get_maps()
    assert all(np.array_equal(a, b) for a, b in zip(restored, alone))
    eng.close()


# Poses of the f16 mode against the f32 path on the reference's images.  Measured on the GPU (first runs of this file): e2e_people gave
# 9 people in f16 mode against 8 in fp32 -- one marginal person whose grouping score sits at a threshold the f16 noise crosses -- and on
# a crop of it one key point went to a neighbouring person (a near-tie limb candidate).  So the contract is on the key points, not on
# their grouping: person counts within POSE_EXTRA of each other, and every key point of either result has a key point of the same
# joint type in the other within POSE_PX pixels at the original scale, except at most max(POSE_MISSING, 10 %) of them (a marginal
# person's own key points among them).
POSE_PX = 4.0
POSE_MISSING = 3
POSE_EXTRA = 1


def _pose_agree(pa, pb):
    pa, pb = np.asarray(pa, np.float64).reshape(-1, 18, 3), np.asarray(pb, np.float64).reshape(-1, 18, 3)
    assert abs(len(pa) - len(pb)) <= POSE_EXTRA, (len(pa), len(pb))

    def unmatched(x, y):
        n, bad = 0, 0
        for j in range(18):
            px, py = x[:, j][x[:, j, 2] > 0, :2], y[:, j][y[:, j, 2] > 0, :2]
            for p in px:
                n += 1
                bad += int(len(py) == 0 or float(np.abs(py - p).max(axis=1).min()) > POSE_PX)
        return n, bad
    na, ba = unmatched(pa, pb)
    nb, bb = unmatched(pb, pa)
    assert max(ba, bb) <= max(POSE_MISSING, 0.1 * max(na, nb)), (ba, bb, na, nb)
    return len(pa), len(pb), na, nb, ba, bb


@pytest.mark.parametrize('name', ['e2e_person', 'e2e_people', 'e2e_dinner'])
def test_pose_detector_call(native, name):
    PD = pkg('pose_detector')
    g = load_e2e(name)
    d16 = PD.PoseDetector(weights=g['weights'], device=0, precision='f16')
    d32 = PD.PoseDetector(weights=g['weights'], device=0)
    p16, _ = d16(g['img'])
    p32, _ = d32(g['img'])
    assert d16.engine._options.get('precision') == 2
    print(name, 'people / key points / unmatched', _pose_agree(p16, p32))
    d16.engine.close(); d32.engine.close()


def test_detect_batch_uniform_and_mixed(native):
    PD = pkg('pose_detector')
    g = load_e2e('e2e_people')
    img = g['img']
    d16 = PD.PoseDetector(weights=g['weights'], device=0, precision='f16')
    d32 = PD.PoseDetector(weights=g['weights'], device=0)
    one16, _ = d16(img)
    uni = d16.detect_batch([img, img[:, ::-1].copy(), img])         # (grows the engine: the option must survive)
    assert d16.engine._options.get('precision') == 2
    assert np.array_equal(np.asarray(uni[0][0]), np.asarray(one16)) and np.array_equal(np.asarray(uni[2][0]), np.asarray(one16))
    small = np.ascontiguousarray(img[: img.shape[0] * 2 // 3, : img.shape[1] // 2])
    mixed = d16.detect_batch([small, img])
    assert np.array_equal(np.asarray(mixed[1][0]), np.asarray(one16))
    print('mixed people / key points / unmatched', _pose_agree(mixed[0][0], d32(small)[0]))
    d16.engine.close(); d32.engine.close()


def test_detect_precise(native):
    PD = pkg('pose_detector')
    g = load_e2e('e2e_precise_people_crop')
    d16 = PD.PoseDetector(weights=g['weights'], device=0, precise=True, precision='f16')
    d32 = PD.PoseDetector(weights=g['weights'], device=0, precise=True)
    p16, _ = d16(g['img'])
    p32, _ = d32(g['img'])
    print('precise people / key points / unmatched', _pose_agree(p16, p32))
    d16.engine.close(); d32.engine.close()


def test_face_hand_detect_boxes(native):
    PD, FH, W = pkg('pose_detector'), pkg('face_hand_detector'), pkg('weights')
    g = load_e2e('e2e_dinner')
    z = np.load(os.path.join(GOLDEN, 'demo_chain_dinner.npz'))
    img = g['img']
    det = PD.PoseDetector(weights=g['weights'], device=0)
    poses, _ = det(img)
    boxes, hboxes, sides = [], [], []
    for i in z['persons']:
        pose = np.asarray(poses[int(i)]).copy()
        unit = det.get_unit_length(pose)
        face, bbox = det.crop_face(img, pose, unit)
        if face is not None:
            boxes.append(tuple(bbox))
        hands = det.crop_hands(img, pose, unit)
        for side in ('left', 'right'):
            if hands[side] is not None:
                hboxes.append(tuple(hands[side]['bbox'])); sides.append(side)
    assert boxes and hboxes
    for cls, arch, seed, bx, extra in (('FaceDetector', 'facenet', int(z['face_seed']), boxes, ()),
                                       ('HandDetector', 'handnet', int(z['hand_seed']), hboxes, (sides,))):
        d16 = getattr(FH, cls)(arch, weights=W.synthetic_weights(seed, arch), device=0, precision='f16')
        d32 = getattr(FH, cls)(arch, weights=W.synthetic_weights(seed, arch), device=0)
        k16 = d16.detect_boxes(img, bx, *extra)
        k32 = d32.detect_boxes(img, bx, *extra)
        assert d16.engine._options.get('precision') == 2
        assert len(k16) == len(k32)
        n, moved = 0, 0
        for a, b in zip(k16, k32):
            for p, q in zip(a, b):
                if p is None or q is None:
                    moved += int((p is None) != (q is None))
                    continue
                n += 1
                if abs(p[0] - q[0]) > 2 or abs(p[1] - q[1]) > 2:
                    moved += 1
        print(cls, n, 'key points,', moved, 'moved')
        assert n > 0 and moved <= max(2, n // 20), (moved, n)
        d16.engine.close(); d32.engine.close()
    det.engine.close()


def test_option_errors_leave_results_unchanged(native):
    seed = 0
    img, _ = _x('posenet', seed, 64, 96)
    eng = native.Engine(0, max_batch=1, max_h=64, max_w=96)
    eng.set_weights(pkg('weights').synthetic_weights(seed))
    for mode in (0, 2):
        eng.set_option('precision', mode)
        eng.forward_u8(img)
        before = eng.get_maps()
        for bad in (-1, 3):
            with pytest.raises(Exception):
                eng.set_option('precision', bad)
        eng.forward_u8(img)
        after = eng.get_maps()
        assert all(np.array_equal(a, b) for a, b in zip(before, after)), mode
    eng.close()
