"""GPU: the opt-in f16 inference mode (engine option "precision" = 2, `precision='f16'` on the detectors) against its arithmetic
contract (tests/f16_emulation.py; include/pose_mi355x.h): single layers, saturation, whole-network maps,
invariance of an image's bits to the launch it is part of, the detectors' entry points, and the option's edges.

The launch forms of conv_f16_kernel -- KS 3 | 7, BN 64 | 128 channels per block (option "f16_bn" forces either at any size), one or two
groups (Engine.conv2d_pair), pooled or not, with or without the segment table of a mixed-size forward -- each under a tight check:
test_forms_single_layer, test_forms_pairs, test_forms_network; the operand edges (f16 subnormals, ties, NaN, infinities) in
test_subnormal_lattice_is_exact and test_nan_and_infinities."""
import functools
import os

import numpy as np
import pytest

import f16_emulation as E
from conftest import GOLDEN, pkg
from oracle import network_ref
from test_gpu_winograd import TOL as F32_TOL
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


def _case_id(c):
    return 'k%d_ci%d_co%d_r%d_p%d_b%d_%dx%d' % tuple(int(v) for v in c)


def _layer_data(case, salt=0):
    """The file's operand distribution for a case (ks, cin, cout, relu, pool, B, H, W)."""
    ks, cin, cout, relu, pool, B, H, W = case
    rng = np.random.default_rng(ks * 1000 + cin + cout + H + salt)
    x = rng.uniform(-1, 1, (B, cin, H, W)).astype(np.float32)
    Wt = (rng.standard_normal((cout, cin, ks, ks)) / np.sqrt(cin * ks * ks)).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, cout).astype(np.float32)
    return x, Wt, b


@pytest.mark.parametrize('case', LAYER_CASES, ids=_case_id)
def test_single_layer_matches_emulation(engine, case):
    ks, cin, cout, relu, pool, B, H, W = case
    x, Wt, b = _layer_data(case)
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


# ---- the launch forms, forced at small shapes (option "f16_bn", Engine.conv2d_pair) ------------------------------------------------------
FORM_CASES = [
    # (ks, cin, cout, relu, pool, B, H, W)
    (7, 48, 128, 1, 0, 2, 13, 21),                # ragged on both edges
    (7, 185, 130, 1, 0, 1, 9, 17),                # partial chunk, a part-used channel block (cout_pad 256)
    (3, 64, 128, 1, 1, 3, 10, 18),                # pooled, ragged
    (3, 3, 128, 0, 0, 1, 8, 16),                  # exactly one tile, one chunk
    (7, 32, 256, 0, 0, 1, 3, 5),                  # the image is smaller than the kernel
    (7, 64, 128, 1, 1, 2, 12, 20),                # 7x7 pooled, ragged
    (3, 32, 64, 1, 0, 2, 9, 17),                  # cout_pad 64: "f16_bn" = 128 does not apply, the launch stays at 64
]


@functools.lru_cache(maxsize=None)
def _form_ref(case):
    """(x, W, b, emulation with float64 sums, the same on unrounded operands, tol): computed once per case; nobody writes to them."""
    x, Wt, b = _layer_data(case)
    ref = E.conv_f16(x, Wt, b, case[3], case[4])
    unrounded = E.conv_f16(x, Wt, b, case[3], case[4], rounded=False)
    return x, Wt, b, ref, unrounded, 2e-5 * max(1.0, float(np.abs(ref).max()))


def _with_f16(engine, bn, fn):
    engine.set_option('precision', 2)
    engine.set_option('f16_bn', bn)
    try:
        return fn()
    finally:
        engine.set_option('f16_bn', 0)
        engine.set_option('precision', 0)


@pytest.mark.parametrize('case', FORM_CASES, ids=_case_id)
def test_forms_single_layer(engine, case):
    """conv_f16_kernel<KS, 64> and <KS, 128> on the same small layer: each within the single-layer bound of the emulation, finite
    everywhere (the output is poisoned), the operand rounding visible -- and the two bit-equal (the contract: nothing depends on BN)."""
    ks, cin, cout, relu, pool, B, H, W = case
    x, Wt, b, ref, unrounded, tol = _form_ref(case)
    ys = {bn: _with_f16(engine, bn, lambda: engine.conv2d(x, Wt, b, relu=bool(relu), pool=bool(pool))) for bn in (64, 128)}
    for bn, y in ys.items():
        assert y.shape == ref.shape and np.isfinite(y).all(), bn
        err, ctl = float(np.abs(y - ref).max()), float(np.abs(y - unrounded).max())
        print('f16_bn %d: err %.3g = %.3g tol, control %.3g tol' % (bn, err, err / tol, ctl / tol))
        assert err <= tol, (bn, err, tol)
        assert ctl > 10 * tol, (bn, ctl, tol)
    assert np.array_equal(ys[64], ys[128]), (float(np.abs(ys[64] - ys[128]).max()), int((ys[64] != ys[128]).sum()))


def test_f16_bn_option_values(engine):
    for bad in (-1, 1, 32, 96, 256):
        with pytest.raises(Exception):
            engine.set_option('f16_bn', bad)
    for good in (64, 128, 0):
        engine.set_option('f16_bn', good)


# (single-layer case, couts of the two groups)
PAIR_CASES = [(FORM_CASES[0], (128, 128)), (FORM_CASES[2], (128, 128)), ((3, 48, 128, 1, 0, 2, 9, 17), (100, 128))]


def _pair_data(case, couts):
    """Group 0: the case's own operands (its first couts[0] output channels); group 1: a second draw of the same distribution."""
    x0, W0, b0 = _layer_data(case)
    x1, W1, b1 = _layer_data(case, salt=7)
    return x0, W0[:couts[0]], b0[:couts[0]], x1, W1[:couts[1]], b1[:couts[1]]


@pytest.mark.parametrize('case,couts', PAIR_CASES, ids=lambda v: _case_id(v) if len(v) == 8 else 'co%d_%d' % v)
def test_forms_pairs(engine, case, couts):
    """Two groups in one launch (blockIdx.z = 1; inputs and outputs as channel slices of wider buffers), shared and separate inputs,
    BN 64 and 128: each group's output is bit-equal to conv2d of that group alone, and swapping the groups swaps the outputs."""
    relu, pool = bool(case[3]), bool(case[4])
    x0, W0, b0, x1, W1, b1 = _pair_data(case, couts)

    def run():
        alone = {(g, i): engine.conv2d(x, Wg, bg, relu=relu, pool=pool) for g, i, x, Wg, bg in ((0, 0, x0, W0, b0), (1, 0, x0, W1, b1), (1, 1, x1, W1, b1))}
        out = {}
        for bn in (64, 128):
            engine.set_option('f16_bn', bn)
            out[bn, 'shared'] = engine.conv2d_pair(x0, W0, b0, W1, b1, relu=relu, pool=pool)
            out[bn, 'separate'] = engine.conv2d_pair(x0, W0, b0, W1, b1, x1=x1, relu=relu, pool=pool)
            out[bn, 'shared swapped'] = engine.conv2d_pair(x0, W1, b1, W0, b0, relu=relu, pool=pool)[::-1]
            out[bn, 'separate swapped'] = engine.conv2d_pair(x1, W1, b1, W0, b0, x1=x0, relu=relu, pool=pool)[::-1]
        return alone, out
    alone, out = _with_f16(engine, 64, run)
    assert not np.array_equal(alone[0, 0][:, :min(couts)], alone[1, 0][:, :min(couts)])
    for (bn, how), (y0, y1) in out.items():
        i1 = int(how.startswith('separate'))
        assert np.isfinite(y0).all() and np.isfinite(y1).all(), (bn, how)
        assert np.array_equal(y0, alone[0, 0]), (bn, how, float(np.abs(y0 - alone[0, 0]).max()))
        assert np.array_equal(y1, alone[1, i1]), (bn, how, float(np.abs(y1 - alone[1, i1]).max()))


def test_pair_entry_fp32(engine):
    """conv2d_pair outside the f16 mode: the direct fp32 kernels with two groups, against the float64 reference at the fp32 bound."""
    case, couts = PAIR_CASES[2]
    x0, W0, b0, x1, W1, b1 = _pair_data(case, couts)
    engine.set_option('precision', 0)
    engine.set_option('conv_algo', 0)
    engine.set_option('ksplit', 1)
    try:
        y0, y1 = engine.conv2d_pair(x0, W0, b0, W1, b1, x1=x1, relu=True)
        s0, s1 = engine.conv2d_pair(x0, W0, b0, W1, b1, relu=True)
    finally:
        engine.set_option('ksplit', 0)
    for y, x, Wg, bg in ((y0, x0, W0, b0), (y1, x1, W1, b1), (s0, x0, W0, b0), (s1, x0, W1, b1)):
        t = network_ref.conv2d_ref(x, Wg, bg, relu=True, pool=False)
        assert y.shape == t.shape and np.isfinite(y).all()
        assert np.abs(y - t).max() <= F32_TOL * max(1.0, np.abs(t).max())


def test_forms_network(native):
    """The segment table of a mixed-size forward and the two-group stage launches at BN = 128, at the smallest sizes: an image's maps
    are bit-equal alone (BN 64 and 128), inside a uniform batch of 3 and inside a mixed list, at both widths."""
    rng = np.random.default_rng(33)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((24, 40), (40, 24), (16, 16))]
    eng = native.Engine(0, max_batch=4, max_h=40, max_w=40)
    try:
        eng.set_weights(pkg('weights').synthetic_weights(0))
        eng.set_option('precision', 2)
        eng.set_option('f16_bn', 64)
        alone = []
        for img in imgs:
            eng.forward_u8(img[None])
            alone.append([m[0] for m in eng.get_maps()])
            assert all(np.isfinite(m).all() and np.abs(m).max() > 0 for m in alone[-1])
        for bn in (64, 128):
            eng.set_option('f16_bn', bn)
            for i, img in enumerate(imgs):
                for pos, B in ((0, 1), (1, 3)):
                    batch = rng.integers(0, 256, (B,) + img.shape, dtype=np.uint8)
                    batch[pos] = img
                    eng.forward_u8(batch)
                    paf, heat = eng.get_maps()
                    assert np.array_equal(paf[pos], alone[i][0]) and np.array_equal(heat[pos], alone[i][1]), (bn, i, B)
            eng.forward_u8_images(imgs)
            for i in range(len(imgs)):
                paf, heat = eng.image_maps(i)
                assert np.array_equal(paf, alone[i][0]) and np.array_equal(heat, alone[i][1]), (bn, i, 'mixed')
    finally:
        eng.close()


# ---- operand edges ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['a', 'b', 'c', 'd'])
@pytest.mark.parametrize('ks,cin', [(3, 16), (3, 48), (7, 16), (7, 48)])
def test_subnormal_lattice_is_exact(engine, kind, ks, cin):
    """Zero tolerance, by derivation (f16_emulation.lattice_case; its premise is tests/test_f16_host.py::
    test_emulation_is_exact_on_the_lattice): every product and every partial sum is exactly representable in fp32, so the kernel must
    EQUAL the float64 convolution of the f16-rounded operands, whatever its summation order.  'a': every activation an f16 subnormal --
    the kernel's conversion and the matrix core must keep them; 'b': every weight one, half of them at ties and a few below 2^-25 --
    the host packer's subnormal / tie branch, through the device; 'c': those unrounded values as activations, 'd': activations at the
    ties of [1, 2] -- the kernel's conversion rounds to nearest even, subnormals included."""
    x, Wt, b = E.lattice_case(kind, ks, cin, seed=ks * 100 + cin)
    ref = E.conv_f16(x, Wt, b)
    assert np.abs(ref).max() > 0.01
    for bn in (64, 128):
        y = _with_f16(engine, bn, lambda: engine.conv2d(x, Wt, b))
        bad = y != ref
        assert not bad.any(), (bn, int(bad.sum()), float(np.abs(y - ref).max()))
    if kind != 'a':
        assert not np.array_equal(y, E.conv_f16(x, Wt, b, rounded=False))


@pytest.mark.parametrize('ks', [3, 7])
def test_nan_and_infinities(engine, ks):
    """f16(NaN) is NaN and f16(+-inf) is +-65504, for activations (the kernel's conversion) and weights (the host packer): the NaN
    pattern of the output equals the emulation's, every other output is finite and within the single-layer bound -- also through the
    ReLU (relu(NaN) is NaN) and the fused 2x2 pool (a window with a NaN is NaN), the forward contract of include/pose_mi355x.h, at both
    block widths."""
    for relu, pool in ((0, 0), (1, 0), (0, 1), (1, 1)):
        case = (ks, 32, 64, relu, pool, 2, 12, 36)
        x, Wt, b = _layer_data(case)
        x[0, 3, 4, 5] = np.nan
        x[0, 17, 5, 18] = np.inf
        x[1, 8, 6, 30] = -np.inf
        ref = E.conv_f16(x, Wt, b, relu, pool)
        nan = np.isnan(ref)
        win = np.zeros((12, 36), bool)                       # the outputs whose window holds the NaN, pooled: any of the four
        win[max(0, 4 - ks // 2):4 + ks // 2 + 1, max(0, 5 - ks // 2):5 + ks // 2 + 1] = True
        if pool:
            win = win.reshape(6, 2, 18, 2).any(axis=(1, 3))
        assert win.sum() == (ks * ks if not pool else {3: 4, 7: 16}[ks])
        assert np.array_equal(nan[0], np.broadcast_to(win, nan[0].shape)) and not nan[1].any() and not np.isinf(ref).any()
        for bn in (64, 128):
            y = _with_f16(engine, bn, lambda: engine.conv2d(x, Wt, b, relu=bool(relu), pool=bool(pool)))
            assert np.array_equal(np.isnan(y), nan), (relu, pool, bn, int(np.isnan(y).sum()), int(nan.sum()))
            assert not np.isinf(y).any()
            tol = 2e-5 * max(1.0, float(np.abs(ref[~nan]).max()))
            assert float(np.abs(y[~nan] - ref[~nan]).max()) <= tol, (relu, pool, bn)
        # one NaN weight (centre tap: no output's window leaves it to the padding): exactly that output channel is NaN
        x, Wt, b = _layer_data(case)
        Wt[37, 5, ks // 2, ks // 2] = np.nan
        ref = E.conv_f16(x, Wt, b, relu, pool)
        nan = np.zeros(ref.shape, bool)
        nan[:, 37] = True
        assert np.array_equal(np.isnan(ref), nan)
        for bn in (0, 64, 128) if relu or pool else (0,):
            y = _with_f16(engine, bn, lambda: engine.conv2d(x, Wt, b, relu=bool(relu), pool=bool(pool)))
            assert np.array_equal(np.isnan(y), nan) and not np.isinf(y).any(), (relu, pool, bn)
            assert float(np.abs(y[~nan] - ref[~nan]).max()) <= 2e-5 * max(1.0, float(np.abs(ref[~nan]).max()))


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
