"""GPU: the loss sum, its gradient and the targets of csrc/pmx_loss.hip at launches past one pass of the capped grid.  loss_stage_kernel runs
at most PMX_LOSS_MAX_BLOCKS = 256 blocks of 256 threads, so one pass covers 65 536 elements = 1 149 map pixels of 57 channels; a thread
then walks on by gridDim.x * 256, and loss_final_kernel adds 256 partials.  Every other loss test stays below 192 map pixels.  The shapes
here are the smallest that reach the later passes: 25 x 24 map pixels (200 x 192) at B = 2 (68 400 elements: some threads make two
passes) and B = 3 (102 600), and 24 x 24 (192 x 192) at B = 4 (131 328: two full passes and exactly one block on a third).

Reference: tests/loss_ref.py::stage_loss (float64 sum of float32 differences) on the maps and targets the library itself returns; the
targets are first compared with loss_ref.targets of loss_ref.labels.  Bound of a loss: a float64 sum of N non-negative terms in any
order is within N * 2**-52 of the exact sum, relatively (the bound of tests/test_gpu_validation_loss.py), N = elements of the branch."""
import numpy as np
import pytest

import conv_bwd_ref as R
import loss_ref
from conftest import pkg
from oracle import fixtures

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
EPS = 2.0 ** -52
SHAPES = [(2, 200, 192), (3, 200, 192), (4, 192, 192)]
ONE_PASS = 256 * 256          # PMX_LOSS_MAX_BLOCKS (csrc/pmx_ctx.h) blocks of 256 threads: the profile list does not carry the grid
PEOPLE = (3, 0, 7, 1)
MASK_KINDS = ('none', 'half', 'sparse', 'all_but_one')


def _rel(a, b):
    return abs(a - b) / b if b else abs(a)


def _mask(kind, h, w, seed):
    m = np.zeros((h, w), bool)
    if kind == 'half':
        m[:, :w // 2] = True
    elif kind == 'sparse':
        m.reshape(-1)[np.random.default_rng(seed).choice(h * w, round(0.01 * h * w), replace=False)] = True
    elif kind == 'all_but_one':
        m[:] = True
        m[0, 0] = False          # map pixel (0, 0) reads pixel (0, 0) with weight 1: the one map pixel that stays
    elif kind == 'all':
        m[:] = True
    return m


def _inputs(B, H, W):
    """per image other people, another mask and maps of another scale; per channel another scale"""
    rng = np.random.default_rng(100 * B + H)
    poses = [fixtures.random_poses(rng, PEOPLE[b], H, W, drop_prob=0.05) for b in range(B)]
    masks = np.stack([_mask(MASK_KINDS[b], H, W, 31 + b) for b in range(B)])
    fh, fw = H // 8, W // 8
    img_scale = (1 + 0.37 * np.arange(B))[:, None, None, None]
    yp = (rng.normal(size=(B, 38, fh, fw)) * img_scale * (0.3 + 0.05 * np.arange(38))[None, :, None, None]).astype(np.float32)
    yh = (rng.normal(size=(B, 19, fh, fw)) * img_scale * (0.2 + 0.03 * np.arange(19))[None, :, None, None]).astype(np.float32)
    return poses, masks, yp, yh


def _ref_targets(poses, masks, H, W):
    t = [loss_ref.targets(*loss_ref.labels((H, W), p), mask=m) for p, m in zip(poses, masks)]
    return tuple(np.stack([a[i] for a in t]) for i in range(3))


@pytest.fixture(scope='module')
def eng(native):
    e = native.Engine(0, max_batch=4, max_h=200, max_w=192)
    e.set_weights(pkg('weights').synthetic_weights(0))
    yield e
    e.close()


@pytest.fixture(scope='module')
def images():
    return np.random.default_rng(77).integers(0, 256, (4, 200, 192, 3), dtype=np.uint8)


@pytest.mark.parametrize('B,H,W', SHAPES)
def test_targets_and_loss_of_given_maps_past_one_pass(eng, B, H, W):
    fh, fw = H // 8, W // 8
    assert B * fh * fw * 57 > ONE_PASS          # the stage launch is capped at PMX_LOSS_MAX_BLOCKS blocks and walks on
    poses, masks, yp, yh = _inputs(B, H, W)
    eng.loss_set_poses(poses, H, W, masks)
    tp, th, tm = eng.loss_targets()
    want_p, want_h, want_m = _ref_targets(poses, masks, H, W)
    dp, dh = np.abs(tp - want_p).max(), np.abs(th - want_h).max()
    print(B, H, W, 'targets: paf %.3g heat %.3g ulp' % (dp / ULP, dh / ULP))
    assert dp <= ULP and dh <= ULP and np.array_equal(tm, want_m)
    assert np.array_equal(tp != 0, want_p != 0)
    assert not tm[0].any() and tm[1].any() and not tm[1].all()
    # block 255, the last of the capped grid, sums live elements on its first pass: a final sum over 255 partials would show
    assert not tm.reshape(-1)[(ONE_PASS - 256) // 57:(ONE_PASS - 1) // 57 + 1].any()
    if B == 4:
        assert tm[3].sum() == fh * fw - 1 and not tm[3, 0, 0]
    eng.set_maps(yp, yh)                        # the external planar layout of LossSrc
    lp, lh = eng.loss_current_maps()
    rp, rh = loss_ref.stage_loss(yp, yh, tp, th, tm)
    print(B, H, W, 'loss: paf %.17g %.17g (%.3g N eps) heat %.17g %.17g (%.3g N eps)'
          % (lp, rp, _rel(lp, rp) / (yp.size * EPS), lh, rh, _rel(lh, rh) / (yh.size * EPS)))
    assert rp > 0 and rh > 0
    assert _rel(lp, rp) <= yp.size * EPS and _rel(lh, rh) <= yh.size * EPS
    assert eng.loss_current_maps() == (lp, lh)          # the same bits on a second run
    # an all-ignored image contributes exactly 0: image k ignored = the reference with that image's differences dropped ...
    for k in (0, B - 1):
        mk = masks.copy()
        mk[k] = True
        eng.loss_set_poses(poses, H, W, mk)
        tmk = eng.loss_targets()[2]
        assert tmk[k].all() and np.array_equal(np.delete(tmk, k, 0), np.delete(tm, k, 0))
        lpk, lhk = eng.loss_current_maps()
        rpk, rhk = loss_ref.stage_loss(yp, yh, tp, th, tmk)
        assert _rel(lpk, rpk) <= yp.size * EPS and _rel(lhk, rhk) <= yh.size * EPS
        assert lpk < lp and lhk < lh
    # ... and all of them ignored is 0.0
    eng.loss_set_poses(poses, H, W, np.ones_like(masks))
    assert eng.loss_current_maps() == (0.0, 0.0)


@pytest.fixture(scope='module')
def run2(eng, images):
    """ONE hooked forward of B = 2 at 200 x 192 with the gradients on -> losses, maps, the gradients of the six stages, the targets"""
    B, H, W = SHAPES[0]
    poses, masks, _, _ = _inputs(B, H, W)
    eng.loss_set_poses(poses, H, W, masks)
    eng.loss_grad_enable(True)
    try:
        total, paf, heat = eng.validate_batch(images[:B])
        maps = eng.get_maps()
        current = eng.loss_current_maps()          # the NHWC cat buffer through the other entry
        grads = [eng.loss_grads(s) for s in range(6)]
        again = eng.validate_batch(images[:B])
    finally:
        eng.loss_grad_enable(False)
    return dict(total=total, paf=paf, heat=heat, maps=maps, current=current, grads=grads, again=again, targets=eng.loss_targets())


def test_validate_batch_past_one_pass(run2):
    B, H, W = SHAPES[0]
    yp, yh = run2['maps']
    assert yp.shape == (B, 38, H // 8, W // 8) and yp.size + yh.size > ONE_PASS
    tp, th, tm = run2['targets']
    rp, rh = loss_ref.stage_loss(yp, yh, tp, th, tm)
    lp, lh = run2['paf'][5], run2['heat'][5]
    print('stage 6: paf %.17g %.17g (%.3g N eps) heat %.17g %.17g (%.3g N eps)'
          % (lp, rp, _rel(lp, rp) / (yp.size * EPS), lh, rh, _rel(lh, rh) / (yh.size * EPS)))
    assert rp > 0 and rh > 0
    assert _rel(lp, rp) <= yp.size * EPS and _rel(lh, rh) <= yh.size * EPS
    assert run2['current'] == (lp, lh)              # the same launch over the same buffer
    again = run2['again']
    assert again[0] == run2['total'] and np.array_equal(again[1], run2['paf']) and np.array_equal(again[2], run2['heat'])
    assert run2['paf'].all() and run2['heat'].all() and len(set(run2['paf'])) == 6


@pytest.mark.parametrize('s', [1, 2, 3, 4, 5, 6])
def test_stage_gradient_past_one_pass_is_the_formula_bit_for_bit(eng, images, run2, s):
    B, H, W = SHAPES[0]
    tp, th, tm = run2['targets']
    assert tm[1].any() and not tm[1].all() and not tm[0].any()
    assert not tm.reshape(-1)[(ONE_PASS - 256) // 57:(ONE_PASS - 1) // 57 + 1].any()          # the last block's elements are live
    eng.set_option('stop_stage', s)
    try:
        eng.forward_u8(images[:B])
        yp, yh = eng.get_maps()
    finally:
        eng.set_option('stop_stage', 6)
    gp, gh = run2['grads'][s - 1]
    assert gp.shape == (B, 38, H // 8, W // 8) and gh.shape == (B, 19, H // 8, W // 8)
    assert np.array_equal(gp.view(np.uint32), R.loss_grad_formula(yp, tp, tm, B).view(np.uint32))
    assert np.array_equal(gh.view(np.uint32), R.loss_grad_formula(yh, th, tm, B).view(np.uint32))
    for g in (gp, gh):                              # +0.0f exactly where the resized mask is set
        sel = np.broadcast_to(tm[:, None], g.shape)
        assert not g.view(np.uint32)[sel].any()
        assert g[~sel].any()
    # the stage's loss against the reference on the same maps
    rp, rh = loss_ref.stage_loss(yp, yh, tp, th, tm)
    assert _rel(run2['paf'][s - 1], rp) <= yp.size * EPS and _rel(run2['heat'][s - 1], rh) <= yh.size * EPS


def test_batch_loss_is_the_mean_of_the_per_image_losses(eng, images):
    """B = 4 at 192 x 192 in one capped launch (NHWC, three passes) against each image alone at B = 1 (planar, 129 blocks, one pass): each
    is within N * 2**-52 of its exact sum, so the mean of the four and the batch value differ by at most 4 * N * 2**-52, N of the batch"""
    B, H, W = SHAPES[2]
    poses, masks, _, _ = _inputs(B, H, W)
    masks[3] = _mask('sparse', H, W, 5)             # all-but-one would leave image 3 a single live map pixel
    eng.loss_set_poses(poses, H, W, masks)
    _, paf, heat = eng.validate_batch(images[:, :H])
    yp, yh = eng.get_maps()
    assert yp.size + yh.size > 2 * ONE_PASS and yp[0].size + yh[0].size <= ONE_PASS
    tp, th, tm = eng.loss_targets()
    rp, rh = loss_ref.stage_loss(yp, yh, tp, th, tm)
    assert _rel(paf[5], rp) <= yp.size * EPS and _rel(heat[5], rh) <= yh.size * EPS
    single = []
    for b in range(B):
        eng.loss_set_poses(poses[b:b + 1], H, W, masks[b:b + 1])
        t1 = eng.loss_targets()
        assert all(np.array_equal(a[0], t[b]) for a, t in zip(t1, (tp, th, tm)))
        eng.set_maps(yp[b:b + 1], yh[b:b + 1])
        single.append(eng.loss_current_maps())
    mp, mh = np.mean([s[0] for s in single]), np.mean([s[1] for s in single])
    print('batch of 4: paf %.17g mean %.17g (%.3g N eps) heat %.17g mean %.17g (%.3g N eps)'
          % (paf[5], mp, _rel(mp, paf[5]) / (yp.size * EPS), heat[5], mh, _rel(mh, heat[5]) / (yh.size * EPS)))
    assert len(set(s[0] for s in single)) == 4
    assert _rel(mp, paf[5]) <= 4 * yp.size * EPS and _rel(mh, heat[5]) <= 4 * yh.size * EPS
