"""GPU: the gradient of compute_loss at the twelve stage outputs (include/pose_mi355x.h: pmx_loss_grad_enable / pmx_get_loss_grads) against
the NumPy formula tests/conv_bwd_ref.py::loss_grad_formula applied to the maps and targets the library itself returns."""
import numpy as np
import pytest

import conv_bwd_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu

H, W, B = 64, 48, 2


@pytest.fixture(scope='module')
def eng(native):
    e = native.Engine(0, max_batch=B, max_h=H, max_w=W)
    e.set_weights(pkg('weights').synthetic_weights(0))
    yield e
    e.close()


@pytest.fixture(scope='module')
def data():
    rng = np.random.default_rng(2024)
    imgs = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    poses = []
    for n in (2, 1):
        p = np.zeros((n, 18, 3))
        p[:, :, 0] = rng.uniform(2, W - 2, (n, 18))
        p[:, :, 1] = rng.uniform(2, H - 2, (n, 18))
        p[:, :, 2] = rng.integers(0, 3, (n, 18))
        poses.append(p)
    masks = np.zeros((B, H, W), bool)
    masks[1, 10:40, 8:30] = True          # a non-trivial ignore mask on one image
    return imgs, poses, masks


@pytest.fixture(scope='module')
def run(eng, data):
    """ONE hooked forward with the gradients on -> its losses, maps, gradients of all six stages, and the targets (computed once)."""
    imgs, poses, masks = data
    eng.loss_set_poses(poses, H, W, masks, 7, 8)
    eng.loss_grad_enable(True)
    try:
        total, paf, heat = eng.validate_batch(imgs)
        maps = eng.get_maps()
        grads = [eng.loss_grads(s) for s in range(6)]
    finally:
        eng.loss_grad_enable(False)
    return dict(total=total, paf=paf, heat=heat, maps=maps, grads=grads, targets=eng.loss_targets())


@pytest.mark.parametrize('s', [1, 2, 3, 4, 5, 6])
def test_stage_gradient_is_the_formula_bit_for_bit(eng, data, run, s):
    imgs, _, _ = data
    t_p, t_h, t_m = run['targets']
    assert t_m[1].any() and not t_m[1].all() and not t_m[0].any()
    eng.set_option('stop_stage', s)
    try:
        eng.forward_u8(imgs)
        yp, yh = eng.get_maps()
    finally:
        eng.set_option('stop_stage', 6)
    gp, gh = run['grads'][s - 1]
    assert gp.shape == (B, 38, H // 8, W // 8) and gh.shape == (B, 19, H // 8, W // 8)
    assert np.array_equal(gp.view(np.uint32), R.loss_grad_formula(yp, t_p, t_m, B).view(np.uint32))
    assert np.array_equal(gh.view(np.uint32), R.loss_grad_formula(yh, t_h, t_m, B).view(np.uint32))
    # +0.0f exactly where the resized mask is set
    for g in (gp, gh):
        sel = np.broadcast_to(t_m[:, None], g.shape)
        assert not g.view(np.uint32)[sel].any()
        assert g[~sel].any()
    # N / 4 * sum g^2 is the stage's loss: c and the product are each one float32 rounding, so g^2 is within 4 * 2^-24
    for g, loss in ((gp, run['paf'][s - 1]), (gh, run['heat'][s - 1])):
        back = g.size / 4.0 * np.sum(g.astype(np.float64) ** 2)
        print('stage', s, 'loss', loss, 'from the gradient', back)
        assert abs(back - loss) <= 4 * 2.0 ** -24 * loss


def test_maps_and_losses_keep_their_bits_with_the_gradients_on(eng, data, run):
    imgs, _, _ = data
    total, paf, heat = eng.validate_batch(imgs)          # gradients off
    maps = eng.get_maps()
    assert total == run['total'] and np.array_equal(paf, run['paf']) and np.array_equal(heat, run['heat'])
    assert np.array_equal(maps[0], run['maps'][0]) and np.array_equal(maps[1], run['maps'][1])


def test_call_sequence_errors(native, eng, data, run):
    imgs, _, _ = data
    with pytest.raises(native.PmxError) as e:           # off
        eng.loss_grads(0)
    assert e.value.code == 6 and 'pmx_loss_grad_enable' in str(e.value)
    eng.loss_grad_enable(True)
    try:
        with pytest.raises(native.PmxError) as e:       # on, but no hooked forward since
            eng.loss_grads(0)
        assert e.value.code == 6
        eng.forward_u8(imgs)                            # not hooked
        with pytest.raises(native.PmxError) as e:
            eng.loss_grads(0)
        assert e.value.code == 6
        for stage in (-1, 6):
            with pytest.raises(native.PmxError) as e:
                eng.loss_grads(stage)
            assert e.value.code == 1 and 'outside 0..5' in str(e.value)
        eng.set_option('stop_stage', 2)
        try:
            eng.validate_batch(imgs)
        finally:
            eng.set_option('stop_stage', 6)
        assert np.array_equal(eng.loss_grads(1)[0], run['grads'][1][0])
        with pytest.raises(native.PmxError) as e:
            eng.loss_grads(2)
        assert e.value.code == 6 and 'stop_stage' in str(e.value)
    finally:
        eng.loss_grad_enable(False)


def test_pose_detector_loss_gradients(native, data, run):
    PD = pkg('pose_detector')
    imgs, poses, masks = data
    det = PD.PoseDetector(weights=pkg('weights').synthetic_weights(0), device=0, max_batch=B, max_size=(H, W))
    out = det.loss_gradients(list(imgs), poses, list(masks))
    ref = det.validation_loss(list(imgs), poses, list(masks))
    for key in ('val/loss', 'val/paf', 'val/heat', 'paf_stages', 'heat_stages'):
        assert out[key] == ref[key], key
    assert out['val/loss'] == run['total']
    assert len(out['paf_grads']) == 6 and len(out['heat_grads']) == 6
    for s in range(6):
        assert np.array_equal(out['paf_grads'][s], run['grads'][s][0]) and np.array_equal(out['heat_grads'][s], run['grads'][s][1])
    with pytest.raises(ValueError):
        det.loss_gradients(list(imgs) * 2, poses * 2, list(masks) * 2)          # more than max_batch images
    with pytest.raises(ValueError):
        det.loss_gradients([], [], None)
