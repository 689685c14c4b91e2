"""GPU: the training steps on f16 head gradients with a static loss scale (include/pose_mi355x.h: options "grad_precision" and
"loss_scale_log2", pmx_train_step_head, pmx_get_transposed_f16_pack (Engine.get_pack(name, 7)); PoseDetector.set_gradient_precision).
A step rewrites the f16 pack of every transposed layer that exists, so the next backward's data gradients come from the new weights; the
loss scale folds into Adam's per-layer scale exactly, so fp32 training under a scale is the training without it, bit for bit, head only
and with the trunk; f16 training runs, head only and with the trunk.  Batch 2 at 64 x 48."""
import numpy as np
import pytest

import test_gpu_head_backward as HB
from conftest import pkg

pytestmark = pytest.mark.gpu

CFG = HB.PRIMARY
B, H, W = CFG['B'], CFG['H'], CFG['W']
SCALES = {'conv4_3_CPM': 0.25, 'conv4_4_CPM': 0.25}
PACK_LAYERS = ('conv4_4_CPM', 'conv5_2_CPM_L2', 'Mconv1_stage3_L1', 'Mconv4_stage6_L2')
K = 10


def _weights():
    return pkg('weights').synthetic_weights(0)


def _f16_engine(native, weights):
    e = native.Engine(0, max_batch=B, max_h=H, max_w=W)
    e.set_weights(weights)
    e.set_option('grad_precision', 2)
    e.set_option('loss_scale_log2', K)
    e.loss_grad_enable(True)
    e.backward_enable(True)
    return e


def _forward_backward(eng):
    imgs, poses, masks = HB._data(**CFG)
    eng.loss_set_poses(poses, H, W, masks, 7, 8)
    eng.validate_batch(imgs)
    eng.backward_head()


def _packs(eng):
    return {nm: eng.get_pack(nm, 't_f16') for nm in PACK_LAYERS}


# ---- 8. no stale pack ----------------------------------------------------------------------------------------------------------------------------
def test_a_step_rewrites_the_f16_packs_of_the_transposed_layers(native):
    a = _f16_engine(native, _weights())
    b = None
    try:
        assert all(p is None for p in _packs(a).values())          # no f16 backward yet
        a.train_enable(True)
        for nm in a.head_layers():
            a.train_set_grad_scale(nm, SCALES.get(nm, 1.0) * 2.0 ** -K)
        _forward_backward(a)
        before = _packs(a)
        assert all(p is not None and p.any() for p in before.values())
        a.train_step_head()
        between = _packs(a)                                        # what the second iteration's data gradients read
        for nm in PACK_LAYERS:
            assert between[nm].shape == before[nm].shape and not np.array_equal(between[nm], before[nm]), nm
        _forward_backward(a)
        a.train_step_head()
        after = _packs(a)
        b = _f16_engine(native, a.get_weights())
        _forward_backward(b)
        fresh = _packs(b)
        for nm in PACK_LAYERS:
            assert after[nm].tobytes() == fresh[nm].tobytes(), nm
            assert not np.array_equal(after[nm], between[nm]), nm
    finally:
        a.close()
        if b is not None:
            b.close()


# ---- 9. the loss scale folds exactly into Adam ------------------------------------------------------------------------------------------------
def _detector(**kw):
    return pkg('pose_detector').PoseDetector(weights=_weights(), device=0, max_batch=B, max_size=(H, W), **kw)


def _batches(n):
    return [HB._data(**dict(CFG, seed=CFG['seed'] + i)) for i in range(n)]


@pytest.mark.parametrize('trunk', [False, True])
def test_fp32_training_under_a_loss_scale_is_the_training_without_it(trunk):
    """trunk: all 92 layers train (mode 2); set_trainable restarts training, and the restart folds 2^-k into the ten trunk layers' scales
    as well -- a layer left at its own scale would see gradients 256 times too large and end with other bits."""
    out = []
    for scale in (256, 1):
        det = _detector()
        try:
            det.set_gradient_precision('f32', loss_scale=scale)
            if trunk:
                det.set_trainable(trunk=True)
            losses = [det.train_step(list(imgs), poses, list(masks))['main/loss'] for imgs, poses, masks in _batches(3)]
            out.append((losses, det.get_weights(), det.optimizer_state()))
        finally:
            det.engine.close()
    (la, wa, sa), (lb, wb, sb) = out
    assert la == lb
    assert sorted(wa) == sorted(wb) and len(wa) == 92
    for nm in wa:
        for i in (0, 1):
            assert np.array_equal(wa[nm][i].view(np.uint32), wb[nm][i].view(np.uint32)), nm
    assert sorted(sa) == sorted(sb) and sum(k.endswith('/t') for k in sa) == (92 if trunk else 82)
    user = dict(SCALES, **(dict.fromkeys(pkg('native').Engine.TRUNK_LAYERS, 0.25) if trunk else {}))
    for key in sa:
        assert np.array_equal(np.asarray(sa[key]), np.asarray(sb[key])), key
        if key.endswith('/scale'):
            assert float(sa[key]) == user.get(key[:-len('/scale')], 1.0), key          # the user's, not the folded one
        if key.endswith('/t'):
            assert int(sa[key]) == 3, key
        if key.endswith('/m_W'):
            assert np.asarray(sa[key]).any(), key


# ---- 10. f16 training runs --------------------------------------------------------------------------------------------------------------------
def _five_steps(precision, loss_scale, trunk=False):
    imgs, poses, masks = HB._data(**CFG)
    det = _detector()
    try:
        det.set_gradient_precision(precision, loss_scale=loss_scale)
        if trunk:
            det.set_trainable(trunk=True)
        losses = [det.train_step(list(imgs), poses, list(masks))['main/loss'] for _ in range(5)]
        state = det.optimizer_state()
        return np.array(losses), det.get_weights(), {k[:-2]: int(v) for k, v in state.items() if k.endswith('/t')}
    finally:
        det.engine.close()


def test_five_f16_head_steps_beside_five_fp32_steps():
    """Finite and falling in both modes.  The two curves and the distance of the final weights are printed (EXPERIMENTS.md E57), not
    asserted: where a gradient is below the f16 resolution Adam's update is sign-like, so no bound on the weights can be derived; the gates
    are the per-layer contracts of tests/test_gpu_head_backward_f16.py and the two tests above."""
    l32, w32, t32 = _five_steps('f32', 1)
    l16, w16, t16 = _five_steps('f16', 1024)
    num = sum(float(((w16[nm][0].astype(np.float64) - w32[nm][0]) ** 2).sum()) for nm in t32)
    den = sum(float((w32[nm][0].astype(np.float64) ** 2).sum()) for nm in t32)
    print('fp32', ' '.join('%.8f' % v for v in l32), 'f16', ' '.join('%.8f' % v for v in l16), 'relative L2 distance of the final head weights %.3e'
          % np.sqrt(num / den))
    for losses, t in ((l32, t32), (l16, t16)):
        assert np.isfinite(losses).all() and losses[4] < losses[0]
        assert len(t) == 82 and set(t.values()) == {5}
    assert all(np.isfinite(w16[nm][0]).all() and np.isfinite(w16[nm][1]).all() for nm in w16)


def test_five_f16_steps_with_the_trunk():
    """Mode 2: the head chain in f16, the trunk chain in fp32 on the scaled trunk gradient; all 92 layers step."""
    losses, w, t = _five_steps('f16', 1024, trunk=True)
    print('f16 head + fp32 trunk', ' '.join('%.8f' % v for v in losses))
    assert np.isfinite(losses).all() and losses[4] < losses[0]
    assert len(t) == 92 and set(t.values()) == {5}
    assert all(np.isfinite(w[nm][0]).all() and np.isfinite(w[nm][1]).all() for nm in w)
