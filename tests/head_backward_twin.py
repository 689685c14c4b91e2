"""NumPy twins of what the head backward (include/pose_mi355x.h: pmx_backward_head) documents besides the per-layer gradients: the channel
map between the concat buffer and the reference's F.concat((h1, h2, feature_map)), and the three sums, each a float32 add, left to right."""
import numpy as np

CAT_C, CAT_FEAT, CAT_PAF, CAT_HEAT = 192, 0, 128, 168          # csrc/pmx_common.h
N_PAF, N_HEAT, N_FEAT = 38, 19, 128
REF_C = N_PAF + N_HEAT + N_FEAT


def cat_of_ref():
    """(185,) the concat-buffer channel that holds the reference's input channel r of Mconv1_*: 38 PAF, 19 heat, 128 feature"""
    return np.concatenate([CAT_PAF + np.arange(N_PAF), CAT_HEAT + np.arange(N_HEAT), CAT_FEAT + np.arange(N_FEAT)])


def ref_of_cat():
    """(192,) the reference channel a concat-buffer channel holds, -1 for the pad channels (csrc/pack_index.h::pmx_pk_ref_of_packed, kind 1)"""
    m = np.full(CAT_C, -1)
    m[cat_of_ref()] = np.arange(REF_C)
    return m


def to_ref(a_cat, axis=1):
    """concat-buffer order -> the reference's order along `axis`: the pad channels are dropped"""
    return np.take(a_cat, cat_of_ref(), axis=axis)


def to_cat(a_ref, axis=1):
    """the reference's order -> concat-buffer order along `axis`, zeros in the pad channels"""
    a_ref = np.asarray(a_ref)
    shape = list(a_ref.shape)
    shape[axis] = CAT_C
    out = np.zeros(shape, a_ref.dtype)
    idx = [slice(None)] * a_ref.ndim
    idx[axis] = cat_of_ref()
    out[tuple(idx)] = a_ref
    return out


def flip_weights_cat(w):
    """OIHW (cout, 185, k, k) -> (192, cout, k, k): the transposed, 180-degree-rotated layer with its output channels in concat-buffer order,
    zero rows for the pad channels (tests/conv_bwd_pack.h::pmx_conv_flip_weights_mapped)"""
    import conv_bwd_ref as R
    return np.ascontiguousarray(to_cat(R.flip_weights(w), axis=0))


def _f32(a):
    return np.asarray(a, dtype=np.float32)


def stage_sum(loss_grad, dx_l1=None, dx_l2=None):
    """u at a stage's PAF or heat output: loss_grad, then + dx(Mconv1_stage{s+1}_L1), then + dx(..._L2); the last stage: loss_grad alone"""
    u = _f32(loss_grad)
    if dx_l1 is None:
        assert dx_l2 is None
        return u.copy()
    u = (u + _f32(dx_l1)).astype(np.float32)
    return (u + _f32(dx_l2)).astype(np.float32)


def feature_order(n_stages):
    """the layers whose data gradients reach the feature map, in the order the backward produces them"""
    names = []
    for s in range(n_stages, 1, -1):
        names += ['Mconv1_stage%d_L1' % s, 'Mconv1_stage%d_L2' % s]
    return names + ['conv5_1_CPM_L1', 'conv5_1_CPM_L2']


def feature_sum(contributions):
    """u at conv4_4_CPM's output: the first contribution, then + each of the rest in feature_order"""
    u = _f32(contributions[0]).copy()
    for c in contributions[1:]:
        u = (u + _f32(c)).astype(np.float32)
    return u


def chain_sum(dx_next):
    """inside a stage: u is the next layer's dx"""
    return _f32(dx_next).copy()
