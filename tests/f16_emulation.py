"""CPU emulation of the f16 inference mode's arithmetic contract (engine option "precision" = 2, include/pose_mi355x.h).  Helper of
tests/test_f16_host.py and tests/test_gpu_f16.py, not collected itself.

Per output of a 3x3 / 7x7 layer: sum over (tap, input channel) of f16(x) * f16(w), where f16() is round-to-nearest-even saturating at
+-65504 -- every product of two f16 values is exact in fp32 and in float64 -- then the fp32 epilogue: 2x2 max-pool of the sums, + bias,
ReLU.  The GPU sums in fp32 in its own fixed order; the emulation sums in float64 (acc='f64') and rounds once, so the two differ by
fp32 summation noise only.  acc='f32' sums the same rounded operands in fp32 (torch CPU order): the pair ('f64', 'f32') measures how far
that noise travels through the network.  The 1x1 layers stay fp32.  Activations are stored as fp32 between layers.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import network_ref

F16_MAX = 65504.0


def f16_round(x):
    """f16(x) as float32: round-to-nearest-even, saturating at +-65504 (NaN stays NaN)."""
    x = np.asarray(x, dtype=np.float32)
    return np.clip(x, -F16_MAX, F16_MAX).astype(np.float16).astype(np.float32)


def conv_f16(x, W, b, relu=False, pool=False, acc='f64', rounded=True):
    """One layer of the f16 mode on NCHW float32 x, OIHW W.  rounded=False: the same epilogue on the unrounded operands (the plain
    fp32 reference of the negative controls)."""
    xr = f16_round(x) if rounded else np.asarray(x, dtype=np.float32)
    wr = f16_round(W) if rounded else np.asarray(W, dtype=np.float32)
    dt = torch.float64 if acc == 'f64' else torch.float32
    with torch.no_grad():
        s = F.conv2d(torch.from_numpy(np.ascontiguousarray(xr)).to(dt), torch.from_numpy(np.ascontiguousarray(wr)).to(dt),
                     padding=W.shape[-1] // 2)
        s = s.to(torch.float32)
        if pool:
            s = F.max_pool2d(s, 2, 2)
        if b is not None:
            s = s + torch.from_numpy(np.asarray(b, dtype=np.float32)).view(1, -1, 1, 1)
        if relu:
            s = F.relu(s)
    return s.numpy()


def conv_f32(x, W, b, relu=False, pool=False):
    """A 1x1 layer (fp32 in the f16 mode): float64 sum rounded once, fp32 epilogue."""
    return conv_f16(x, W, b, relu, pool, acc='f64', rounded=False)


def forward_f16(weights, x, acc='f64'):
    """posenet (oracle/network_ref.layer_table(), the forward of network_ref.forward) in the f16 mode: (paf, heat) of the last stage."""
    ks = {name: k for name, _, _, k in network_ref.layer_table()}

    def conv(name, h, relu=True, pool=False):
        W, b = weights[name]
        if ks[name] == 1:
            return conv_f32(h, W, b, relu, pool)
        return conv_f16(h, W, b, relu, pool, acc=acc)

    h = conv('conv1_1', np.asarray(x, dtype=np.float32))
    h = conv('conv1_2', h, pool=True)
    h = conv('conv2_1', h)
    h = conv('conv2_2', h, pool=True)
    h = conv('conv3_1', h); h = conv('conv3_2', h); h = conv('conv3_3', h)
    h = conv('conv3_4', h, pool=True)
    h = conv('conv4_1', h); h = conv('conv4_2', h); h = conv('conv4_3_CPM', h); h = conv('conv4_4_CPM', h)
    feat = h
    h1, h2 = feat, feat
    for i in range(1, 5):
        h1 = conv('conv5_%d_CPM_L1' % i, h1)
        h2 = conv('conv5_%d_CPM_L2' % i, h2)
    h1 = conv('conv5_5_CPM_L1', h1, relu=False)
    h2 = conv('conv5_5_CPM_L2', h2, relu=False)
    for s in range(2, 7):
        hc = np.concatenate((h1, h2, feat), axis=1)
        h1, h2 = hc, hc
        for i in range(1, 7):
            h1 = conv('Mconv%d_stage%d_L1' % (i, s), h1)
            h2 = conv('Mconv%d_stage%d_L2' % (i, s), h2)
        h1 = conv('Mconv7_stage%d_L1' % s, h1, relu=False)
        h2 = conv('Mconv7_stage%d_L2' % s, h2, relu=False)
    return h1, h2


def rel_err(a, b):
    """max |a - b| relative to max(1, max |b|) (the suite's network-map measure)."""
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(1.0, float(np.abs(b).max())))
