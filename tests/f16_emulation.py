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


def lattice_case(kind, ks, cin, seed, cout=128, B=2, H=10, W=18):
    """(x, W, b) on which every fp32 summation order of the f16 mode is exact, so that a kernel must EQUAL conv_f16.
    'a': x = k * 2^-24, integer |k| <= 1023 -- every nonzero activation an f16 subnormal -- and W = m * 2^8, integer |m| <= 4.
    'b': the roles swapped, and the weights unrounded: half of them at ties, (k + 1/2) * 2^-24, and a few below the smallest f16
    subnormal's half: 2^-25 (the tie to zero), its float32 successor (rounds up to 2^-24) and -2^-26 (rounds to -0).
    'c': 'a' with the unrounded small values of 'b' as the activations (the device's conversion at subnormal ties).
    After f16() every operand is q * 2^-24, |q| <= 1023, or m * 2^8: a product is an integer multiple of 2^-16 of at most
    1023 * 4 * 2^-16, and a sum of the cin * ks * ks <= 48 * 49 of them stays below 147; with a bias that is a multiple of 2^-16 of at
    most 1 every partial result is a multiple of 2^-16 below 2^8 = 2^-16 * 2^24: representable in fp32, so no addition rounds.
    'd': the device's conversion at ties of normal numbers: x = +-(1 + (2 j + 1) * 2^-11), halfway between two f16 values of [1, 2], and
    W = m, integer |m| <= 2.  f16(x) is a multiple of 2^-10 of at most 2, a sum stays below 48 * 49 * 2 * 2 = 9408, the bias is a
    multiple of 2^-10 of at most 1: multiples of 2^-10 below 2^14 = 2^-10 * 2^24, exact again."""
    rng = np.random.default_rng(seed)
    xs, ws = (B, cin, H, W), (cout, cin, ks, ks)
    if kind == 'd':
        x = ((1 + (2 * rng.integers(0, 1024, xs) + 1) * 2.0 ** -11) * rng.choice([-1.0, 1.0], xs)).astype(np.float32)
        Wt = rng.integers(-2, 3, ws).astype(np.float32)
        return x, Wt, (rng.integers(-1024, 1025, cout) * 2.0 ** -10).astype(np.float32)
    sub = (rng.integers(-1023, 1024, xs if kind in 'ac' else ws) * 2.0 ** -24).astype(np.float32)
    big = (rng.integers(-4, 5, ws if kind in 'ac' else xs) * 2.0 ** 8).astype(np.float32)
    if kind != 'a':
        ties = rng.random(sub.shape) < 0.5
        ties &= sub < np.float32(1023 * 2.0 ** -24)                     # (so that a tie never rounds past 1023 * 2^-24)
        sub = np.where(ties, sub + np.float32(2.0 ** -25), sub).astype(np.float32)
        flat = sub.reshape(-1)
        at = rng.choice(flat.size, 12, replace=False)
        flat[at[0:4]] = np.float32(2.0 ** -25)
        flat[at[4:8]] = np.nextafter(np.float32(2.0 ** -25), np.float32(1))
        flat[at[8:12]] = np.float32(-2.0 ** -26)
    x, Wt = (sub, big) if kind in 'ac' else (big, sub)
    b = np.zeros(cout, np.float32) if cin == 16 else (rng.integers(-65536, 65537, cout) * 2.0 ** -16).astype(np.float32)
    return x, Wt, b


def rel_err(a, b):
    """max |a - b| relative to max(1, max |b|) (the suite's network-map measure)."""
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(1.0, float(np.abs(b).max())))
