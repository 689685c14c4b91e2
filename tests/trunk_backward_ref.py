"""Host references of the trunk backward (include/pose_mi355x.h: pmx_backward_trunk), shared by the host and the GPU tests: the trunk's graph,
the strip rules restated, the order-defined twin of a weight gradient for given (strips, rows) and the pooled layers' rule in NumPy."""
import ctypes as C

import numpy as np

import conv_bwd_ref as R

# name, cin, cout, resolution level, pooled afterwards -- conv1_1 .. conv4_2 (CocoPoseNet.py:136-149)
TRUNK = [('conv1_1', 3, 64, 0, False), ('conv1_2', 64, 64, 0, True), ('conv2_1', 64, 128, 1, False), ('conv2_2', 128, 128, 1, True),
         ('conv3_1', 128, 256, 2, False), ('conv3_2', 256, 256, 2, False), ('conv3_3', 256, 256, 2, False), ('conv3_4', 256, 256, 2, True),
         ('conv4_1', 256, 512, 3, False), ('conv4_2', 512, 512, 3, False)]
NAMES = [t[0] for t in TRUNK]
POOLED = [t[0] for t in TRUNK if t[4]]
WAVES, TRUNK_MAX_STRIPS, CONV1_STRIPS = 2048, 512, 2048


def _cut(total, s0, cap):
    """rows rounded DOWN: s0 <= S < 2 s0"""
    s0 = max(1, min(s0, cap, total))
    r = total // s0
    return -(-total // r), r


def units(cin, cout):
    """waves of one strip of the generic 3x3 kernel: (tap row, 32 co, 2 x 32 ci)"""
    return -(-(-(-cin // 32)) // 2) * 3 * -(-cout // 32)


def trunk_strips(name, B, H, forced=0):
    """(strips, rows, waves) of a trunk layer's weight gradient for a batch of B images of network-input height H"""
    _, cin, cout, level, _ = TRUNK[NAMES.index(name)]
    if name == 'conv1_1':
        s, r = _cut(B * H, forced if forced > 0 else CONV1_STRIPS, CONV1_STRIPS)
        return s, r, s
    u = units(cin, cout)
    s, r = _cut(B * (H >> level), forced if forced > 0 else -(-WAVES // u), TRUNK_MAX_STRIPS)
    return s, r, s * u


def wgrad_twin(g, x, strips, rows):
    """tests/conv_wgrad_twin.c for GIVEN (strips, rows): dw (cout, cin, 3, 3) float32"""
    g = np.ascontiguousarray(g, dtype=np.float32)
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, cout, H, W = g.shape
    cin = x.shape[1]
    assert x.shape == (B, cin, H, W) and (strips - 1) * rows < B * H <= strips * rows
    dw = np.empty((cout, cin, 3, 3), np.float32)
    R.twin_lib().conv_wgrad_twin(g.ctypes.data, x.ctypes.data, B, H, W, cout, cin, 3, int(strips), int(rows), dw.ctypes.data)
    return dw


def pool_twin(a, u):
    """(pooled, g) of the pooled layers from the post-ReLU, pre-pool output a (B, C, H, W) and the gradient u at the pooled map: the 2 x 2
    maximum; u at the FIRST maximum of each window in the order (0,0), (0,1), (1,0), (1,1) where that a > 0, +0.0 elsewhere."""
    a = np.asarray(a, dtype=np.float32)
    u = np.asarray(u, dtype=np.float32)
    B, c, H, W = a.shape
    win = a.reshape(B, c, H // 2, 2, W // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(B, c, H // 2, W // 2, 4)
    first = np.argmax(win, axis=-1)
    pooled = win.max(axis=-1)
    sel = np.zeros(win.shape, bool)
    np.put_along_axis(sel, first[..., None], True, axis=-1)
    g = np.where(sel & (win > 0), u[..., None], np.float32(0)).astype(np.float32)
    g = g.reshape(B, c, H // 2, W // 2, 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(B, c, H, W)
    return np.ascontiguousarray(pooled), np.ascontiguousarray(g)


def pool_scatter(a, u):
    """pool_twin's g in the dtype of u (a float64 dx is scattered by the same rule as the float32 one): u at the FIRST maximum of each
    2 x 2 window of a where that a > 0, +0.0 elsewhere."""
    a = np.asarray(a, dtype=np.float32)
    u = np.asarray(u)
    B, c, H, W = a.shape
    assert u.shape == (B, c, H // 2, W // 2)
    win = windows(a)
    sel = np.zeros(win.shape, bool)
    np.put_along_axis(sel, np.argmax(win, axis=-1)[..., None], True, axis=-1)
    g = np.where(sel & (win > 0), u[..., None], u.dtype.type(0))
    return np.ascontiguousarray(g.reshape(B, c, H // 2, W // 2, 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(B, c, H, W))


def windows(a):
    B, c, H, W = a.shape
    return a.reshape(B, c, H // 2, 2, W // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(B, c, H // 2, W // 2, 4)


# ---- lattice inputs of the pool kernels' test entry --------------------------------------------------------------------------------------
POOL_CASES = [(C_, H, W) for C_ in (32, 64, 96) for (H, W) in ((2, 2), (6, 10), (16, 12))]
POOL_SEED = 11          # fixed: every census class is present in every case (asserted where the inputs are made)


def pool_lattice(C_, H, W):
    """(z, a, u, census): z = the output of a 1x1 convolution of R.lattice_inputs (4 -> C_ channels, batch 2, in float64: exact on the lattice),
    a = relu(z), u the gradient at the pooled map, census = R.lattice_census(z, u, relu = 1, pool = 1)."""
    x, w, b, u = R.lattice_inputs(1, 4, C_, H, W, 2, 1, POOL_SEED + C_ + H)
    z = np.einsum('bihw,oi->bohw', x.astype(np.float64), w[:, :, 0, 0].astype(np.float64)) + b.astype(np.float64)[None, :, None, None]
    z32 = z.astype(np.float32)
    assert np.array_equal(z32.astype(np.float64), z)
    return z32, np.maximum(z32, np.float32(0)), u, R.lattice_census(z, u, 1, 1)
