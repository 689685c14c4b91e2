"""CPU emulation of the f16 gradients of one convolution layer (engine option "grad_precision" = 2, include/pose_mi355x.h:
pmx_conv2d_backward).  Helper of tests/test_conv_backward_f16_host.py and tests/test_gpu_conv_backward_f16.py, not collected itself.

dw[co][ci][ky][kx] = sum over pixels of f16(g) * f16(x shifted by the tap), out-of-image taps zero; every product of two f16 values is
exact in fp32 and in float64.  The GPU sums in fp32 -- 16 products per MFMA in an order that belongs to the hardware, the MFMAs of a strip
one after the other, the strips left to right -- and the emulation in float64, rounding once: they differ by fp32 summation noise, which
dw_sum_bound bounds from the documented grouping (csrc/wgrad_strips.h, restated below).  dx is the f16 forward (f16_emulation.conv_f16)
of the transposed, flipped layer on g."""
import numpy as np

import conv_bwd_ref as R
from f16_emulation import conv_f16, f16_round

# ---- the strip and group rule of csrc/wgrad_strips.h (pmx_wgrad_f16_*), restated ------------------------------------------------------------
WAVES = 4096                # PMX_WGRAD_F16_WAVES
MAX_STRIPS = 32             # PMX_WGRAD_MAX_STRIPS (include/pose_mi355x.h)
GROUP = 16                  # pixels per MFMA: an image row is cut into ceil(W / 16) groups, the last one padded with zeros


def _up32(c):
    return (c + 31) // 32 * 32


def blocks(cout, cin, ks):
    """Blocks of four waves per strip: (tap row, 4 x 32 co, NCI x 32 ci), NCI = 1 / 2 for 7x7 / 3x3."""
    per = 1 if ks == 7 else 2
    return (_up32(cout) // 32 + 3) // 4 * ks * ((_up32(cin) // 32 + per - 1) // per)


def strips_for(B, H, cout, cin, ks, s0=0):
    """(S strips, R rows per strip) of B * H image rows: s0 > 0 is option "wgrad_strips", else as many strips as give WAVES waves."""
    total = B * H
    if s0 <= 0:
        waves = 4 * blocks(cout, cin, ks)
        s0 = (WAVES + waves - 1) // waves
    s0 = max(1, min(s0, MAX_STRIPS, total))
    rows = (total + s0 - 1) // s0
    return (total + rows - 1) // rows, rows


def groups(W):
    return (W + GROUP - 1) // GROUP


def mfmas_per_strip(B, H, W, cout, cin, ks, s0=0):
    """(G, S): the largest number of MFMAs one accumulator sees in a strip -- one per 16-pixel group of each of its R rows -- and S."""
    S, rows = strips_for(B, H, cout, cin, ks, s0)
    return rows * groups(W), S


# ---- the arithmetic --------------------------------------------------------------------------------------------------------------------------
def dw64_of_rounded(g, x, k):
    """The float64 weight gradient of f16(g), f16(x) (exact products, float64 sums)."""
    w0 = np.zeros((g.shape[1], x.shape[1], k, k), np.float32)
    return R.conv_grads64(f16_round(g), f16_round(x), w0)[1]


def dw_f16(g, x, k):
    """The contract's dw, float32: float64 sum of the exact products, rounded once."""
    return dw64_of_rounded(g, x, k).astype(np.float32)


def dx_f16(g, w):
    """The contract's dx, float32: the f16 forward of w'[ci][co][ky][kx] = w[co][ci][ks-1-ky][ks-1-kx] on g (no bias, ReLU or pool)."""
    return conv_f16(g, R.flip_weights(w), None)


def abs_products(g, x, k, rounded=True):
    """sum over pixels of |g * x| per dw element, float64 (rounded: of the f16 operands)."""
    ga, xa = (np.abs(f16_round(a)) if rounded else np.abs(np.asarray(a, np.float64)) for a in (g, x))
    w0 = np.zeros((g.shape[1], x.shape[1], k, k), np.float32)
    return R.conv_grads64(ga, xa, w0)[1]


def dw_sum_bound(g, x, k, m):
    """m * 2^-23 * sum |f16(g) * f16(x)| per element, float64.  m = 16 + G + S (mfmas_per_strip): an element's sum passes through at most 16
    additions inside one MFMA, G additions of an MFMA's result to the accumulator and S - 1 additions of the combine, plus the one rounding of
    the reference; each addition errs by at most one unit of the partial sum, which the sum of magnitudes bounds.  The unit is 2^-23 and not
    2^-24 because the matrix core's internal addition may truncate instead of rounding to nearest."""
    return m * 2.0 ** -23 * abs_products(g, x, k)


def operand_rounding_bound(g, x, k):
    """((1 + 2^-11)^2 - 1) * sum |g * x| of the UNROUNDED operands: how far dw of the rounded operands lies from dw of the unrounded ones
    when every |g|, |x| is in the f16 normal range (relative rounding error 2^-11 each)."""
    return ((1.0 + 2.0 ** -11) ** 2 - 1.0) * abs_products(g, x, k, rounded=False)


# ---- lattices on which every fp32 summation order is exact ------------------------------------------------------------------------------------
def lattice_inputs(k, cin, cout, H, W, B, seed):
    """x integers in [-8, 8], w in [-2, 2], b = 0, dy = g (relu = pool = 0) integers in [-4, 4], float32.  Every product g * x is an integer of at
    most 32, so every partial sum of dw is an integer of at most 32 * B * H * W < 2^24 (asserted by the tests): no addition rounds.  dx sums
    cout * k * k products of at most 8 in magnitude."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-8, 9, (B, cin, H, W)).astype(np.float32)
    w = rng.integers(-2, 3, (cout, cin, k, k)).astype(np.float32)
    dy = rng.integers(-4, 5, (B, cout, H, W)).astype(np.float32)
    return x, w, np.zeros(cout, np.float32), dy


def edge_lattice_inputs(kind, on, k, cin, cout, H, W, B, seed):
    """The operand-edge values of f16_emulation.lattice_case carried to g (on = 'g') or to x (on = 'x'): what pins the device's conversion
    of both operands of the weight gradient to f16_rn_sat.  `edge` is the operand named by `on`, `other` the other one.
    'b': edge = unrounded subnormals -- q * 2^-24, |q| <= 1023, half of them at ties (q + 1/2) * 2^-24, a few at 2^-25 (the tie to zero), its
    float32 successor (rounds up to 2^-24) and -2^-26 (rounds to -0) -- and other = m * 2^8, integer |m| <= 4.  After f16() a product is a
    multiple of 2^-16 of at most 1023 * 4 * 2^-16; a sum of B * H * W <= 1104 of them stays below 69 < 2^8 = 2^-16 * 2^24: exact.
    'd': edge = +-(1 + (2 j + 1) * 2^-11), halfway between two f16 values of [1, 2], other integers in [-2, 2]: multiples of 2^-10 whose sums
    stay below 1104 * 2 * 2 < 2^14 = 2^-10 * 2^24: exact.
    w is integer in [-2, 2], so dx = sum over cout * k * k <= 128 * 49 products f16(g) * w is exact too: of multiples of 2^-24 below
    1023 * 2 * 6272 * 2^-24 < 1 ('b' on g), of 2^8 ('b' on x), of 2^-10 below 2 * 2 * 6272 < 2^14 ('d' on g), of integers ('d' on x)."""
    rng = np.random.default_rng(seed)
    shapes = {'g': (B, cout, H, W), 'x': (B, cin, H, W)}
    es, os_ = shapes[on], shapes['x' if on == 'g' else 'g']
    w = rng.integers(-2, 3, (cout, cin, k, k)).astype(np.float32)
    if kind == 'd':
        edge = ((1 + (2 * rng.integers(0, 1024, es) + 1) * 2.0 ** -11) * rng.choice([-1.0, 1.0], es)).astype(np.float32)
        other = rng.integers(-2, 3, os_).astype(np.float32)
    else:
        assert kind == 'b'
        edge = (rng.integers(-1023, 1024, es) * 2.0 ** -24).astype(np.float32)
        ties = (rng.random(es) < 0.5) & (edge < np.float32(1023 * 2.0 ** -24))          # (so that a tie never rounds past 1023 * 2^-24)
        edge = np.where(ties, edge + np.float32(2.0 ** -25), edge).astype(np.float32)
        flat = edge.reshape(-1)
        at = rng.choice(flat.size, 12, replace=False)
        flat[at[0:4]] = np.float32(2.0 ** -25)
        flat[at[4:8]] = np.nextafter(np.float32(2.0 ** -25), np.float32(1))
        flat[at[8:12]] = np.float32(-2.0 ** -26)
        other = (rng.integers(-4, 5, os_) * 2.0 ** 8).astype(np.float32)
    x, dy = (other, edge) if on == 'g' else (edge, other)
    return x, w, np.zeros(cout, np.float32), dy
