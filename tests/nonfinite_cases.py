"""Helper of tests/test_nonfinite_host.py and tests/test_gpu_nonfinite.py, not collected itself: the single-layer cases of the forward
contract for non-finite values (include/pose_mi355x.h: relu(NaN) = NaN, a 2x2 pool with a NaN input is NaN, +-inf follow IEEE
arithmetic), the values planted into their inputs, and the masks the two files compare with.

A case is a launch form of the library with the smallest shape the bit-exact tests of tests/test_gpu_conv.py / test_gpu_winograd.py
use for it.  plant() puts, in this order and as far as the case's budget allows,
  nan     a NaN at an odd (y, x) -- the interior of a 2x2 tile --; the host test checks with the twin that the clean pre-ReLU output at
          that pixel is negative in at least one channel (so a ReLU that drops the NaN returns 0 there, not the clean value), and, for
          pooled cases, that the NaN reaches exactly one output of the 2x2 group below / right of it while a finite bump in x makes the
          group's other three pre-pool values of one channel larger than anything else in that channel's map (a pool that drops the NaN
          returns the largest of them);
  corner  a NaN on the last row and last column: its window covers the padding;
  +inf    in the middle of the map;
  -inf    in the last image, in the last input channel (the ragged 16- / 32-channel chunk where cin is no multiple);
  extras  the case's own positions (slab seam, tail tiles).
With two images the +inf goes into the first (next to the NaN) and the corner NaN and the -inf into the second, with three or more into
the third.  The budget: the bound mask -- every output that may be non-finite -- covers at most one third of an image's outputs, so that two thirds
are compared exactly; a value that would break it is left out (plant() returns what it planted), except the first NaN of a map too small
for any value (3 x 5 under a 7x7 kernel: its whole map is one patch).  KINDS says which cases are short of a kind -- those two, all others
carry all four -- and tests/test_nonfinite_host.py holds plant() to it."""
import functools

import numpy as np

from oracle import conv_fma_ref as R
from oracle import network_ref as N

TOL = 2e-5          # the bar of tests/test_gpu_conv.py / test_gpu_winograd.py between a kernel and torch: TOL * max(1, max |ref|)


def _c(cid, kind, shape, pool=False, extras=(), **opts):
    return dict(id=cid, kind=kind, shape=shape, pool=pool, extras=tuple(extras), opts=opts)


NAN, INF = float('nan'), float('inf')
# shape = (B, cin, H, W, cout, k); direct: variant = force_variant_k<k>, ksplit; wino: algo = conv_algo, tail = wino_tail, unit = wino_unit_g
CASES = [
    _c('v1_k3', 'direct', (2, 16, 10, 12, 64, 3), variant=2),
    _c('v1_k1', 'direct', (2, 128, 8, 16, 128, 1), variant=3),
    _c('v5_k7', 'direct', (2, 48, 6, 46, 128, 7), variant=10),
    _c('v5_k3_pool', 'direct', (2, 35, 16, 16, 64, 3), pool=True, variant=14),
    _c('v5_k3_ragged', 'direct', (2, 20, 9, 9, 19, 3), variant=16),
    _c('v6_k7', 'direct', (2, 33, 13, 46, 128, 7), variant=17),
    _c('v6_k3', 'direct', (2, 140, 25, 92, 256, 3), variant=18, extras=[(0, 7, 12, 45, NAN), (1, 9, 12, 46, INF)]),
    _c('v6_k3_pool', 'direct', (2, 128, 12, 46, 128, 3), pool=True, variant=19),
    _c('v6_k7_nine', 'direct', (2, 17, 7, 46, 200, 7), variant=21),
    _c('strip_k7', 'direct', (2, 32, 10, 46, 128, 7), variant=8),
    _c('strip_k3', 'direct', (2, 32, 7, 30, 128, 3), variant=9),
    _c('conv1_1', 'direct', (2, 3, 20, 24, 64, 3), variant=20),
    _c('splitk5_k7', 'direct', (1, 185, 16, 16, 64, 7), variant=15, ksplit=5),
    _c('splitk5_k7_wide', 'direct', (1, 185, 20, 28, 64, 7), variant=15, ksplit=5),      # the same launch form on a map with room for the infinities
    _c('splitk3_k3_pool', 'direct', (1, 100, 24, 32, 128, 3), pool=True, variant=13, ksplit=3),
    _c('default_k1', 'direct', (2, 100, 9, 13, 38, 1)),
    _c('wino_rect_130', 'wino', (2, 32, 9, 15, 130, 3), algo=2),
    _c('wino_rect_pool', 'wino', (3, 64, 22, 18, 128, 3), pool=True, algo=2),
    _c('wino_rect_k7', 'wino', (2, 32, 19, 21, 128, 7), algo=2),
    _c('wino_rect_k7_tiny', 'wino', (1, 32, 3, 5, 128, 7), algo=2),
    _c('wino_run', 'wino', (1, 64, 3, 46, 128, 3), algo=2),
    _c('wino_run_pool_seam', 'wino', (2, 32, 24, 92, 128, 3), pool=True, algo=2, extras=[(0, 5, 8, 45, NAN), (1, 6, 16, 46, NAN)]),
    _c('wino_tail', 'wino', (1, 64, 10, 46, 128, 3), algo=2, tail=1, extras=[(0, 9, 9, 20, NAN), (0, 3, 2, 10, INF)]),
    _c('wino_tail_pool', 'wino', (1, 128, 20, 184, 128, 3), pool=True, algo=2, tail=1, extras=[(0, 9, 19, 40, NAN), (0, 3, 5, 100, NAN)]),
    _c('wino_merged_tails', 'wino', (7, 64, 24, 46, 132, 3), algo=2, tail=1, extras=[(3, 9, 23, 40, NAN), (4, 3, 4, 10, INF)]),
    _c('wino_unit_k7', 'wino', (1, 128, 46, 46, 128, 7), algo=3, unit=-1),
]
CASE_IDS = [c['id'] for c in CASES]
# maps smaller than the patch of one planted value: the third cannot hold, the one NaN is planted all the same
TOO_SMALL = {'wino_rect_k7_tiny'}
# what plant() puts into a case: every other case carries all four kinds (and its extras).  The 16 x 16 map of the 5-slice split-K case
# has room for two 7x7 windows; 'splitk5_k7_wide' is that launch form with all four.
KINDS_ALL = ('nan', 'corner', '+inf', '-inf')
KINDS = {'wino_rect_k7_tiny': ('nan',), 'splitk5_k7': ('nan', 'corner')}


def data(case):
    """The files' usual operands: standard_normal x and bias, weights scaled by 1 / sqrt(K)."""
    B, cin, H, W, cout, k = case['shape']
    rng = np.random.default_rng(4000 + sum(case['shape']) + 7 * CASE_IDS.index(case['id']))
    x = rng.standard_normal((B, cin, H, W)).astype('f')
    w = (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype('f')
    return x, w, rng.standard_normal(cout).astype('f')


def window_mask(pos, B, H, W, k):
    """(B, H, W) bool: the pre-pool outputs whose k x k window holds one of the positions (b, c, y, x, value)."""
    m = np.zeros((B, H, W), bool)
    p = k // 2
    for b, _, y, x, _ in pos:
        m[b, max(0, y - p):y + p + 1, max(0, x - p):x + p + 1] = True
    return m


def tile_any(m):
    """(B, ceil(H / 2), ceil(W / 2)): any of an even-aligned 2x2 tile."""
    B, H, W = m.shape
    q = np.zeros((B, H + H % 2, W + W % 2), bool)
    q[:, :H, :W] = m
    return q.reshape(B, (H + 1) // 2, 2, (W + 1) // 2, 2).any(axis=(2, 4))


def bound_mask(case, pos):
    """(B, Ho, Wo) bool: where the contract allows a non-finite output.  A direct kernel: the outputs whose window (pooled: one of the
    four windows) holds a planted value.  A Winograd kernel: every output of a 2x2 tile one of whose windows does -- the transforms
    share the tile's 4 x 4 (7x7: 8 x 8) patch and compute inf - inf."""
    B, cin, H, W, cout, k = case['shape']
    m = window_mask(pos, B, H, W, k)
    t = tile_any(m)
    if case['pool']:
        return t[:, :H // 2, :W // 2]
    if case['kind'] == 'wino':
        return np.repeat(np.repeat(t, 2, axis=1), 2, axis=2)[:, :H, :W]
    return m


def pool_bump(case, x, w, at):
    """Pooled cases: the NaN at odd (y, x) reaches, of the 2x2 group (y + 1 .. y + 2, x + 1 .. x + 2), the output (y + 1, x + 1) only.  Adds
    a finite bump to x[b, c2, y + 2, x + 2]: taps (2, 1), (1, 2), (1, 1) of the group's other three outputs, (2, 2) of the NaN one and the
    first row / column of five neighbours.  (c2, n) is the (input, output) channel pair whose three taps exceed the other five (and 0) by
    the largest gap; the bump is sized so that the three pre-pool values of channel n exceed a map of range +-10 (standard_normal
    operands: |z| stays below 7).  Returns (c2, n): tests/test_nonfinite_host.py checks the property with the twin."""
    b, _, y, xx, _ = at
    three = np.minimum(np.minimum(w[:, :, 2, 1], w[:, :, 1, 2]), w[:, :, 1, 1])
    other = np.maximum(w[:, :, 0, :].max(axis=2), w[:, :, :, 0].max(axis=2))
    gap = three - np.maximum(other, 0)
    n, c2 = np.unravel_index(np.argmax(gap), gap.shape)
    assert gap[n, c2] > 0
    x[b, c2, y + 2, xx + 2] = np.float32(40.0 / gap[n, c2])
    return int(c2), int(n)


def plant(case, x, w):
    """Plants the values into x (in place; pooled cases get their bump first) and returns (positions planted, (c2, n) of the bump or
    None).  Deterministic: depends on the case alone."""
    B, cin, H, W, cout, k = case['shape']
    y0, x0 = min(3, H - 1), min(5, W - 1)                   # odd coordinates: the second row / column of a 2x2 tile
    y0, x0 = y0 - (1 - y0 % 2), x0 - (1 - x0 % 2)
    want = [(0, 1 % cin, y0, x0, NAN), (min(1, B - 1), 0, H - 1, W - 1, NAN), (2 if B > 2 else 0, 2 % cin, H // 2, (2 * W) // 3, INF),
            (B - 1, cin - 1, (2 * H) // 3, W // 3, -INF)] + list(case['extras'])
    bump = None
    if case['pool']:
        bump = pool_bump(case, x, w, want[0])
    pos = []
    for p in want:
        frac = bound_mask(case, pos + [p]).mean(axis=(1, 2)).max()
        if frac <= 1 / 3 or (not pos and case['id'] in TOO_SMALL):
            pos.append(p)
    for b, c, y, xx, v in pos:
        x[b, c, y, xx] = v
    return pos, bump


def cleaned(x, pos):
    xc = x.copy()
    for b, c, y, xx, _ in pos:
        xc[b, c, y, xx] = 0.0
    return xc


def unit_plan(case):
    """(unit_g, unit_from) of the twin for the case's launch form (tests/test_gpu_winograd.py restates conv_select.hip's plan)."""
    B, cin, H, W, cout, k = case['shape']
    o = case['opts']
    g = -(-((cin + 31) // 32) // (8 - (3 if k == 7 else 0)))
    if o.get('tail'):
        return g, R.wino_run_unit_from(H, W)
    if o.get('algo') == 3:
        return g, 0
    return 0, 0


def twin(case, x, w, b, relu, pool=None):
    """The order-defined plain-C twin of the case's launch form."""
    pool = case['pool'] if pool is None else pool
    if case['kind'] == 'direct':
        return R.conv_fma(x, w, b, relu=relu, pool=pool, splitk=case['opts'].get('ksplit', 1))
    g, uf = unit_plan(case)
    return R.conv_wino(x, w, b, relu, pool, unit_g=g, unit_from=uf)


@functools.lru_cache(maxsize=None)
def prepared(cid):
    """(case, x planted, x cleaned, w, b, positions, bump, bound mask) of a case -- built once, shared, never written to."""
    case = CASES[CASE_IDS.index(cid)]
    x, w, b = data(case)
    pos, bump = plant(case, x, w)
    xc = cleaned(x, pos)
    for a in (x, xc, w, b):
        a.setflags(write=False)
    return case, x, xc, w, b, pos, bump, bound_mask(case, pos)


@functools.lru_cache(maxsize=None)
def references(cid, relu):
    """(twin, torch) outputs on the planted input of a case -- computed once per (case, relu)."""
    case, x, xc, w, b, pos, bump, bound = prepared(cid)
    t = twin(case, x, w, b, relu)
    r = N.conv2d_ref(x.copy(), w.copy(), b.copy(), relu=relu, pool=case['pool'])        # (torch wants writable arrays)
    t.setflags(write=False)
    r.setflags(write=False)
    return t, r


def check_against_contract(case, y, y_clean, t, ref, bound):
    """The four assertions of a single-layer case: y = the output on the planted input, y_clean = the same function on the cleaned
    input, t = the twin on the planted input (None: y IS the twin), ref = torch on the planted input."""
    cid = case['id']
    assert y.shape == ref.shape == y_clean.shape
    bad, rbad = ~np.isfinite(y), ~np.isfinite(ref)
    bb = np.broadcast_to(bound[:, None], y.shape)
    assert rbad.any() and np.isnan(y).any(), (cid, 'nothing non-finite came out')
    if t is not None:                                                             # (a) the bit bar, NaN positions included
        assert np.array_equal(y, t, equal_nan=True), (cid, int(((y != t) & ~(np.isnan(y) & np.isnan(t))).sum()))
    if case['kind'] == 'direct':                                                  # (b) the non-finite set
        assert np.array_equal(bad, rbad), (cid, int(bad.sum()), int(rbad.sum()), np.argwhere(bad != rbad)[:6].tolist())
    else:
        assert not (rbad & ~bad).any(), (cid, 'finite where the float reference is not', int((rbad & ~bad).sum()), np.argwhere(rbad & ~bad)[:6].tolist())
    assert not (bad & ~bb).any(), (cid, 'non-finite outside the bound', int((bad & ~bb).sum()), np.argwhere(bad & ~bb)[:6].tolist())
    assert np.isfinite(y_clean).all(), cid
    assert np.array_equal(y[~bb], y_clean[~bb]), (cid, 'outside the bound the planted values changed bits', int((y[~bb] != y_clean[~bb]).sum()))   # (c)
    fin = ~bad & ~rbad                                                            # (d) finite entries vs torch
    if fin.any():                                                                 # (none in a map that is one patch)
        tol = TOL * max(1.0, float(np.abs(ref[~rbad]).max()))
        err = float(np.abs(y[fin] - ref[fin]).max())
        assert err <= tol, (cid, err, tol)
    else:
        assert cid in TOO_SMALL, cid
