"""Host (no GPU): the plain-C twins (oracle/conv_fma_ref.c) meet the forward contract for non-finite values on their own -- the CPU
proof of the conditions tests/test_gpu_nonfinite.py relies on when it holds the kernels to the twins bit for bit.

For every single-layer case of tests/nonfinite_cases.py, against the float reference oracle/network_ref.py::conv2d_ref (F.relu and
F.max_pool2d propagate NaN, as numpy.maximum and col.max of the reference's CPU path do):
  * conv_fma (direct kernels) is non-finite exactly where torch is; conv_wino on a superset of torch's positions and a subset of the
    tile bound;
  * everything outside the bound is bit-equal to the twin on the input with the planted values replaced by 0;
  * the bound covers at most one third of each image's outputs, the rest is compared exactly;
  * what the planted NaN is there for: its pixel's clean pre-ReLU output is negative in some channel, and in pooled cases the other
    three pre-pool values of its 2x2 group are the largest of their channel's map."""
import numpy as np
import pytest

import nonfinite_cases as NF


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('cid', NF.CASE_IDS)
def test_twins_meet_the_contract(cid, relu):
    case, x, xc, w, b, pos, bump, bound = NF.prepared(cid)
    t, ref = NF.references(cid, relu)
    t_clean = NF.twin(case, xc, w, b, relu)
    NF.check_against_contract(case, t, t_clean, None, ref, bound)
    if relu:            # the C twins' own ReLU on a NaN / -inf / +inf, spelled out
        z = NF.twin(case, x, w, b, 0)
        assert np.array_equal(np.isnan(t), np.isnan(z)) and (t[~np.isnan(t)] >= 0).all()
        assert not np.signbit(t[t == 0]).any()


@pytest.mark.parametrize('cid', NF.CASE_IDS)
def test_planted_values_are_where_they_matter(cid):
    case, x, xc, w, b, pos, bump, bound = NF.prepared(cid)
    B, cin, H, W, cout, k = case['shape']
    frac = bound.mean(axis=(1, 2))
    assert (frac <= 1 / 3).all() or cid in NF.TOO_SMALL, (cid, frac.tolist())
    assert bound.any() and np.isnan(pos[0][4]) and (np.isnan(x).sum(), np.isinf(x).sum()) == (sum(np.isnan(p[4]) for p in pos), sum(np.isinf(p[4]) for p in pos))
    # which kinds the case carries: all four (and every extra) unless NF.KINDS names it
    kinds = []
    for bb, c, y, xx, v in pos[:4]:
        kinds.append('+inf' if v == np.inf else '-inf' if v == -np.inf else 'corner' if (y, xx) == (H - 1, W - 1) else 'nan')
    assert tuple(kinds) == NF.KINDS.get(cid, NF.KINDS_ALL), (cid, kinds)
    if cid not in NF.KINDS:
        assert len(pos) == 4 + len(case['extras']) and pos[3][0] == B - 1 and pos[3][1] == cin - 1, (cid, pos)
    # the clean input: the planted pixels hold their drawn values again (the bump of a pooled case stays)
    x0, _, _ = NF.data(case)
    xb = xc.copy()
    for bb, c, y, xx, _ in pos:
        xb[bb, c, y, xx] = x0[bb, c, y, xx]
    z = NF.twin(case, xb, w, b, 0, pool=False)                          # pre-ReLU, pre-pool
    b0, _, y0, xx0, _ = pos[0]
    assert y0 % 2 == 1 and xx0 % 2 == 1 and z[b0, :, y0, xx0].min() < 0, (cid, float(z[b0, :, y0, xx0].min()))
    if case['pool']:
        c2, n = bump
        zn = z[b0, n].copy()
        three = [zn[y0 + 1, xx0 + 2], zn[y0 + 2, xx0 + 1], zn[y0 + 2, xx0 + 2]]
        zn[y0 + 1:y0 + 3, xx0 + 1:xx0 + 3] = -np.inf
        assert min(three) > zn.max(), (cid, three, float(zn.max()))
        # and the NaN reaches, before the pool, exactly one output of that group (direct kernels)
        m = NF.window_mask(pos[:1], B, H, W, k)[b0, y0 + 1:y0 + 3, xx0 + 1:xx0 + 3]
        assert m.tolist() == [[True, False], [False, False]]


def test_case_list_covers_the_launch_forms():
    ids = set(NF.CASE_IDS)
    assert len(ids) == len(NF.CASE_IDS) == 26
    pooled = [c['id'] for c in NF.CASES if c['pool']]
    assert len(pooled) == 6 and all(c['shape'][5] == 3 for c in NF.CASES if c['pool'])
    assert {c['opts'].get('variant') for c in NF.CASES if c['kind'] == 'direct'} >= {2, 3, 10, 14, 16, 17, 18, 19, 21, 8, 9, 20, 15, 13, None}
