"""GPU: the head backward under option "grad_precision" = 2 with a static loss scale (include/pose_mi355x.h: pmx_backward_head, options
"grad_precision" and "loss_scale_log2", pmx_backward_g_census).  The pattern of tests/test_gpu_head_backward.py: one retained forward +
backward per configuration, everything fetched, every layer checked from the run's own retained arrays so that no error compounds.
  dw of the 58 3x3 / 7x7 layers   against the float64 sum of the products of the ROUNDED operands, within the f16 kernel's documented bound
                                  (16 + R * ceil(fw / 16) + S) * 2^-23 * sum |f16(g) * f16(x)| -- which the fp32 kernel's result does
                                  not meet (it multiplies the unrounded operands): the negative control
  g of every layer with consumers against the float64 sum of the consumers' data gradients (f16(g) * f16(w') for the 3x3 / 7x7 consumers, the
                                  unrounded products for the 1x1 ones), within n * 2^-23 * sum |p| per consumer of n = cout * ks^2 terms --
                                  any fp32 summation order of exact products -- plus 2^-23 * |u| per float32 add of the documented sums
  the fp32 parts                  the 1x1 layers' dw bit for bit the host twin's, every db within 2^-23 of float64, the maps untouched
and: the same bits on every run and under "f16_bn" / "conv_algo", no leak back into an fp32 run, the loss scale exact in fp32, the error
codes, the census against NumPy.
A: the primary case of test_gpu_head_backward.py (8 x 6 maps: one padded group per row).  B: 3 x 40 x 160, two stages, four strips asked for:
5 x 20 maps (two groups per row, the second of 4 pixels), 15 map rows in strips of 4, so the borders lie inside images and one strip is short."""
import functools

import numpy as np
import pytest

import conv_bwd_ref as R
import f16_grad_emulation as G
import grad_census_ref as census_ref
from f16_emulation import f16_round
from test_gpu_head_backward import PRIMARY, _data, _head
from test_gpu_head_backward import _weights as _make_weights

pytestmark = pytest.mark.gpu

INVALID, STATE = 1, 6
U23 = 2.0 ** -23
A = PRIMARY                                                               # B = 2, 64 x 48, 6 stages, automatic strips
B_CFG = dict(B=3, H=40, W=160, stages=2, strips=4, seed=2031)
K = 10                                                                    # loss_scale_log2 of the shared runs: gradients of 0.1 .. 5
CENSUS_LAYERS = ('conv4_3_CPM', 'conv5_3_CPM_L1', 'Mconv1_stage2_L2', 'Mconv5_stage6_L1', 'Mconv7_stage6_L2', 'conv5_5_CPM_L1')


@functools.lru_cache(maxsize=None)
def _weights():
    """the synthetic weights, made once (read-only)"""
    return _make_weights()


@pytest.fixture(scope='module')
def eng(native):
    e = native.Engine(0, max_batch=3, max_h=64, max_w=160)
    e.set_weights(_weights())
    yield e
    e.close()


def _run(eng, cfg, gp=2, k=K, late=(), fetch=True, census=()):
    """One retained forward + head backward under grad_precision gp and loss_scale_log2 k; `late`: options set AFTER the forward, so that
    the backward alone runs under them (the retained arrays are then the same whatever they are)."""
    imgs, poses, masks = _data(**cfg)
    n = cfg['stages']
    eng.loss_set_poses(poses, cfg['H'], cfg['W'], masks, 7, 8)
    eng.set_option('stop_stage', n)
    eng.set_option('wgrad_strips', cfg['strips'])
    eng.set_option('grad_precision', gp)
    eng.set_option('loss_scale_log2', k)
    eng.loss_grad_enable(True)
    eng.backward_enable(True)
    try:
        total, paf, heat = eng.validate_batch(imgs)
        out = dict(cfg=cfg, gp=gp, k=k, total=total, paf=paf, heat=heat, maps=eng.get_maps(), lg=[eng.loss_grads(s) for s in range(n)])
        assert eng.loss_grad_scale_log2() == k
        for key, val, _ in late:
            eng.set_option(key, val)
        eng.backward_head()
        names = list(_head(n))
        out['dw'], out['db'] = {}, {}
        for nm in names:
            out['dw'][nm], out['db'][nm] = eng.layer_grad(nm)
        out['trunk'] = eng.trunk_grad()
        if fetch:
            out['a'] = {nm: eng.retained(nm, 0) for nm in names + ['conv4_2']}
            out['g'] = {nm: eng.retained(nm, 1) for nm in names}
        out['census'] = {nm: eng.g_census(nm) for nm in census}
        out['maps_after'] = eng.get_maps()
    finally:
        eng.backward_enable(False)
        eng.loss_grad_enable(False)
        for key, _, default in late:
            eng.set_option(key, default)
        for key, default in (('stop_stage', 6), ('wgrad_strips', 0), ('grad_precision', 0), ('loss_scale_log2', 0)):
            eng.set_option(key, default)
    return out


_runs = {}


def _cached(eng, key):
    """the runs the tests share, made once: (configuration 'A' | 'B', grad_precision, k)"""
    if key not in _runs:
        name, gp, k = key
        _runs[key] = _run(eng, A if name == 'A' else B_CFG, gp=gp, k=k, census=CENSUS_LAYERS if name == 'A' else ())
    return _runs[key]


def _input(run, d):
    """a layer's input in the reference's channel order (Mconv1_*: 38 PAF, 19 heat, 128 feature)"""
    return np.concatenate([run['a'][p] for p in d['x']], axis=1)


def _is_f16(w):
    return w.shape[-1] > 1


def _dx_refs(run):
    """Per layer, from the run's own g: (dx64, n * 2^-23 * sum |p|) of the data gradient as the chain under test computes it -- the
    products of the rounded operands for a 3x3 / 7x7 layer under grad_precision 2, else of the unrounded ones; computed once per run."""
    if 'dx_refs' not in run:
        W = _weights()
        refs = {}
        for nm in _head(run['cfg']['stages']):
            w, g = W[nm][0], run['g'][nm]
            if run['gp'] == 2 and _is_f16(w):
                w, g = f16_round(w), f16_round(g)
            n = w.shape[0] * w.shape[-1] ** 2
            refs[nm] = (R.dx_pair(g, w)[0], n * U23 * R.dx_pair(np.abs(g), np.abs(w))[0])
        run['dx_refs'] = refs
    return run['dx_refs']


def _upstream(run, nm):
    """(u64, bound, n consumers) at the output of layer nm: the loss gradient of a stage output plus the consumers' data gradients; the
    bound: the consumers' own, plus 2^-23 * |u| per float32 add of the documented sums"""
    head = _head(run['cfg']['stages'])
    refs = _dx_refs(run)
    d = head[nm]
    shape = run['a'][nm].shape
    u, bound, terms = np.zeros(shape), np.zeros(shape), 0
    if d['out'] is not None:
        s, b = d['out']
        u = u + run['lg'][s - 1][b].astype(np.float64)
        terms += 1
    cons = 0
    for other, od in head.items():
        off = 0
        for p in od['x']:
            c = run['a'][p].shape[1]
            if p == nm:
                u = u + refs[other][0][:, off:off + c]
                bound = bound + refs[other][1][:, off:off + c]
                terms += 1
                cons += 1
            off += c
    return u, bound + max(terms - 1, 0) * U23 * np.abs(u), cons


def _dw_check(run, nm, d):
    """(error, bound) of dw of a 3x3 / 7x7 layer against the float64 sum of the rounded operands' products"""
    cfg = run['cfg']
    w = _weights()[nm][0]
    ks = w.shape[-1]
    g, x = run['g'][nm], _input(run, d)
    S, rows = G.strips_for(cfg['B'], cfg['H'] // 8, w.shape[0], w.shape[1], ks, cfg['strips'])
    m = 16 + rows * G.groups(cfg['W'] // 8) + S
    return np.abs(run['dw'][nm].astype(np.float64) - G.dw64_of_rounded(g, x, ks)), G.dw_sum_bound(g, x, ks, m)


def _check_f16_layers(run, stage):
    head = _head(run['cfg']['stages'])
    W = _weights()
    names = [nm for nm, d in head.items() if d['stage'] == stage]
    assert names
    n_f16 = 0
    for nm in names:
        d, w = head[nm], W[nm][0]
        a, g, dw, db = run['a'][nm], run['g'][nm], run['dw'][nm], run['db'][nm]
        for what, arr in (('a', a), ('g', g), ('dw', dw), ('db', db)):
            assert np.isfinite(arr).all(), 'unwritten (poisoned) or non-finite %s of %s' % (what, nm)
        assert dw.shape == w.shape and g.shape == a.shape
        if _is_f16(w):
            n_f16 += 1
            err, bound = _dw_check(run, nm, d)
            print(nm, 'dw err / bound %.4f' % float((err / np.maximum(bound, 1e-300)).max()), '|dw| max %.3e' % float(np.abs(dw).max()))
            assert (err <= bound).all(), (nm, float((err / np.maximum(bound, 1e-300)).max()))
            assert np.abs(dw).max() > 0, nm
        sel = a > 0 if d['relu'] else np.ones(a.shape, bool)
        assert not g.view(np.uint32)[~sel].any(), nm          # +0.0f by bits where a > 0 is false
        assert g[sel].any(), nm
        u64, ubound, cons = _upstream(run, nm)
        if cons == 0:          # the last stage's outputs: the loss gradient itself
            s, b = d['out']
            assert np.array_equal(g.view(np.uint32), run['lg'][s - 1][b].view(np.uint32)), nm
            continue
        assert cons == (2 if d['out'] is not None else 2 * run['cfg']['stages'] if nm == 'conv4_4_CPM' else 1), (nm, cons)
        eu = np.abs(g.astype(np.float64) - u64)
        print(nm, 'g err / bound %.4f' % float((eu[sel] / np.maximum(ubound[sel], 1e-300)).max()), '|u| max %.3e' % float(np.abs(u64).max()),
              'consumers', cons)
        assert (eu[sel] <= ubound[sel]).all(), (nm, float((eu[sel] / np.maximum(ubound[sel], 1e-300)).max()))
    if stage == 0:
        dx64, tbound = _dx_refs(run)['conv4_3_CPM']
        et = np.abs(run['trunk'].astype(np.float64) - dx64)
        print('trunk_grad err / bound %.4f' % float((et / np.maximum(tbound, 1e-300)).max()), '|u| max %.3e' % float(np.abs(dx64).max()))
        assert np.isfinite(run['trunk']).all() and run['trunk'].shape == dx64.shape
        assert (et <= tbound).all()
    return n_f16


# ---- 1. the per-layer contract ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stage', range(7))
def test_every_layer_of_case_a(eng, stage):
    n = _check_f16_layers(_cached(eng, ('A', 2, K)), stage)
    assert n == (2, 6, 10, 10, 10, 10, 10)[stage]          # the 58 layers with ksize > 1


@pytest.mark.parametrize('stage', range(3))
def test_every_layer_of_case_b(eng, stage):
    assert G.strips_for(3, 5, 128, 128, 7, 4) == (4, 4) and G.groups(20) == 2
    n = _check_f16_layers(_cached(eng, ('B', 2, K)), stage)
    assert n == (2, 6, 10)[stage]


def test_the_fp32_chain_does_not_meet_the_f16_bound(eng):
    """The negative control, and what fails without the feature: with the option at 0 the weight gradients are sums of the products of the
    UNROUNDED operands, which lie outside the bound around the sum of the rounded operands' products."""
    run = _cached(eng, ('A', 0, K))
    head = _head(A['stages'])
    outside = []
    for nm, d in head.items():
        if _is_f16(_weights()[nm][0]):
            err, bound = _dw_check(run, nm, d)
            if (err > bound).any():
                outside.append(nm)
    print('layers whose fp32 dw violates the f16 bound:', len(outside), 'of 58')
    assert outside


# ---- 2. the fp32 parts keep their contract in the f16 run ------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['A', 'B'])
def test_fp32_parts_keep_their_contract(eng, case):
    run = _cached(eng, (case, 2, K))
    cfg = run['cfg']
    W = _weights()
    n_1x1 = 0
    for nm, d in _head(cfg['stages']).items():
        g = run['g'][nm]
        db64 = g.astype(np.float64).sum(axis=(0, 2, 3))
        assert (np.abs(run['db'][nm].astype(np.float64) - db64) <= U23 * np.abs(db64)).all(), nm
        if not _is_f16(W[nm][0]):
            n_1x1 += 1
            assert np.array_equal(run['dw'][nm], R.wgrad_twin(g, _input(run, d), 1, cfg['strips'])), nm
    assert n_1x1 == (24 if case == 'A' else 8)
    for i in (0, 1):
        assert np.array_equal(run['maps'][i].view(np.uint32), run['maps_after'][i].view(np.uint32))


# ---- 3. the same bits on every run and under the forward's options ------------------------------------------------------------------------------
def _same_grads(x, y, what):
    for nm in x['dw']:
        assert np.array_equal(x['dw'][nm].view(np.uint32), y['dw'][nm].view(np.uint32)), (what, nm)
        assert np.array_equal(x['db'][nm].view(np.uint32), y['db'][nm].view(np.uint32)), (what, nm)
    assert np.array_equal(x['trunk'].view(np.uint32), y['trunk'].view(np.uint32)), what


@pytest.mark.parametrize('late', [None, ('f16_bn', 64, 0), ('f16_bn', 128, 0), ('conv_algo', 0, 1), ('conv_algo', 2, 1)])
def test_same_bits_on_every_run_and_setting(eng, late):
    run = _cached(eng, ('A', 2, K))
    again = _run(eng, A, late=[late] if late else (), fetch=False)
    assert again['total'] == run['total']
    _same_grads(run, again, late)


# ---- 4. switching back ---------------------------------------------------------------------------------------------------------------------------
def test_fp32_after_f16_is_the_fp32_of_before(eng):
    first = _run(eng, A, gp=0)
    between = _run(eng, A, gp=2, fetch=False)
    third = _run(eng, A, gp=0)
    _same_grads(first, third, 'fp32 / f16 / fp32')
    for nm in first['g']:
        assert np.array_equal(first['g'][nm].view(np.uint32), third['g'][nm].view(np.uint32)), nm
        assert np.array_equal(first['a'][nm].view(np.uint32), third['a'][nm].view(np.uint32)), nm
    for s in range(A['stages']):
        for i in (0, 1):
            assert np.array_equal(first['lg'][s][i].view(np.uint32), third['lg'][s][i].view(np.uint32)), s
    assert any(not np.array_equal(first['dw'][nm], between['dw'][nm]) for nm in first['dw'])          # the f16 run in between was one


# ---- 5. the loss scale is exact in fp32 ---------------------------------------------------------------------------------------------------------
def test_loss_scale_is_exact_in_fp32(eng):
    """2^8 times every gradient, bit for bit: rounding commutes with a power of two unless an unscaled intermediate is subnormal in fp32, and
    the gradients here are 1e-7 .. 1e-2."""
    base, scaled = _run(eng, A, gp=0, k=0), _run(eng, A, gp=0, k=8)
    f = np.float32(256)
    assert scaled['total'] == base['total'] and np.array_equal(scaled['paf'], base['paf']) and np.array_equal(scaled['heat'], base['heat'])
    for i in (0, 1):
        assert np.array_equal(scaled['maps'][i].view(np.uint32), base['maps'][i].view(np.uint32))
        assert np.array_equal(scaled['maps_after'][i].view(np.uint32), base['maps'][i].view(np.uint32))
    for s in range(A['stages']):
        for i in (0, 1):
            assert np.array_equal(scaled['lg'][s][i], f * base['lg'][s][i]), ('loss gradient', s, i)
    for nm in base['dw']:
        for what in ('dw', 'db', 'g'):
            assert np.array_equal(scaled[what][nm], f * base[what][nm]), (what, nm, int((scaled[what][nm] != f * base[what][nm]).sum()))
        assert np.array_equal(scaled['a'][nm].view(np.uint32), base['a'][nm].view(np.uint32)), nm
    assert np.array_equal(scaled['trunk'], f * base['trunk'])
    assert np.abs(base['trunk']).max() > 0


# ---- 6. errors -----------------------------------------------------------------------------------------------------------------------------------
def test_error_codes(native):
    eng = native.Engine(0, max_batch=A['B'], max_h=A['H'], max_w=A['W'])          # (its own: no f16 backward has built a pack here)
    try:
        eng.set_weights(_weights())
        _error_codes(native, eng)
    finally:
        eng.close()


def _error_codes(native, eng):
    def refused(code, fn, *args):
        with pytest.raises(native.PmxError) as e:
            fn(*args)
        assert e.value.code == code, (e.value.code, str(e.value))
        return str(e.value)

    for bad in (-1, 25):
        assert 'loss_scale_log2' in refused(INVALID, eng.set_option, 'loss_scale_log2', bad)
    for ok in (24, 0):
        eng.set_option('loss_scale_log2', ok)
    imgs, poses, masks = _data(**A)
    eng.loss_set_poses(poses, A['H'], A['W'], masks, 7, 8)
    eng.loss_grad_enable(True)
    eng.backward_enable(True)
    try:
        refused(STATE, eng.g_census, 'conv4_3_CPM')                # no retained forward yet
        eng.validate_batch(imgs)
        refused(STATE, eng.g_census, 'conv4_3_CPM')                # retained, but no backward yet
        assert eng.get_pack('conv4_4_CPM', 7) is None              # no f16 backward yet: PMX_ERR_STATE
        n = native.C.c_size_t(0)
        assert eng.lib.pmx_get_transposed_f16_pack(eng._ctx, b'conv4_4_CPM', None, 0, native.C.byref(n)) == STATE
        assert eng.lib.pmx_get_transposed_f16_pack(eng._ctx, b'no_such_layer', None, 0, native.C.byref(n)) == INVALID
        eng.set_option('grad_precision', 2)
        eng.set_option('precision', 2)
        try:
            assert 'precision' in refused(STATE, eng.backward_head)
        finally:
            eng.set_option('precision', 0)
        eng.backward_head()                                        # the context stays usable
        refused(INVALID, eng.g_census, 'no_such_layer')
        refused(INVALID, eng.g_census, 'conv4_2')
        assert eng.lib.pmx_backward_g_census(eng._ctx, b'conv4_3_CPM', None) == INVALID
        assert eng.g_census('conv4_3_CPM')['nonzero'] > 0
        pack = eng.get_pack('conv4_4_CPM', 't_f16')
        assert pack is not None and pack.dtype == np.uint16 and pack.size == eng.get_pack('conv4_4_CPM', 't_w').size
        assert eng.get_pack('conv5_4_CPM_L1', 7) is None           # a 1x1 layer has none
    finally:
        eng.set_option('grad_precision', 0)
        eng.backward_enable(False)
        eng.loss_grad_enable(False)


# ---- 7. the census ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [0, K])
def test_census_equals_numpy(eng, k):
    run = _cached(eng, ('A', 2, k))
    for nm in CENSUS_LAYERS:
        want = census_ref.census(run['g'][nm])
        print(k, nm, run['census'][nm])
        assert run['census'][nm] == want, (nm, run['census'][nm], want)
        assert want['nonzero'] > 0 and want['nan'] == 0 and want['saturated'] == 0


def test_the_loss_scale_lowers_the_flushed_count(eng):
    unscaled, scaled = _cached(eng, ('A', 2, 0)), _cached(eng, ('A', 2, K))
    for nm in CENSUS_LAYERS:
        assert scaled['census'][nm]['flushed'] <= unscaled['census'][nm]['flushed'], nm
    print({nm: (unscaled['census'][nm]['flushed'], scaled['census'][nm]['flushed']) for nm in CENSUS_LAYERS})
