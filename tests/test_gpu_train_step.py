"""GPU: the head training step (include/pose_mi355x.h: pmx_train_*) -- Adam on the 82 layers after conv4_2 and the weight packs rewritten on
the device.  The Adam launch bit for bit against tests/adam_twin.py from the library's own gradients; every pack bit for bit against the
packs a fresh context builds by one-off launches from the fetched weights; what a step must not touch; the loss trajectory of five steps against
float64 torch; the state round trip; the error codes.  Batch 2 at 64 x 48 (the network fixes the weight shapes)."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import adam_twin as A
import test_gpu_head_backward as HB
import train_ref as TR
from conftest import pkg

pytestmark = pytest.mark.gpu

CFG = HB.PRIMARY                       # batch 2 at 64 x 48, six stages
B, H, W = CFG['B'], CFG['H'], CFG['W']
MARGIN = HB.MARGIN                     # 16: test_whole_chain_against_float64_autograd's margin over torch's float32 run
SCALES = {'conv4_3_CPM': 0.25, 'conv4_4_CPM': 0.25}
TRUNK = TR.TRUNK
PACKS = ('w', 'b', 'wino', 't_w', 't_wino')


def _weights():
    return pkg('weights').synthetic_weights(0)


def _engine(native, weights=None, backward=True):
    e = native.Engine(0, max_batch=B, max_h=H, max_w=W)
    e.set_weights(_weights() if weights is None else weights)
    e.loss_grad_enable(True)
    if backward:
        e.backward_enable(True)
    return e


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _fb(eng, stages=6, algo=2, grads=False):
    """one retained forward + backward on the fixed batch -> losses, maps (and every dw, db, the trunk gradient)"""
    imgs, poses, masks = HB._data(**CFG)
    eng.loss_set_poses(poses, H, W, masks, 7, 8)
    eng.set_option('stop_stage', stages)
    eng.set_option('conv_algo', algo)
    try:
        total, paf, heat = eng.validate_batch(imgs)
        out = dict(total=total, paf=paf, heat=heat, maps=eng.get_maps())
        eng.backward_head()
        if grads:
            out['grads'] = {nm: eng.layer_grad(nm) for nm in eng.head_layers(stages)}
            out['trunk'] = eng.trunk_grad()
    finally:
        eng.set_option('stop_stage', 6)
        eng.set_option('conv_algo', 1)
    return out


def _same_run(a, b):
    ok = a['total'] == b['total'] and np.array_equal(a['paf'], b['paf']) and np.array_equal(a['heat'], b['heat'])
    ok = ok and all(_same(a['maps'][i], b['maps'][i]) for i in (0, 1))
    if 'grads' in a and 'grads' in b:
        ok = ok and _same(a['trunk'], b['trunk']) and sorted(a['grads']) == sorted(b['grads'])
        ok = ok and all(_same(a['grads'][nm][j], b['grads'][nm][j]) for nm in a['grads'] for j in (0, 1))
    return ok


def _packs(eng, names):
    return {(nm, k): eng.get_pack(nm, k) for nm in names for k in PACKS}


def _diff_packs(pa, pb):
    bad = []
    for key in pa:
        x, y = pa[key], pb[key]
        if (x is None) != (y is None) or (x is not None and not _same(x, y)):
            bad.append(key)
    return bad


def _digest(state):
    h = hashlib.sha256()
    for nm in sorted(state):
        for a in state[nm][:6]:
            h.update(np.ascontiguousarray(a).tobytes())
        h.update(str(state[nm][6]).encode())
    return h.hexdigest()


def _state(eng, names):
    """{layer: (W, b, m_W, v_W, m_b, v_b, t)}"""
    out = {}
    for nm in names:
        w, b = eng.get_layer(nm)
        out[nm] = (w, b) + eng.train_get_state(nm)
    return out


def _twin_step(old, grads, names, adam, scales=SCALES):
    """the twin applied to the state `old` of `names` and the library's own gradients -> the expected state"""
    new = {}
    for nm in names:
        w, b, mw, vw, mb, vb, t = old[nm]
        dw, db = grads[nm]
        w1, mw1, vw1 = A.step32(w, mw, vw, dw, scales.get(nm, 1.0), t + 1, **adam)
        b1, mb1, vb1 = A.step32(b, mb, vb, db, scales.get(nm, 1.0), t + 1, **adam)
        new[nm] = (w1, b1, mw1, vw1, mb1, vb1, t + 1)
    return new


def _mismatches(got, want):
    bad = []
    for nm in want:
        for j, what in enumerate(('W', 'b', 'm_W', 'v_W', 'm_b', 'v_b')):
            if not _same(got[nm][j], want[nm][j]):
                bad.append((nm, what, int((_bits(got[nm][j]) != _bits(want[nm][j])).sum())))
        if got[nm][6] != want[nm][6]:
            bad.append((nm, 't', got[nm][6], want[nm][6]))
    return bad


# ---- the sequence the tests share: made once, step by step -------------------------------------------------------------------------------
class Seq(object):
    """One training context: a forward in f16 mode (so that the f16 packs exist), a run with training off, training on (conv4_3_CPM /
    conv4_4_CPM at 1/4), a run, then steps 1, 2 (non-zero moments), 3 (alpha 1e-5) under conv_algo 2 -- all five kinds of pack exist from
    the first backward on -- and step 4 with stop_stage 2.  Each step is compared with the twin when it is made; the tests read the records."""

    def __init__(self, native):
        self.eng = e = _engine(native)
        self.head = e.head_layers()
        assert len(self.head) == 82
        imgs, _, _ = HB._data(**CFG)
        e.set_option('precision', 2)
        e.forward_u8(imgs)
        e.set_option('precision', 0)
        self.off = _fb(e, grads=True)                       # training off
        self.trunk0 = {nm: e.get_layer(nm) for nm in TRUNK}
        self.trunk_packs0 = {(nm, k): e.get_pack(nm, k) for nm in TRUNK for k in ('w', 'b', 'wino')}
        e.train_enable(True)
        for nm, sc in SCALES.items():
            e.train_set_grad_scale(nm, sc)
        self.on = _fb(e, grads=True)                        # training on, no step yet
        self.adam = dict(A.DEFAULTS)
        self.state = _state(e, self.head)
        self.start = self.state
        self.records = []
        self.digests = []

    def step(self, stages=6, adam=None):
        e = self.eng
        if adam is not None:
            self.adam = dict(adam)
            e.train_set_adam(**self.adam)
        names = e.head_layers(stages)
        run = _fb(e, stages=stages, grads=True) if self.records else self.on
        e.train_step_head()
        got = _state(e, self.head)
        want = dict(self.state)
        want.update(_twin_step(self.state, run['grads'], names, self.adam))
        self.records.append(dict(bad=_mismatches(got, want), names=names, t=[got[nm][6] for nm in self.head],
                                 moved=sum(not _same(got[nm][0], self.state[nm][0]) for nm in names), loss=run['total']))
        self.digests.append(_digest(got))
        self.state = got

    def upto(self, k):
        plan = [dict(), dict(), dict(adam=dict(A.DEFAULTS, alpha=1e-5)), dict(stages=2)]
        while len(self.records) < k:
            if len(self.records) == 3:          # before the stop_stage 2 step: what it must keep
                self.packs3 = _packs(self.eng, self.head)
                self.state3 = self.state
            self.step(**plan[len(self.records)])
        return self.records[k - 1]


_seq = {}


@pytest.fixture(scope='module')
def seq(native):
    if 'seq' not in _seq:
        _seq['seq'] = Seq(native)
    yield _seq['seq']
    _seq.pop('seq').eng.close()


@pytest.fixture(scope='module')
def fresh(native, seq):
    """A context that never trains: it gets the weights the training context holds after step 3 through pmx_set_layer and builds every
    pack by a one-off launch, lazily, under the same options.  Made when the training context stands at step 3, with what the tests compare: the
    next forward + backward of both contexts under conv_algo 2 and 0, and every pack of every head layer of both."""
    seq.upto(3)
    assert len(seq.records) == 3          # (every test that goes further asks for this fixture first)
    e = _engine(native, weights=seq.eng.get_weights())
    e.cmp = {2: (_fb(seq.eng, algo=2, grads=True), _fb(e, algo=2, grads=True))}
    e.packs = (_packs(seq.eng, seq.head), _packs(e, seq.head))
    e.cmp[0] = (_fb(seq.eng, algo=0, grads=True), _fb(e, algo=0, grads=True))
    yield e
    e.close()


# ---- 1. Adam bits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 2, 3])
def test_adam_bits_of_every_layer(seq, k):
    """W, b, m, v, t of all 82 layers after step k = the twin on the state before it and the library's own gradients, bit for bit: k = 1
    from zero moments, k = 2 with t = 2 and non-zero moments, k = 3 after alpha = 1e-5; conv4_3_CPM / conv4_4_CPM at scale 1/4."""
    rec = seq.upto(k)
    print('step', k, 'loss', rec['loss'], 'layers whose weights moved', rec['moved'], 'mismatches', rec['bad'][:5])
    assert rec['t'] == [k] * 82 and len(rec['names']) == 82
    assert rec['moved'] == 82
    assert not rec['bad'], rec['bad'][:10]


def test_adam_kernel_on_crafted_segments(seq):
    """The launch itself on caller arrays: segment lengths around the 16-byte vector and the 64-float pad, one longer than a block's 4096
    floats plus a tail; exact zeros, a denormal g * g, |g| = 1e-20 and 1e4; per-segment scale and alpha_t; the pad floats keep their bits."""
    lens = [1, 3, 4, 5, 63, 64, 65, 2 * 4096 + 37]
    rng = np.random.default_rng(5)
    off, pos = [], 0
    for n in lens:
        off.append(pos)
        pos += -(-n // 64) * 64 + (64 if n % 64 == 0 else 0)          # (a pad after every segment, also after the 64-float one)
    total = pos
    poison = np.full(total, 0x7fc0dead, np.uint32).view(np.float32)
    w, m, v, g = [poison.copy() for _ in range(4)]
    scale = np.array([1.0, 0.25, 1.0, 0.3, 1.0, 0.25, 1.0, 0.25], 'f')
    a_t = np.array([A.alpha_t(t) for t in (1, 2, 3, 1000, 1, 5, 7, 2)], 'f')
    special = np.array([0.0, -0.0, 1e-20, -1e-20, 1e4, -1e4, 3e-23, 1.0], 'f')          # (1e-20)^2 and (3e-23)^2: denormal and zero
    for i, (o, n) in enumerate(zip(off, lens)):
        w[o:o + n] = rng.normal(0, 0.05, n)
        g[o:o + n] = rng.normal(0, 1, n) * 10.0 ** rng.uniform(-8, 1, n)
        fresh_state = i % 2 == 0
        m[o:o + n] = 0 if fresh_state else rng.normal(0, 1e-2, n)
        v[o:o + n] = 0 if fresh_state else rng.uniform(0, 1e-3, n)
        k = min(n, len(special))
        g[o:o + k] = special[:k]
    g[off[-1] + 4096 - 3:off[-1] + 4096 + 3] = special[:6]          # across the border of two blocks
    assert (g[off[2]:off[2] + 4][2] ** 2 > 0) and (g[off[2]:off[2] + 4][2] ** 2 < np.finfo('f').tiny)
    w1, m1, v1 = seq.eng.adam_apply(w, m, v, g, off, lens, scale, a_t, np.float32(1 - 0.9), np.float32(1 - 0.999), np.float32(1e-8))
    inside = np.zeros(total, bool)
    for i, (o, n) in enumerate(zip(off, lens)):
        inside[o:o + n] = True
        we, me, ve = A.step32(w[o:o + n], m[o:o + n], v[o:o + n], g[o:o + n], scale[i], 0, a_t=a_t[i])
        for what, got, want in (('w', w1, we), ('m', m1, me), ('v', v1, ve)):
            assert _same(got[o:o + n], want), (n, what, int((_bits(got[o:o + n]) != _bits(want)).sum()))
        assert np.isfinite(we).all()
        if i % 2 == 0:
            assert _same(w1[o:o + 1], w[o:o + 1])          # g = +0 on fresh state: the weight keeps its bits
    for got in (w1, m1, v1):
        assert (_bits(got)[~inside] == 0x7fc0dead).all()


# ---- 2. pack bits ------------------------------------------------------------------------------------------------------------------------
def test_every_pack_equals_one_off_launches(seq, fresh):
    mine, theirs = fresh.packs
    exist = {k: sum(mine[(nm, k)] is not None for nm in seq.head) for k in PACKS}
    print('packs in existence', exist)
    wino = sum(seq.eng.layer_shape(nm)[-1] > 1 for nm in seq.head)
    # the 3x3 / 7x7 layers of the head: conv4_3_CPM, conv4_4_CPM, 2 x conv5_1 .. 3_CPM, 5 stages x 2 x Mconv1 .. 5
    assert exist == {'w': 82, 'b': 82, 'wino': wino, 't_w': 82, 't_wino': wino} and wino == 2 + 6 + 50
    assert not _diff_packs(mine, theirs), _diff_packs(mine, theirs)[:10]


@pytest.mark.parametrize('algo', [2, 0])
def test_next_forward_and_backward_equal_a_fresh_context(seq, fresh, algo):
    """maps, losses, the 82 dw / db and the trunk gradient of the next forward + backward: the trained context against the fresh one"""
    a, b = fresh.cmp[algo]
    assert _same_run(a, b)
    assert not _same(a['maps'][0], seq.off['maps'][0])          # (and they are not the untrained maps)


def test_stop_stage_keeps_the_later_stages(seq, fresh):
    rec = seq.upto(4)
    e = seq.eng
    assert len(rec['names']) == 2 + 10 + 14 and not rec['bad'], rec['bad'][:10]
    late = [nm for nm in seq.head if nm not in rec['names']]
    assert len(late) == 56
    for nm in late:
        assert _mismatches({nm: seq.state[nm]}, {nm: seq.state3[nm]}) == [], nm
        assert seq.state[nm][6] == 3
    assert all(seq.state[nm][6] == 4 for nm in rec['names'])
    now = _packs(e, seq.head)
    assert not _diff_packs({k: v for k, v in now.items() if k[0] in late}, {k: v for k, v in seq.packs3.items() if k[0] in late})
    assert len(_diff_packs({k: v for k, v in now.items() if k[0] in rec['names'] and k[1] == 'w'},
                           {k: v for k, v in seq.packs3.items() if k[0] in rec['names'] and k[1] == 'w'})) == len(rec['names'])
    for nm in rec['names']:          # the fresh context follows through pmx_set_layer and rebuilds its packs by one-off launches
        fresh.set_layer(nm, *e.get_layer(nm))
    b = _fb(fresh, stages=2, grads=True)
    assert not _diff_packs(now, _packs(fresh, seq.head)), _diff_packs(now, _packs(fresh, seq.head))[:10]
    assert _same_run(_fb(e, stages=2, grads=True), b)


# ---- 3. unchanged where nothing was asked ---------------------------------------------------------------------------------------------------
def test_trunk_untouched_and_training_without_a_step_changes_nothing(seq):
    seq.upto(3)
    assert _same_run(seq.off, seq.on)
    for nm in TRUNK:
        w, b = seq.eng.get_layer(nm)
        assert _same(w, seq.trunk0[nm][0]) and _same(b, seq.trunk0[nm][1]), nm
        assert _same(w, _weights()[nm][0]) and _same(b, _weights()[nm][1]), nm          # (pmx_get_layer un-packs what pmx_set_layer packed)
    assert not _diff_packs(self_packs(seq), seq.trunk_packs0)
    W0 = _weights()
    for nm in seq.head:          # the master store at enable = the weights installed
        assert _same(seq.start[nm][0], W0[nm][0]) and _same(seq.start[nm][1], W0[nm][1]), nm
        assert not seq.start[nm][2].any() and not seq.start[nm][3].any() and seq.start[nm][6] == 0


def self_packs(seq):
    return {(nm, k): seq.eng.get_pack(nm, k) for nm in TRUNK for k in ('w', 'b', 'wino')}


def test_two_runs_from_the_same_start_give_the_same_bits(native, seq):
    seq.upto(1)
    e = _engine(native)
    try:
        e.train_enable(True)
        for nm, sc in SCALES.items():
            e.train_set_grad_scale(nm, sc)
        _fb(e)
        e.train_step_head()
        assert _digest(_state(e, seq.head)) == seq.digests[0]
        # pmx_set_layer with training on: the master weights follow, Adam's state of the layer stays
        nm = 'Mconv1_stage2_L1'
        before = e.train_get_state(nm)
        e.set_layer(nm, *_weights()[nm])
        got = e.get_layer(nm)
        assert _same(got[0], _weights()[nm][0]) and _same(got[1], _weights()[nm][1])
        after = e.train_get_state(nm)
        assert after[4] == before[4] == 1 and all(_same(x, y) for x, y in zip(before[:4], after[:4])) and after[0].any()
    finally:
        e.close()


# ---- 4. other modes see the new weights -----------------------------------------------------------------------------------------------------
def test_f16_mode_after_a_step(seq, fresh):
    """the f16 packs existed before the first step (Seq.__init__): they must not be used stale"""
    seq.upto(3)
    if len(seq.records) > 3:
        for nm in seq.head:
            fresh.set_layer(nm, *seq.eng.get_layer(nm))
    imgs, _, _ = HB._data(**CFG)
    maps = []
    for e in (seq.eng, fresh):
        e.set_option('precision', 2)
        try:
            e.forward_u8(imgs)
            maps.append(e.get_maps())
        finally:
            e.set_option('precision', 0)
    assert _same(maps[0][0], maps[1][0]) and _same(maps[0][1], maps[1][1])


# ---- 5, 6. it trains; the state round trip --------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def det():
    d = pkg('pose_detector').PoseDetector(weights=_weights(), device=0, max_batch=B, max_size=(H, W))
    yield d
    d.engine.close()


def test_five_steps_against_float64_torch(det):
    """main/loss of five steps on one batch: falls at every step, and follows the float64 torch run of the same five steps (head only,
    trunk frozen, Chainer's Adam in float64).  Tolerance: the largest deviation over the trajectory of the float32 torch run (float32
    autograd, the float32 contract) from the float64 one, times the margin 16 of test_whole_chain_against_float64_autograd -- different but
    legitimate float32 orders.  The float64 losses of this fixture are 1.899, 0.791, 0.548, 0.465, 0.423: falls of 58, 31, 15 and 9 % per step
    (>= 1 % asserted); the library's largest deviation from them was 5.8e-8, the float32 torch run's 3.2e-6 (ratio 0.018; EXPERIMENTS.md E38)."""
    imgs, poses, masks = HB._data(**CFG)
    lib = np.array([det.train_step(list(imgs), poses, list(masks))['main/loss'] for _ in range(5)])
    targets = det.engine.loss_targets()
    l64, _ = TR.trajectory(_weights(), imgs, targets, 5, 'float64', SCALES)
    l32, _ = TR.trajectory(_weights(), imgs, targets, 5, 'float32', SCALES)
    tol = MARGIN * np.abs(l32 - l64).max()
    dev = np.abs(lib - l64)
    print('library', lib, 'float64', l64, 'float32 torch deviation', np.abs(l32 - l64), 'library deviation', dev, 'ratio to the yardstick',
          dev.max() / np.abs(l32 - l64).max())
    assert (l64[1:] <= 0.99 * l64[:-1]).all()
    assert (lib[1:] < lib[:-1]).all()
    assert (dev <= tol).all()


def test_state_round_trip(det, tmp_path):
    imgs, poses, masks = HB._data(**CFG)
    if not det._train_on:
        det.train_step(list(imgs), poses, list(masks))
    path = str(tmp_path / 'trained.npz')
    pkg('weights').save_npz(path, det.get_weights())
    opt = det.optimizer_state()
    np.savez(str(tmp_path / 'opt.npz'), **opt)
    other = pkg('pose_detector').PoseDetector(weights_file=path, device=0, max_batch=B, max_size=(64, 64))
    try:
        other.load_optimizer_state(np.load(str(tmp_path / 'opt.npz')))
        a = det.train_step(list(imgs), poses, list(masks))
        b = other.train_step(list(imgs), poses, list(masks))
        assert a == b
        wa, wb = det.get_weights(), other.get_weights()
        assert sorted(wa) == sorted(wb) and len(wa) == 92
        for nm in wa:
            assert _same(wa[nm][0], wb[nm][0]) and _same(wa[nm][1], wb[nm][1]), nm
        sa, sb = det.optimizer_state(), other.optimizer_state()
        assert sorted(sa) == sorted(sb) and all(_same(np.asarray(sa[k], np.float32), np.asarray(sb[k], np.float32)) for k in sa)
        with pytest.raises(ValueError):
            det.train_step(list(imgs) * 2, poses * 2, list(masks) * 2)          # more than max_batch
        # a larger image: `det` grows its context (64 x 48 -> 64 x 64) and carries weights and Adam's state over; `other` was made that large
        big = HB._data(B=B, H=64, W=64, seed=7)
        a = det.train_step(list(big[0]), big[1], list(big[2]))
        b = other.train_step(list(big[0]), big[1], list(big[2]))
        assert a == b and det._cap == (B, 64, 64)
        wa, wb = det.get_weights(), other.get_weights()
        assert all(_same(wa[nm][0], wb[nm][0]) and _same(wa[nm][1], wb[nm][1]) for nm in wa)
        sa, sb = det.optimizer_state(), other.optimizer_state()
        assert all(_same(np.asarray(sa[k], np.float32), np.asarray(sb[k], np.float32)) for k in sa) and int(sa['conv4_3_CPM/t']) == int(sb['conv4_3_CPM/t']) > 1
    finally:
        other.engine.close()


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------------------
def test_error_codes(native):
    imgs, poses, masks = HB._data(**CFG)
    e = _engine(native, backward=False)
    face = native.Engine(0, max_batch=1, max_h=64, max_w=64, arch='facenet')
    lib = e.lib

    def refused(code, fn, *args):
        with pytest.raises(native.PmxError) as err:
            fn(*args)
        assert err.value.code == code, (err.value.code, str(err.value))

    def forward():
        e.forward_u8(imgs)
        return e.get_maps()
    try:
        ref = forward()
        refused(6, e.train_enable)                              # pmx_backward_enable is off
        refused(6, e.train_step_head)                           # training is off
        refused(6, e.train_set_adam)
        e.backward_enable(True)
        e.set_option('precision', 2)
        refused(6, e.train_enable)                              # not fp32
        e.set_option('precision', 0)
        refused(6, face.train_enable)                           # a facenet context
        refused(6, face.train_step_head)
        e.train_enable(True)
        refused(6, e.train_step_head)                           # no backward
        e.loss_set_poses(poses, H, W, masks, 7, 8)
        e.validate_batch(imgs)
        refused(6, e.train_step_head)                           # a retained forward, still no backward
        e.backward_head()
        e.set_option('precision', 2)
        refused(6, e.train_step_head)                           # not fp32
        e.set_option('precision', 0)
        refused(1, e.train_set_grad_scale, 'no_such_layer', 1.0)
        refused(1, e.train_set_grad_scale, 'conv4_2', 1.0)      # a trunk layer
        refused(1, e.get_layer, 'no_such_layer')
        refused(1, e.train_get_state, 'no_such_layer')
        refused(1, e.train_set_adam, -1.0)
        n = C.c_size_t(0)
        assert lib.pmx_get_pack(e._ctx, b'no_such_layer', 0, None, 0, C.byref(n)) == 1
        assert lib.pmx_get_pack(e._ctx, b'conv4_3_CPM', 7, None, 0, C.byref(n)) == 1
        assert lib.pmx_get_pack(e._ctx, b'conv4_3_CPM', 0, None, 0, None) == 1
        assert lib.pmx_get_pack(e._ctx, b'conv5_4_CPM_L1', 2, None, 0, C.byref(n)) == 6          # a 1x1 layer has no Winograd pack
        assert lib.pmx_train_step_head(None) == 1 and lib.pmx_train_enable(None, 1) == 1
        assert lib.pmx_get_layer(e._ctx, b'conv1_1', None, None) == 1 and lib.pmx_get_layer(e._ctx, None, None, None) == 1
        assert lib.pmx_train_set_state(e._ctx, b'conv4_3_CPM', None, None, None, None, 0) == 1
        assert lib.pmx_train_set_grad_scale(e._ctx, None, 1.0) == 1
        assert lib.pmx_adam_apply(e._ctx, None, None, None, None, 0, None, None, None, None, 1, 0.1, 0.001, 1e-8) == 1
        maps = forward()
        assert _same(maps[0], ref[0]) and _same(maps[1], ref[1])          # nothing above changed a weight
        e.loss_set_poses(poses, H, W, masks, 7, 8)
        e.validate_batch(imgs)
        e.backward_head()
        e.train_step_head()
        g = e.layer_grad('conv4_3_CPM')                         # the gradients stay readable
        refused(6, e.train_step_head)                           # consumed
        assert _same(g[0], e.layer_grad('conv4_3_CPM')[0])
        after = forward()
        assert not _same(after[0], ref[0])
        assert _same(forward()[0], after[0])
        e.train_enable(False)
        refused(6, e.train_step_head)
        assert _same(forward()[0], after[0])                    # the trained weights stay when the stores go
    finally:
        e.close()
        face.close()
