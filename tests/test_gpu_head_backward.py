"""GPU: the head backward (include/pose_mi355x.h: pmx_backward_enable / pmx_backward_head) -- the gradients of the 82 layers after conv4_2.
Per layer, from the library's own retained arrays: dw bit for bit against the order-defined host twin and within the bound of a float32 sum
of products, db and the upstream gradients against float64, the ReLU gates by bits.  The whole chain against float64 torch autograd, with
torch's own float32 autograd as the yardstick (the figures of a run: EXPERIMENTS.md E37).
Pinned per layer, in every run (primary, stop_stage 2 with forced strips, the four option sweeps; figures: E40): the upstream gradient g of
every layer that has a consumer, over its open gates, and the trunk gradient, against the float64 sum of the consumers' data gradients with
the same sum of torch's float32 data gradients, added in float32 in the documented order, as the yardstick (conv_bwd_ref.ratio, at most
MARGIN in L2 and in the maximum).  The elementwise bound n * TOL * max(1, |u|max) stays beside it; gradients here are 1e-4 .. 5e-3 in size,
so its floor is an absolute 2e-5 that a data gradient through a path of lower precision would pass."""
import collections

import numpy as np
import pytest

import conv_bwd_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu

TOL = 2e-5          # tests/test_gpu_conv.py: one dispatcher result, err <= TOL * max(1, |ref|max)
MARGIN = R.MARGIN    # 16: relative L2 error over that of torch's float32 -- of a dw over the whole chain, of a data gradient per layer
MAX_B, MAX_H, MAX_W = 3, 64, 48
PRIMARY = dict(B=2, H=64, W=48, stages=6, strips=0, seed=2024)
SECONDARY = dict(B=3, H=48, W=40, stages=2, strips=4, seed=2025)          # 18 map rows in strips of 5: every border inside an image
SWEEP = [('conv_algo', 0, 1), ('conv_algo', 1, 1), ('conv_algo', 2, 1), ('ksplit', 2, 0)]


def _weights():
    return pkg('weights').synthetic_weights(0)


@pytest.fixture(scope='module')
def eng(native):
    e = native.Engine(0, max_batch=MAX_B, max_h=MAX_H, max_w=MAX_W)
    e.set_weights(_weights())
    yield e
    e.close()


def _data(B, H, W, seed, **_):
    rng = np.random.default_rng(seed)
    imgs = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    poses = []
    for n in ([2, 1, 3])[:B]:
        p = np.zeros((n, 18, 3))
        p[:, :, 0] = rng.uniform(2, W - 2, (n, 18))
        p[:, :, 1] = rng.uniform(2, H - 2, (n, 18))
        p[:, :, 2] = rng.integers(0, 3, (n, 18))
        poses.append(p)
    masks = np.zeros((B, H, W), bool)
    masks[1, 10:40, 8:30] = True          # a non-trivial ignore mask on one image
    return imgs, poses, masks


# ---- the head's graph -------------------------------------------------------------------------------------------------------------------
def _head(n):
    """name -> dict(x = the layers whose outputs, in the reference's channel order, are the layer's input; relu; out = (stage, branch) for a
    stage output) of the layers after conv4_2 that a forward of n stages runs, in the forward's order per branch."""
    L = collections.OrderedDict()
    L['conv4_3_CPM'] = dict(x=['conv4_2'], relu=True, stage=0, out=None)
    L['conv4_4_CPM'] = dict(x=['conv4_3_CPM'], relu=True, stage=0, out=None)
    for b, br in enumerate(('L1', 'L2')):
        prev = 'conv4_4_CPM'
        for i in range(1, 6):
            nm = 'conv5_%d_CPM_%s' % (i, br)
            L[nm] = dict(x=[prev], relu=i < 5, stage=1, out=(1, b) if i == 5 else None)
            prev = nm
    for s in range(2, n + 1):
        outs = ['conv5_5_CPM_L1', 'conv5_5_CPM_L2'] if s == 2 else ['Mconv7_stage%d_L1' % (s - 1), 'Mconv7_stage%d_L2' % (s - 1)]
        for b, br in enumerate(('L1', 'L2')):
            prev = None
            for i in range(1, 8):
                nm = 'Mconv%d_stage%d_%s' % (i, s, br)
                L[nm] = dict(x=outs + ['conv4_4_CPM'] if i == 1 else [prev], relu=i < 7, stage=s, out=(s, b) if i == 7 else None)
                prev = nm
    return L


# ---- one retained forward + backward, everything fetched ---------------------------------------------------------------------------------
def _run(eng, cfg, options=(), fetch=True):
    imgs, poses, masks = _data(**cfg)
    n = cfg['stages']
    eng.loss_set_poses(poses, cfg['H'], cfg['W'], masks, 7, 8)
    eng.set_option('stop_stage', n)
    eng.set_option('wgrad_strips', cfg['strips'])
    for key, val, _ in options:
        eng.set_option(key, val)
    eng.loss_grad_enable(True)
    eng.backward_enable(True)
    try:
        total, paf, heat = eng.validate_batch(imgs)
        out = dict(cfg=cfg, total=total, paf=paf, heat=heat, maps=eng.get_maps(), lg=[eng.loss_grads(s) for s in range(n)])
        eng.backward_head()
        names = list(_head(n))
        assert names and sorted(names) == sorted(eng.head_layers(n))
        out['dw'], out['db'] = {}, {}
        for nm in names:
            out['dw'][nm], out['db'][nm] = eng.layer_grad(nm)
        out['trunk'] = eng.trunk_grad()
        if fetch:
            out['a'] = {nm: eng.retained(nm, 0) for nm in names + ['conv4_2']}
            out['g'] = {nm: eng.retained(nm, 1) for nm in names}
        out['maps_after'] = eng.get_maps()
    finally:
        eng.backward_enable(False)
        eng.loss_grad_enable(False)
        for key, _, default in options:
            eng.set_option(key, default)
        eng.set_option('stop_stage', 6)
        eng.set_option('wgrad_strips', 0)
    return out


_runs = {}


def _cached(eng, key):
    """the runs the tests share, made once: 'primary', 'secondary', ('sweep', i)"""
    if key not in _runs:
        if key == 'primary':
            _runs[key] = _run(eng, PRIMARY)
        elif key == 'secondary':
            _runs[key] = _run(eng, SECONDARY)
        else:
            _runs[key] = _run(eng, PRIMARY, options=[SWEEP[key[1]]])
    return _runs[key]


def _refs(run):
    """float64 references of every layer of a run, from the run's own retained arrays (computed once per run): x, (dx64, dw64, db64) of
    conv_grads64(g, x, w) and u64 = the sum of the consumers' dx64 slices + the loss gradient at a stage output, n = the consumers; dx32 =
    torch's float32 data gradient for the same g, and u32 = the same sum of dx32 slices made of float32 adds in the order of THE SUMS of the
    header: the loss gradient first, then the consumers as the backward reaches them (the last stage first, L1 before L2)."""
    if 'refs' in run:
        return run['refs']
    W = _weights()
    head = _head(run['cfg']['stages'])
    refs = {}
    for nm, d in head.items():
        x = np.concatenate([run['a'][p] for p in d['x']], axis=1)
        refs[nm] = dict(x=x, grads=R.conv_grads64(run['g'][nm], x, W[nm][0]), n=0, dx32=R.dx_pair(run['g'][nm], W[nm][0])[1].astype(np.float32))
    for nm, d in head.items():
        if d['out'] is not None:
            s, b = d['out']
            refs[nm]['u64'] = run['lg'][s - 1][b].astype(np.float64)
            refs[nm]['u32'] = run['lg'][s - 1][b].copy()
        else:
            refs[nm]['u64'] = np.zeros(run['a'][nm].shape)
    for nm, d in head.items():
        off = 0
        for p in d['x']:
            c = run['a'][p].shape[1]
            if p in refs:
                refs[p]['u64'] = refs[p]['u64'] + refs[nm]['grads'][0][:, off:off + c]
                refs[p]['n'] += 1
            off += c
    for nm in sorted(head, key=lambda nm: (-head[nm]['stage'], nm.endswith('_L2'))):          # (stable: the forward's order within a branch)
        off = 0
        for p in head[nm]['x']:
            c = run['a'][p].shape[1]
            if p in refs:
                part = refs[nm]['dx32'][:, off:off + c]
                refs[p]['u32'] = refs[p]['u32'] + part if 'u32' in refs[p] else part.copy()
                assert refs[p]['u32'].dtype == np.float32
            off += c
    run['refs'] = refs
    return refs


def _check_layers(run, stage):
    W = _weights()
    cfg = run['cfg']
    head = _head(cfg['stages'])
    refs = _refs(run)
    names = [nm for nm, d in head.items() if d['stage'] == stage]
    assert names
    for nm in names:
        d, r = head[nm], refs[nm]
        w = W[nm][0]
        k = w.shape[-1]
        a, g, dw, db = run['a'][nm], run['g'][nm], run['dw'][nm], run['db'][nm]
        for what, arr in (('a', a), ('g', g), ('dw', dw), ('db', db)):
            assert np.isfinite(arr).all(), 'unwritten (poisoned) or non-finite %s of %s' % (what, nm)
        assert dw.shape == w.shape and g.shape == a.shape
        dx64, dw64, db64 = r['grads']
        twin = R.wgrad_twin(g, r['x'], k, cfg['strips'])
        err = np.abs(dw.astype(np.float64) - dw64)
        bound = R.dw_bound(g, r['x'], w, dw64)
        edb = np.abs(db.astype(np.float64) - db64)
        sel = a > 0 if d['relu'] else np.ones(a.shape, bool)
        u64 = r['u64']
        eu = np.abs(g.astype(np.float64) - u64)[sel].max() if sel.any() else 0.0
        ubound = r['n'] * TOL * max(1.0, np.abs(u64).max())
        # g over torch's float32 against float64, on the open gates (closed: zero in all three)
        ur = R.ratio(np.where(sel, g, 0), np.where(sel, u64, 0), np.where(sel, r['u32'], 0)) if r['n'] else (0.0, 0.0, 0.0)
        print(nm, 'dw != twin', int((dw != twin).sum()), 'dw err / bound', float((err / np.maximum(bound, 1e-300)).max()),
              'db', float((edb / np.maximum(np.abs(db64), 1e-300)).max()), 'u', eu, 'bound', ubound, 'n', r['n'], 'gates open', float(sel.mean()),
              'u r_l2 %.3f r_max %.3f rel. L2 %.3e' % ur)
        assert np.array_equal(dw, twin), (nm, int((dw != twin).sum()))
        assert (err <= bound).all(), nm
        assert (edb <= 2.0 ** -23 * np.abs(db64)).all(), nm
        assert not g.view(np.uint32)[~sel].any(), nm          # +0.0f by bits where a > 0 is false
        assert g[sel].any(), nm
        if r['n'] == 0:          # the last stage's outputs: the loss gradient itself
            s, b = d['out']
            assert s == cfg['stages'] and np.array_equal(g.view(np.uint32), run['lg'][s - 1][b].view(np.uint32)), nm
        else:
            assert r['n'] == (2 if d['out'] is not None else 2 * cfg['stages'] if nm == 'conv4_4_CPM' else 1), (nm, r['n'])
            assert eu <= ubound, (nm, eu, ubound)
            assert ur[0] <= MARGIN and ur[1] <= MARGIN, (nm, ur)
    if stage == 0:
        dx64 = refs['conv4_3_CPM']['grads'][0]
        et = np.abs(run['trunk'] - dx64).max()
        tr = R.ratio(run['trunk'], dx64, refs['conv4_3_CPM']['dx32'])
        print('trunk_grad', et, np.abs(dx64).max(), 'r_l2 %.3f r_max %.3f rel. L2 %.3e' % tr)
        assert np.isfinite(run['trunk']).all() and run['trunk'].shape == dx64.shape
        assert et <= TOL * max(1.0, np.abs(dx64).max())
        assert tr[0] <= MARGIN and tr[1] <= MARGIN, tr


@pytest.mark.parametrize('stage', range(7))
def test_every_layer_of_the_primary_case(eng, stage):
    _check_layers(_cached(eng, 'primary'), stage)


@pytest.mark.parametrize('stage', range(3))
def test_every_layer_with_stop_stage_and_forced_strips(eng, stage):
    run = _cached(eng, 'secondary')
    assert R.strips_for(3, 6, 128, 128, 7, 4) == (4, 5)
    _check_layers(run, stage)


@pytest.mark.parametrize('stage', range(7))
@pytest.mark.parametrize('opt', range(len(SWEEP)))
def test_layers_under_the_forward_options(eng, opt, stage):
    """The kernel form of every data gradient follows the options; each dw is the twin of THAT run's g and x (Mconv2_stage2_L1 among them)."""
    run = _cached(eng, ('sweep', opt))
    _check_layers(run, stage)
    if stage == 2:
        r = _refs(run)['Mconv2_stage2_L1']
        assert np.array_equal(run['dw']['Mconv2_stage2_L1'], R.wgrad_twin(run['g']['Mconv2_stage2_L1'], r['x'], 7, 0))


# ---- the whole chain ---------------------------------------------------------------------------------------------------------------------
def _torch_grads(imgs, targets, n, dtype):
    """autograd of the total loss of the whole network in `dtype` on the CPU -> {head layer: dW float64}"""
    import torch
    import torch.nn.functional as F
    W = _weights()
    head = _head(n)
    P = {}
    for nm, (w, b) in W.items():
        P[nm] = (torch.tensor(w, dtype=dtype, requires_grad=nm in head), torch.tensor(b, dtype=dtype))

    def conv(nm, h, relu=True):
        h = F.conv2d(h, P[nm][0], P[nm][1], padding=P[nm][0].shape[-1] // 2)
        return F.relu(h) if relu else h
    t_p, t_h, t_m = targets
    keep = torch.tensor(~t_m[:, None])
    tp, th = torch.tensor(t_p, dtype=dtype), torch.tensor(t_h, dtype=dtype)
    h = torch.tensor(imgs.transpose(0, 3, 1, 2).copy()).to(dtype) / 255 - 0.5
    for blk in (('conv1_1', 'conv1_2'), ('conv2_1', 'conv2_2'), ('conv3_1', 'conv3_2', 'conv3_3', 'conv3_4')):
        for nm in blk:
            h = conv(nm, h)
        h = F.max_pool2d(h, 2, 2)
    for nm in ('conv4_1', 'conv4_2', 'conv4_3_CPM', 'conv4_4_CPM'):
        h = conv(nm, h)
    feat = h
    h1 = h2 = feat
    for i in range(1, 6):
        h1, h2 = conv('conv5_%d_CPM_L1' % i, h1, i < 5), conv('conv5_%d_CPM_L2' % i, h2, i < 5)
    loss = (((h1 - tp) * keep) ** 2).mean() + (((h2 - th) * keep) ** 2).mean()
    for s in range(2, n + 1):
        h1 = h2 = torch.cat((h1, h2, feat), dim=1)
        for i in range(1, 8):
            h1, h2 = conv('Mconv%d_stage%d_L1' % (i, s), h1, i < 7), conv('Mconv%d_stage%d_L2' % (i, s), h2, i < 7)
        loss = loss + (((h1 - tp) * keep) ** 2).mean() + (((h2 - th) * keep) ** 2).mean()
    loss.backward()
    return {nm: P[nm][0].grad.double().numpy() for nm in head}


def test_whole_chain_against_float64_autograd(eng):
    """Relative L2 error of every dw against float64 torch autograd of the whole network; the yardstick is the same error of torch's own
    float32 autograd, the margin 16 x per tensor (the Winograd forms over a direct fp32 sum; near-zero ReLU gates flip in either run)."""
    import torch
    run = _cached(eng, 'primary')
    imgs, poses, masks = _data(**PRIMARY)
    eng.loss_set_poses(poses, PRIMARY['H'], PRIMARY['W'], masks, 7, 8)
    targets = eng.loss_targets()
    g64 = _torch_grads(imgs, targets, 6, torch.float64)
    g32 = _torch_grads(imgs, targets, 6, torch.float32)
    head = _head(6)
    worst = collections.defaultdict(lambda: (0.0, 0.0, 0.0, ''))
    bad = []
    for nm, d in head.items():
        ref = g64[nm]
        nrm = np.sqrt((ref ** 2).sum())
        assert nrm > 0, nm
        e_lib = np.sqrt(((run['dw'][nm].astype(np.float64) - ref) ** 2).sum()) / nrm
        e_t32 = np.sqrt(((g32[nm] - ref) ** 2).sum()) / nrm
        ratio = e_lib / e_t32
        if ratio > worst[d['stage']][0]:
            worst[d['stage']] = (ratio, e_lib, e_t32, nm)
        if not e_lib <= MARGIN * e_t32:
            bad.append((nm, e_lib, e_t32, ratio))
    for s in sorted(worst):
        print('stage %d: worst ratio %.3f (library %.3e, torch float32 %.3e) at %s' % ((s,) + worst[s]))
    print('maximum ratio', max(v[0] for v in worst.values()))
    assert not bad, bad


# ---- further checks -----------------------------------------------------------------------------------------------------------------------
def test_forward_keeps_its_bits_with_retention_on(eng):
    run = _cached(eng, 'primary')
    imgs, poses, masks = _data(**PRIMARY)
    eng.loss_set_poses(poses, PRIMARY['H'], PRIMARY['W'], masks, 7, 8)
    eng.loss_grad_enable(True)
    try:
        total, paf, heat = eng.validate_batch(imgs)          # retention off
        maps = eng.get_maps()
        lg = [eng.loss_grads(s) for s in range(6)]
    finally:
        eng.loss_grad_enable(False)
    assert total == run['total'] and np.array_equal(paf, run['paf']) and np.array_equal(heat, run['heat'])
    for i in (0, 1):
        assert np.array_equal(maps[i].view(np.uint32), run['maps'][i].view(np.uint32))
        assert np.array_equal(maps[i].view(np.uint32), run['maps_after'][i].view(np.uint32))          # the backward restores the last stage's maps
        for s in range(6):
            assert np.array_equal(lg[s][i].view(np.uint32), run['lg'][s][i].view(np.uint32)), s


def test_same_bits_on_every_run(eng):
    run = _cached(eng, 'primary')
    again = _run(eng, PRIMARY, fetch=False)
    for nm in run['dw']:
        assert np.array_equal(run['dw'][nm].view(np.uint32), again['dw'][nm].view(np.uint32)), nm
        assert np.array_equal(run['db'][nm].view(np.uint32), again['db'][nm].view(np.uint32)), nm
    assert np.array_equal(run['trunk'].view(np.uint32), again['trunk'].view(np.uint32))


def test_error_codes(native, eng):
    run = _cached(eng, 'primary')
    imgs, poses, masks = _data(**PRIMARY)
    H, W = PRIMARY['H'], PRIMARY['W']

    def refused(code, fn, *args):
        with pytest.raises(native.PmxError) as e:
            fn(*args)
        assert e.value.code == code, (e.value.code, str(e.value))

    refused(6, eng.backward_head)                           # retention off
    eng.loss_set_poses(poses, H, W, masks, 7, 8)
    eng.loss_grad_enable(True)
    eng.backward_enable(True)
    try:
        refused(6, eng.backward_head)                       # on, no retained forward yet
        refused(6, eng.layer_grad, 'conv4_3_CPM')
        refused(6, eng.trunk_grad)
        refused(6, eng.retained, 'conv4_2')
        eng.validate_batch(imgs)
        refused(6, eng.layer_grad, 'conv4_3_CPM')           # retained, but no backward yet
        refused(6, eng.retained, 'conv4_3_CPM', 1)
        assert eng.retained('conv4_2').shape == (2, 512, H // 8, W // 8)
        eng.forward_u8(imgs)                                # a forward since then that was not retained
        refused(6, eng.backward_head)
        eng.validate_batch(imgs)
        eng.set_option('precision', 2)
        try:
            refused(6, eng.backward_head)                   # fp32 only
        finally:
            eng.set_option('precision', 0)
        eng.backward_head()                                 # the context stays usable: the same bits as the shared run
        refused(1, eng.layer_grad, 'no_such_layer')
        refused(1, eng.layer_grad, 'conv4_2')               # a trunk layer
        refused(1, eng.retained, 'no_such_layer')
        refused(1, eng.retained, 'conv4_2', 1)
        refused(1, eng.retained, 'conv4_3_CPM', 2)
        assert eng.lib.pmx_get_layer_grad(eng._ctx, b'conv4_3_CPM', None, None) == 1
        assert eng.lib.pmx_get_trunk_grad(eng._ctx, None) == 1
        assert eng.lib.pmx_get_retained(eng._ctx, b'conv4_3_CPM', 0, None) == 1
        for nm in ('conv4_3_CPM', 'Mconv1_stage2_L2', 'Mconv7_stage6_L1'):
            dw, db = eng.layer_grad(nm)
            assert np.array_equal(dw.view(np.uint32), run['dw'][nm].view(np.uint32)) and np.array_equal(db.view(np.uint32), run['db'][nm].view(np.uint32)), nm
        eng.set_option('stop_stage', 2)
        try:
            eng.validate_batch(imgs)
            eng.backward_head()
            refused(6, eng.layer_grad, 'Mconv1_stage3_L1')  # a stage that stop_stage cut off
            refused(6, eng.retained, 'Mconv7_stage6_L2')
            assert np.isfinite(eng.layer_grad('Mconv7_stage2_L2')[0]).all()
        finally:
            eng.set_option('stop_stage', 6)
    finally:
        eng.backward_enable(False)
        eng.loss_grad_enable(False)
    face = native.Engine(0, max_batch=1, max_h=64, max_w=64, arch='facenet')
    try:
        refused(6, face.backward_enable, True)
        refused(6, face.backward_head)
    finally:
        face.close()


def test_pose_detector_head_gradients(native, eng):
    run = _cached(eng, 'primary')
    PD = pkg('pose_detector')
    imgs, poses, masks = _data(**PRIMARY)
    det = PD.PoseDetector(weights=_weights(), device=0, max_batch=PRIMARY['B'], max_size=(PRIMARY['H'], PRIMARY['W']))
    out = det.head_gradients(list(imgs), poses, list(masks))
    assert out['val/loss'] == run['total']
    for s in range(6):
        assert np.array_equal(out['paf_grads'][s], run['lg'][s][0]) and np.array_equal(out['heat_grads'][s], run['lg'][s][1])
    assert sorted(out['grads']) == sorted(run['dw']) and len(out['grads']) == 82
    for nm, (dw, db) in out['grads'].items():
        assert np.array_equal(dw.view(np.uint32), run['dw'][nm].view(np.uint32)) and np.array_equal(db.view(np.uint32), run['db'][nm].view(np.uint32)), nm
    assert np.array_equal(out['trunk_grad'].view(np.uint32), run['trunk'].view(np.uint32))
    with pytest.raises(ValueError):
        det.head_gradients(list(imgs) * 2, poses * 2, list(masks) * 2)          # more than max_batch images
