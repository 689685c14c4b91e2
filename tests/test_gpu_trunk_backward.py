"""GPU: the trunk backward (include/pose_mi355x.h: pmx_backward_enable(ctx, 2) / pmx_backward_trunk) -- the gradients of conv1_1 .. conv4_2.
The whole chain against float64 torch autograd of the full network with torch's own float32 autograd as the yardstick; per layer, from the
library's own retained arrays, dw bit for bit against the order-defined host twin; the pool kernels and conv1_1's weight-gradient kernel
through their test entries on the integer lattice (the figures of a run: EXPERIMENTS.md E39).
Pinned per layer, under conv_algo 1, 0 and 2 in both cases (test_every_trunk_layer_s_output_and_upstream_gradient; figures: E40): the
prepared input by bits against the documented formula; every retained output a against relu(conv(x) + b) of the layer's own input x, and
every upstream gradient g against the masked or pool-scattered data gradient of the layer after it, both in float64 torch with torch's
float32 result as the yardstick (conv_bwd_ref.ratio, at most MARGIN in L2 and in the maximum); g of conv4_2 by bits against the masked
trunk gradient of the head."""
import numpy as np
import pytest

import adam_twin as A
import conv_bwd_ref as R
import test_gpu_head_backward as HB
import trunk_backward_ref as T
from conftest import pkg
from oracle import postprocess_ref as P

pytestmark = pytest.mark.gpu

MARGIN = HB.MARGIN      # relative L2 error over that of torch's float32 (the head test's margin): of a gradient over the whole chain, of an
                        # output or an upstream gradient per layer
TOL = HB.TOL            # one dispatcher result: err <= TOL * max(1, |ref|max)
MAX_B, MAX_H, MAX_W = 3, 64, 48
CASES = {'primary': dict(B=2, H=64, W=48, stages=6, seed=2024),          # the head test's primary case
         'secondary': dict(B=3, H=40, W=56, stages=6, seed=2026)}        # level 3 is 5 x 7: every level has partial tiles
# (case, "wgrad_strips", "conv_algo"): both cases under the rule, with strip borders inside images, and under every forward form
RUNS = [(c, s, 1) for c in CASES for s in (0, 3, 5)] + [(c, 0, a) for c in CASES for a in (0, 2)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope='module')
def eng(native):
    e = native.Engine(0, max_batch=MAX_B, max_h=MAX_H, max_w=MAX_W)
    e.set_weights(HB._weights())
    yield e
    e.close()


def _run(eng, case, strips=0, algo=1, fetch=True):
    """one mode-2 forward + backward_head + backward_trunk; all 92 gradients and, with fetch, the trunk's retained arrays"""
    cfg = CASES[case]
    imgs, poses, masks = HB._data(**cfg)
    eng.loss_set_poses(poses, cfg['H'], cfg['W'], masks, 7, 8)
    eng.set_option('wgrad_strips', strips)
    eng.set_option('conv_algo', algo)
    eng.set_option('trunk_keep_g', 1)
    eng.loss_grad_enable(True)
    eng.backward_enable(2)
    try:
        total, paf, heat = eng.validate_batch(imgs)
        out = dict(cfg=cfg, strips=strips, total=total, paf=paf, heat=heat, maps=eng.get_maps())
        eng.backward_head()
        eng.backward_trunk()
        names = T.NAMES + eng.head_layers(6)
        assert len(names) == 92
        out['dw'], out['db'] = {}, {}
        for nm in names:
            out['dw'][nm], out['db'][nm] = eng.layer_grad(nm)
        out['trunk'] = eng.trunk_grad()
        if fetch:
            out['input'] = eng.retained('input', 0)
            out['a'] = {nm: eng.retained(nm, 0) for nm in T.NAMES}
            out['g'] = {nm: eng.retained(nm, 1) for nm in T.NAMES}
            out['pooled'] = {nm: eng.retained(nm, 2) for nm in T.POOLED}
    finally:
        eng.backward_enable(False)
        eng.loss_grad_enable(False)
        eng.set_option('wgrad_strips', 0)
        eng.set_option('conv_algo', 1)
        eng.set_option('trunk_keep_g', 0)
    return out


_runs = {}


def _cached(eng, key):
    if key not in _runs:
        _runs[key] = _run(eng, *key)
    return _runs[key]


# ---- 1. the whole chain ------------------------------------------------------------------------------------------------------------------
def _torch_grads(imgs, targets, dtype):
    """autograd of the total loss of the whole six-stage network in `dtype` on the CPU -> {trunk layer: (dW, db) float64}.  The network of
    test_gpu_head_backward._torch_grads with the trunk's weights AND biases as leaves."""
    import torch
    import torch.nn.functional as F
    W = HB._weights()
    P = {nm: (torch.tensor(w, dtype=dtype, requires_grad=nm in T.NAMES), torch.tensor(b, dtype=dtype, requires_grad=nm in T.NAMES)) for nm, (w, b) in W.items()}

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
    for s in range(2, 7):
        h1 = h2 = torch.cat((h1, h2, feat), dim=1)
        for i in range(1, 8):
            h1, h2 = conv('Mconv%d_stage%d_L1' % (i, s), h1, i < 7), conv('Mconv%d_stage%d_L2' % (i, s), h2, i < 7)
        loss = loss + (((h1 - tp) * keep) ** 2).mean() + (((h2 - th) * keep) ** 2).mean()
    loss.backward()
    return {nm: (P[nm][0].grad.double().numpy(), P[nm][1].grad.double().numpy()) for nm in T.NAMES}


@pytest.mark.parametrize('case', list(CASES))
def test_whole_chain_against_float64_autograd(eng, case):
    """Relative L2 error of the ten trunk dw and db against float64 torch autograd of the whole network over the same error of torch's own
    float32 autograd: at most 16, the head test's margin for the same reason (other summation orders and kernel forms than a direct fp32
    sum; near-zero ReLU gates and pool ties flip in either float32 run)."""
    import torch
    run = _cached(eng, (case, 0, 1))
    cfg = CASES[case]
    imgs, poses, masks = HB._data(**cfg)
    eng.loss_set_poses(poses, cfg['H'], cfg['W'], masks, 7, 8)
    targets = eng.loss_targets()
    g64 = _torch_grads(imgs, targets, torch.float64)
    g32 = _torch_grads(imgs, targets, torch.float32)
    bad = []
    for nm in T.NAMES:
        for k, what in enumerate(('dw', 'db')):
            ref = g64[nm][k]
            nrm = np.sqrt((ref ** 2).sum())
            assert nrm > 0, (nm, what)
            e_lib = np.sqrt(((run[what][nm].astype(np.float64) - ref) ** 2).sum()) / nrm
            e_t32 = np.sqrt(((g32[nm][k] - ref) ** 2).sum()) / nrm
            print('%s %s %s: ratio %.3f (library %.3e, torch float32 %.3e)' % (case, nm, what, e_lib / e_t32, e_lib, e_t32))
            if not e_lib <= MARGIN * e_t32:
                bad.append((nm, what, e_lib, e_t32))
    assert not bad, bad


# ---- 2. every layer from the library's own retained arrays ------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,strips,algo', RUNS)
def test_every_trunk_layer_against_the_twin(eng, case, strips, algo):
    run = _cached(eng, (case, strips, algo))
    cfg = CASES[case]
    B, H = cfg['B'], cfg['H']
    assert np.isfinite(run['input']).all() and run['input'].shape == (B, 3, H, cfg['W'])
    for t, (nm, cin, cout, level, pool) in enumerate(T.TRUNK):
        a, g, dw, db = run['a'][nm], run['g'][nm], run['dw'][nm], run['db'][nm]
        x = _x_of(run, t)
        assert a.shape == g.shape == (B, cout, H >> level, cfg['W'] >> level) and x.shape[1] == cin and dw.shape == (cout, cin, 3, 3), nm
        for what, arr in (('a', a), ('g', g), ('dw', dw), ('db', db)):
            assert np.isfinite(arr).all(), 'unwritten (poisoned) or non-finite %s of %s' % (what, nm)
        s, r, _ = T.trunk_strips(nm, B, H, strips)
        twin = T.wgrad_twin(g, x, s, r)
        print(case, strips, algo, nm, 'strips', s, 'rows', r, 'dw != twin', int((_bits(dw) != _bits(twin)).sum()), 'gates open', float((a > 0).mean()))
        assert np.array_equal(_bits(dw), _bits(twin)), (nm, int((_bits(dw) != _bits(twin)).sum()))
        db64 = g.astype(np.float64).sum(axis=(0, 2, 3))
        assert (np.abs(db.astype(np.float64) - db64) <= 2.0 ** -23 * np.abs(db64)).all(), nm
        assert not _bits(g)[~(a > 0)].any(), nm                         # +0.0f by bits where a > 0 is false
        assert g.any(), nm
        if pool:
            pooled = run['pooled'][nm]
            assert np.array_equal(pooled, T.windows(a).max(axis=-1)), nm
            gw = T.windows(g)
            assert ((gw != 0).sum(axis=-1) <= 1).all(), nm
            # the one non-zero of a window sits at the first maximum of a
            first = T.windows(a).argmax(axis=-1)
            assert not np.where(np.arange(4) == first[..., None], 0, gw).any(), nm
    if strips and (case, strips) != ('secondary', 3):          # (three strips of three images end where the images do)
        assert T.trunk_strips('conv1_2', B, H, strips)[1] % H != 0          # a strip border inside an image


# ---- 2b. every layer's output and upstream gradient against float64, torch's float32 as the yardstick ------------------------------------------
def _x_of(run, t):
    """the input of trunk layer t: the prepared input, the pooled map or the output of the layer before it"""
    return run['input'] if t == 0 else run['pooled'][T.NAMES[t - 1]] if T.TRUNK[t - 1][4] else run['a'][T.NAMES[t - 1]]


def _layer_refs(run):
    """(reference, yardstick) pairs of a run from the run's own retained arrays, computed once per run: 'a' of every layer from its own
    input, 'g' of conv1_1 .. conv4_1 from g of the layer after it, gated or scattered by the library's own a (nothing can flip)."""
    if 'layer_refs' not in run:
        W = HB._weights()
        refs = {'a': {}, 'g': {}}
        for t, nm in enumerate(T.NAMES):
            refs['a'][nm] = R.fwd_pair(_x_of(run, t), W[nm][0], W[nm][1], relu=True)
        for t in range(len(T.NAMES) - 2, -1, -1):
            nm, nxt = T.NAMES[t], T.NAMES[t + 1]
            a = run['a'][nm]
            rule = (lambda dx: T.pool_scatter(a, dx)) if T.TRUNK[t][4] else (lambda dx: np.where(a > 0, dx, 0.0))
            refs['g'][nm] = tuple(rule(dx) for dx in R.dx_pair(run['g'][nxt], W[nxt][0]))
        run['layer_refs'] = refs
    return run['layer_refs']


@pytest.mark.parametrize('case,algo', [(c, a) for c in CASES for a in (1, 0, 2)])
def test_every_trunk_layer_s_output_and_upstream_gradient(eng, case, algo):
    """What test_every_trunk_layer_against_the_twin takes as given.  Each quantity is checked on the layer's own inputs as the library
    retained them, so no error carries from layer to layer and no gate or arg-maximum can differ between library, reference and yardstick.
    The prepared input: no other test pins it per element (tests/test_gpu_network.py sees it through the maps), so it is compared here by
    bits with the float32 evaluation of the documented formula, divide by 255, then subtract 0.5 (csrc/prep.hip promises exactly that)."""
    run = _cached(eng, (case, 0, algo))
    cfg = CASES[case]
    imgs = HB._data(**cfg)[0]
    want = np.concatenate([P.preprocess(im) for im in imgs])
    assert want.dtype == np.float32 and np.array_equal(_bits(run['input']), _bits(want)), int((_bits(run['input']) != _bits(want)).sum())
    refs = _layer_refs(run)
    bad = []
    for nm in T.NAMES:
        a = run['a'][nm]
        a64, a32 = refs['a'][nm]
        r_l2, r_max, e = R.ratio(a, a64, a32)
        ea = np.abs(a - a64).max()
        print('%s algo %d %s a: r_l2 %.3f r_max %.3f rel. L2 %.3e max err %.3e |a|max %.3g' % (case, algo, nm, r_l2, r_max, e, ea, np.abs(a64).max()))
        if not (r_l2 <= MARGIN and r_max <= MARGIN and ea <= TOL * max(1.0, np.abs(a64).max())):
            bad.append((nm, 'a', r_l2, r_max, ea))
    top = T.NAMES[-1]
    assert run['trunk'].shape == run['a'][top].shape
    link = np.where(run['a'][top] > 0, run['trunk'], np.float32(0))
    assert link.dtype == np.float32 and np.array_equal(_bits(run['g'][top]), _bits(link)), int((_bits(run['g'][top]) != _bits(link)).sum())
    for nm in T.NAMES[-2::-1]:
        g64, g32 = refs['g'][nm]
        r_l2, r_max, e = R.ratio(run['g'][nm], g64, g32)
        print('%s algo %d %s g: r_l2 %.3f r_max %.3f rel. L2 %.3e |g|max %.3g' % (case, algo, nm, r_l2, r_max, e, np.abs(g64).max()))
        if not (r_l2 <= MARGIN and r_max <= MARGIN):
            bad.append((nm, 'g', r_l2, r_max))
    assert not bad, bad


# ---- 3. the pool kernels on the lattice -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C_,H,W', T.POOL_CASES)
def test_pool_kernels_on_the_lattice(eng, C_, H, W):
    z, a, u, census = T.pool_lattice(C_, H, W)
    for cls in ('tied', 'tied_not_first', 'dead_windows', 'zeros', 'zero_selected', 'unique_1', 'unique_2', 'unique_3'):
        assert census[cls] > 0, (cls, census)
    pooled, g = eng.pool_backward_test(a, u)
    want_g = R.mask_rule(u, z, 1, 1)
    assert np.array_equal(pooled, T.windows(a).max(axis=-1))
    assert np.array_equal(g, want_g) and not _bits(g)[want_g == 0].any()
    tp, tg = T.pool_twin(a, u)
    assert np.array_equal(_bits(pooled), _bits(tp)) and np.array_equal(_bits(g), _bits(tg))


# ---- 4. conv1_1's weight-gradient kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,H,W', [(1, 2, 2), (1, 8, 8), (2, 5, 7), (3, 16, 24)])
def test_conv1_wgrad_kernel(eng, B, H, W):
    rng = np.random.default_rng(B * 1000 + H * 10 + W)
    x = rng.standard_normal((B, 3, H, W)).astype('f')
    g = (rng.standard_normal((B, 64, H, W)) * (rng.random((B, 64, H, W)) < 0.6)).astype('f')
    xl = rng.integers(-1, 2, (B, 3, H, W)).astype('f')
    gl = rng.integers(-2, 3, (B, 64, H, W)).astype('f')
    dw64 = R.conv_grads64(gl, xl, np.zeros((64, 3, 3, 3), 'f'))[1]
    for forced in (0, 1, B * H):
        s, r, _ = T.trunk_strips('conv1_1', B, H, forced)
        dw, s_lib, r_lib = eng.conv1_wgrad(x, g, forced)
        assert (s_lib, r_lib) == (s, r), (forced, s_lib, r_lib, s, r)
        twin = T.wgrad_twin(g, x, s, r)
        assert np.array_equal(_bits(dw), _bits(twin)), (forced, int((_bits(dw) != _bits(twin)).sum()))
        dwl = eng.conv1_wgrad(xl, gl, forced)[0]
        assert np.array_equal(dwl.astype(np.float64), dw64), forced


# ---- 5. the same bits on every run ------------------------------------------------------------------------------------------------------------
def test_same_bits_on_every_run(eng):
    run = _cached(eng, ('primary', 0, 1))
    again = _run(eng, 'primary', fetch=False)
    assert len(run['dw']) == 92
    for nm in run['dw']:
        assert np.array_equal(_bits(run['dw'][nm]), _bits(again['dw'][nm])) and np.array_equal(_bits(run['db'][nm]), _bits(again['db'][nm])), nm


# ---- 6. error codes ---------------------------------------------------------------------------------------------------------------------------
def test_error_codes(native, eng):
    run = _cached(eng, ('primary', 0, 1))
    cfg = CASES['primary']
    imgs, poses, masks = HB._data(**cfg)
    H, W = cfg['H'], cfg['W']

    def refused(code, fn, *args):
        with pytest.raises(native.PmxError) as e:
            fn(*args)
        assert e.value.code == code, (e.value.code, str(e.value))

    refused(6, eng.backward_trunk)                              # retention off
    eng.loss_set_poses(poses, H, W, masks, 7, 8)
    eng.loss_grad_enable(True)
    eng.backward_enable(True)
    try:                                                        # mode 1
        refused(6, eng.backward_enable, 2)                      # 2 while 1 is on
        eng.validate_batch(imgs)
        eng.backward_head()
        refused(6, eng.backward_trunk)                          # mode is not 2
        refused(1, eng.layer_grad, 'conv4_2')                   # mode 1 refuses trunk names as ever
        refused(1, eng.layer_grad, 'conv1_1')
        refused(1, eng.retained, 'conv1_2', 0)
        refused(1, eng.retained, 'conv1_2', 2)
        dw, db = eng.layer_grad('conv4_3_CPM')                  # ... and is usable
        assert np.array_equal(_bits(dw), _bits(run['dw']['conv4_3_CPM']))
    finally:
        eng.backward_enable(False)
    try:                                                        # mode 2 (no "trunk_keep_g")
        eng.backward_enable(2)
        refused(6, eng.backward_enable, 1)                      # 1 while 2 is on
        eng.backward_enable(2)                                  # (the same mode again: nothing happens)
        refused(6, eng.backward_trunk)                          # no retained forward
        refused(6, eng.layer_grad, 'conv1_1')
        eng.validate_batch(imgs)
        refused(6, eng.backward_trunk)                          # the head backward has not run
        eng.backward_head()
        refused(6, eng.layer_grad, 'conv1_1')                   # no trunk backward yet
        refused(6, eng.layer_grad, 'conv4_2')
        eng.set_option('precision', 2)
        try:
            refused(6, eng.backward_trunk)                      # fp32 only
        finally:
            eng.set_option('precision', 0)
        assert eng.retained('conv1_1', 0).shape == (2, 64, H, W)
        assert eng.retained('conv2_2', 2).shape == (2, 128, H // 4, W // 4)
        refused(1, eng.retained, 'conv1_1', 2)                  # not a pooled layer
        refused(1, eng.retained, 'conv4_2', 2)
        refused(1, eng.retained, 'conv4_3_CPM', 2)
        refused(1, eng.retained, 'conv1_1', 3)
        refused(6, eng.retained, 'conv1_1', 1)                  # g before the trunk backward
        eng.backward_trunk()                                    # the context is usable after every refusal: the shared run's bits
        refused(6, eng.retained, 'conv1_1', 1)                  # g is kept with "trunk_keep_g" only
        assert eng.lib.pmx_get_layer_grad(eng._ctx, b'conv1_1', None, None) == 1
        assert eng.lib.pmx_get_retained(eng._ctx, b'conv1_1', 0, None) == 1
        for nm in ('conv1_1', 'conv1_2', 'conv3_4', 'conv4_2', 'conv4_3_CPM', 'Mconv7_stage6_L1'):
            dw, db = eng.layer_grad(nm)
            assert np.array_equal(_bits(dw), _bits(run['dw'][nm])) and np.array_equal(_bits(db), _bits(run['db'][nm])), nm
        eng.forward_u8(imgs)                                    # a forward since then that was not retained
        refused(6, eng.backward_trunk)
        refused(6, eng.layer_grad, 'conv1_1')
    finally:
        eng.backward_enable(False)
        eng.loss_grad_enable(False)
    face = native.Engine(0, max_batch=1, max_h=64, max_w=64, arch='facenet')
    try:
        refused(6, face.backward_enable, 2)
        refused(6, face.backward_trunk)
    finally:
        face.close()


# ---- 7. mode 2 and the head training step -------------------------------------------------------------------------------------------------------
def test_head_training_step_in_mode_2(native):
    cfg = CASES['primary']
    imgs, poses, masks = HB._data(**cfg)
    e = native.Engine(0, max_batch=cfg['B'], max_h=cfg['H'], max_w=cfg['W'])
    try:
        e.set_weights(HB._weights())
        e.loss_set_poses(poses, cfg['H'], cfg['W'], masks, 7, 8)
        e.loss_grad_enable(True)
        e.backward_enable(2)
        e.train_enable(True)
        heads = ('conv4_3_CPM', 'Mconv1_stage2_L2', 'Mconv7_stage6_L1')
        before = {nm: e.get_layer(nm) for nm in heads + tuple(T.NAMES)}
        e.validate_batch(imgs)
        e.backward_head()
        e.backward_trunk()
        grads = {nm: e.layer_grad(nm) for nm in heads + tuple(T.NAMES)}
        e.train_step_head()
        for nm in heads:
            w, b = e.get_layer(nm)
            for got, old, grad in ((w, before[nm][0], grads[nm][0]), (b, before[nm][1], grads[nm][1])):
                want = A.step32(old, np.zeros_like(old), np.zeros_like(old), grad, 1.0, 1)[0]
                assert np.array_equal(_bits(got), _bits(want)), nm
            assert not np.array_equal(_bits(w), _bits(before[nm][0])), nm
        for nm in T.NAMES:
            w, b = e.get_layer(nm)
            assert np.array_equal(_bits(w), _bits(before[nm][0])) and np.array_equal(_bits(b), _bits(before[nm][1])), nm
            dw, db = e.layer_grad(nm)                           # the step consumes the head's gradients and leaves the trunk's
            assert np.array_equal(_bits(dw), _bits(grads[nm][0])) and np.isfinite(dw).all() and dw.any(), nm
        e.validate_batch(imgs)
        e.backward_head()
        e.backward_trunk()                                      # the next backward runs, on the updated head
        dw, _ = e.layer_grad('conv1_1')
        assert np.isfinite(dw).all() and not np.array_equal(_bits(dw), _bits(grads['conv1_1'][0]))
    finally:
        e.close()


# ---- 8. PoseDetector.network_gradients ----------------------------------------------------------------------------------------------------------
def test_pose_detector_network_gradients(eng):
    run = _cached(eng, ('primary', 0, 1))
    cfg = CASES['primary']
    PD = pkg('pose_detector')
    imgs, poses, masks = HB._data(**cfg)
    det = PD.PoseDetector(weights=HB._weights(), device=0, max_batch=cfg['B'], max_size=(cfg['H'], cfg['W']))
    out = det.network_gradients(list(imgs), poses, list(masks))
    assert out['val/loss'] == run['total']
    assert sorted(out['grads']) == sorted(run['dw']) and len(out['grads']) == 92
    for nm, (dw, db) in out['grads'].items():
        assert np.array_equal(_bits(dw), _bits(run['dw'][nm])) and np.array_equal(_bits(db), _bits(run['db'][nm])), nm
    assert np.array_equal(_bits(out['trunk_grad']), _bits(run['trunk']))
    with pytest.raises(ValueError):
        det.network_gradients(list(imgs) * 2, poses * 2, list(masks) * 2)          # more than max_batch images
