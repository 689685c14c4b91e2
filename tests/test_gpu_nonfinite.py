"""GPU: the forward contract for non-finite values (include/pose_mi355x.h): relu(NaN) is NaN, a 2x2 pool with
a NaN input is NaN, +-inf follow IEEE arithmetic -- in every convolution kernel, as in the float reference (oracle/network_ref.py:
F.relu, F.max_pool2d; the reference's CPU path: numpy.maximum, col.max).  fmaxf and v_med3_f32 return the non-NaN operand: a kernel that
uses them for the ReLU turns a NaN activation into 0, for the pool into a neighbour, and a network whose weights hold a NaN after a
diverged training step returns finite maps and a finite loss.

Single layers (tests/nonfinite_cases.py: one case per launch form, NaN / +inf / -inf planted into standard_normal data; the twins'
side of the argument is tests/test_nonfinite_host.py): (a) bit-equal to the plain-C twin, NaN positions included; (b) non-finite
exactly where torch is (direct kernels) / between torch's set and the 2x2-tile bound (Winograd: the transforms share a patch and
compute inf - inf); (c) outside the bound bit-equal to the same launch on the input with the planted values replaced by 0; (d) finite
entries within the files' TOL of torch.  A NaN weight goes through the device packers; the network cases through the trunk, the fused
conv1 launch, the Winograd layers' direct fall-backs and the 1x1 pair kernel, up to the validation loss."""
import numpy as np
import pytest

import nonfinite_cases as NF
from conftest import pkg
from oracle import network_ref as N
from oracle import postprocess_ref as P

pytestmark = pytest.mark.gpu


def _launch(engine, case, x, w, b, relu):
    k, o = case['shape'][5], case['opts']
    for kk in (1, 3, 7):
        engine.set_option('force_variant_k%d' % kk, -1)
    try:
        if case['kind'] == 'direct':
            if o.get('variant') is not None:
                engine.set_option('force_variant_k%d' % k, o['variant'])
            engine.set_option('ksplit', o.get('ksplit', 1))
        else:
            engine.set_option('conv_algo', o['algo'])
            engine.set_option('wino_tail', o.get('tail', -1))
            engine.set_option('wino_unit_g', o.get('unit', 0))
        return engine.conv2d(x, w, b, relu=bool(relu), pool=case['pool'])
    finally:
        engine.set_option('force_variant_k%d' % k, -1)
        engine.set_option('ksplit', 0)
        engine.set_option('conv_algo', 1)                     # (the library's default)
        engine.set_option('wino_tail', -1)
        engine.set_option('wino_unit_g', 0)


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('cid', NF.CASE_IDS)
def test_single_layer_keeps_nonfinite_values(engine, cid, relu):
    case, x, xc, w, b, pos, bump, bound = NF.prepared(cid)
    t, ref = NF.references(cid, relu)
    y = _launch(engine, case, x, w, b, relu)
    y_clean = _launch(engine, case, xc, w, b, relu)
    print('%s relu %d: %d planted, non-finite outputs %d (torch %d, bound %d of %d)'
          % (cid, relu, len(pos), int((~np.isfinite(y)).sum()), int((~np.isfinite(ref)).sum()), int(bound.sum()) * y.shape[1], y.size))
    NF.check_against_contract(case, y, y_clean, t, ref, bound)


@pytest.mark.parametrize('cid', ['v5_k3_ragged', 'v6_k3_pool', 'wino_rect_130', 'wino_rect_k7', 'v1_k1', 'default_k1'])
def test_nan_weight_makes_its_output_channel_nan(engine, cid):
    """One NaN at a centre tap W[co, ci, k/2, k/2] (no window leaves it to the padding), clean x, relu = 1: output channel co is all
    NaN -- the direct and the Winograd packs (G g G^T of a NaN tap is NaN in all 16 frequencies) of the device packers carry it --,
    every other channel is bit-equal to the clean run, and the whole output equals the twin.  The transposed packs: the next test."""
    case = NF.CASES[NF.CASE_IDS.index(cid)]
    x, w, b = NF.data(case)
    B, cin, H, W, cout, k = case['shape']
    co, ci = cout - 2, cin - 3
    y_clean = _launch(engine, case, x, w, b, 1)
    wn = w.copy()
    wn[co, ci, k // 2, k // 2] = np.nan
    y = _launch(engine, case, x, wn, b, 1)
    assert np.isfinite(y_clean).all()
    assert np.isnan(y[:, co]).all(), (cid, int(np.isnan(y[:, co]).sum()), y[:, co].size)
    rest = np.arange(cout) != co
    assert np.array_equal(y[:, rest], y_clean[:, rest]), cid
    assert np.array_equal(y, NF.twin(case, x, wn, b, 1), equal_nan=True), cid


@pytest.mark.parametrize('k,cin,cout,H,W,B,algo', [(3, 48, 64, 10, 12, 2, 0), (3, 128, 64, 10, 12, 2, 2), (7, 40, 64, 9, 13, 1, 0),
                                                    (7, 128, 64, 9, 13, 1, 2), (1, 100, 38, 9, 13, 1, 0)])
def test_nan_weight_reaches_the_data_gradient_through_the_transposed_pack(engine, k, cin, cout, H, W, B, algo):
    """pmx_conv2d_backward's data gradient is the forward of the TRANSPOSED layer (w'[ci][co] = w[co][ci] flipped), packed by the device
    packers in the direct form (conv_algo 0) or the Winograd form (conv_algo 2, where the transposed layer has 64 input and 128 output channels).  One
    NaN at the centre tap W[co, ci] (relu = pool = 0, so g = dy in both runs): dx is NaN exactly where torch's float32 data gradient
    is -- all of input channel ci --, and every other input channel is bit-equal to the run with clean weights."""
    import conv_bwd_ref
    rng = np.random.default_rng(8000 + 10 * k + algo)
    x = rng.standard_normal((B, cin, H, W)).astype('f')
    w = (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype('f')
    dy = rng.standard_normal((B, cout, H, W)).astype('f')
    co, ci = cout - 2, cin - 3
    wn = w.copy()
    wn[co, ci, k // 2, k // 2] = np.nan
    for kk in (1, 3, 7):
        engine.set_option('force_variant_k%d' % kk, -1)
    out = {}
    try:
        for a in sorted({0, algo}):
            engine.set_option('conv_algo', a)
            out[a] = engine.conv2d_backward(x, w, None, dy, want=('dx',))['dx']
        dx = engine.conv2d_backward(x, wn, None, dy, want=('dx',))['dx']
    finally:
        engine.set_option('conv_algo', 1)
    dx64, dx32 = conv_bwd_ref.dx_pair(dy, wn)
    nan = np.zeros(x.shape, bool)
    nan[:, ci] = True
    assert np.array_equal(np.isnan(dx32), nan) and np.array_equal(np.isnan(dx64), nan)
    if algo:
        assert not np.array_equal(out[algo], out[0]), 'the Winograd kernel did not run the data gradient'
    clean = out[algo]
    assert np.isfinite(clean).all()
    assert np.array_equal(np.isnan(dx), nan) and not np.isinf(dx).any(), (int(np.isnan(dx).sum()), int(nan.sum()))
    assert np.array_equal(dx[~nan], clean[~nan])
    assert np.abs(clean[~nan] - dx64[~nan]).max() <= NF.TOL * max(1.0, np.abs(dx64[~nan]).max())


# the direct form of the fused conv1 launch (conv1_fused_kernel) takes conv1_2 on 8 x 16 tiles, which the selection picks from two tiles
# per CU on (conv_mfma.hip::conv_pick_variant): two images of 184 x 184 are 552 tiles; below that conv1_1 and conv1_2 run as two launches
DIRECT_FUSED = (2, 184, 184)


def _net(native, B, hw=(64, 96)):
    h, wd = hw
    w = pkg('weights').synthetic_weights(0)
    eng = native.Engine(0, max_batch=B, max_h=h, max_w=wd)
    eng.set_weights(w)
    imgs = np.random.default_rng(60 + B).integers(0, 256, (B, h, wd, 3), dtype=np.uint8)
    x = np.concatenate([P.preprocess(im) for im in imgs])
    eng.loss_set_poses([np.zeros((0, 18, 3))] * B, h, wd)
    return w, eng, imgs, x


@pytest.mark.parametrize('layer,B', [(l, B) for l in ('conv4_2', 'conv1_1', 'Mconv3_stage2_L1') for B in (1, 2)] + [('conv1_1/direct', 2)])
def test_network_nan_weight_reaches_maps_and_loss(native, layer, B):
    """One NaN in a centre tap of a ReLU'd layer -- what a diverged training step leaves behind: the last-stage maps are NaN exactly
    where oracle/network_ref's are on the same weights (everywhere), the stage losses are NaN from the first stage the layer feeds
    (conv4_2, conv1_1: all six of both branches; Mconv3_stage2_L1: the PAF loss of stage 2, both from stage 3) and so is the total; with the clean weights set again the context
    returns its old maps bit for bit.  conv1_1 runs inside the fused conv1 launch, in its Winograd form (conv1_wino_kernel, option
    conv1_wino = 2) and, 'conv1_1/direct', in its direct form (conv1_fused_kernel, conv1_wino = 0, two images of 184 x 184)."""
    layer, form = (layer.split('/') + [''])[:2]
    w, eng, imgs, x = _net(native, B, DIRECT_FUSED[1:] if form else (64, 96))
    try:
        if layer == 'conv1_1':
            eng.set_option('conv1_wino', 0 if form else 2)
        total0, p0, h0 = eng.validate_batch(imgs)
        paf0, heat0 = eng.get_maps()
        assert np.isfinite(paf0).all() and np.isfinite(heat0).all() and np.isfinite(total0) and np.isfinite(p0).all() and np.isfinite(h0).all()
        Wn, bn = w[layer][0].copy(), w[layer][1]
        k = Wn.shape[2]
        Wn[5, 1, k // 2, k // 2] = np.nan
        eng.set_layer(layer, Wn, bn)
        eng.profile_reset(); eng.profile_enable(True)
        total, p, h = eng.validate_batch(imgs)
        kernels = {e['kernel'] for e in eng.profile()}
        eng.profile_enable(False)
        paf, heat = eng.get_maps()
        assert any('pair' in kn for kn in kernels), kernels
        if layer == 'conv1_1':
            ran = (any(kn.startswith('conv_wino1_') for kn in kernels), any('conv1_fused' in kn for kn in kernels))
            assert ran == ((False, True) if form else (True, False)), kernels
        wn = dict(w)
        wn[layer] = (Wn, bn)
        stages = N.forward(wn, x, all_stages=True)
        # the reference on the same weights: NaN everywhere from the layer on (a ReLU keeps it, every later window meets it)
        nan_p, nan_h = [bool(np.isnan(rp).any()) for rp, _ in stages], [bool(np.isnan(rh).any()) for _, rh in stages]
        if layer.startswith('Mconv'):          # stage 2's L1 branch: its heat maps are clean, stage 3 reads both
            assert nan_p == [False] + [True] * 5 and nan_h == [False, False] + [True] * 4
        else:
            assert nan_p == [True] * 6 and nan_h == [True] * 6
        assert np.isnan(stages[-1][0]).all() and np.isnan(stages[-1][1]).all()
        assert np.array_equal(np.isnan(paf), np.isnan(stages[-1][0])) and np.array_equal(np.isnan(heat), np.isnan(stages[-1][1])), \
            (int(np.isnan(paf).sum()), paf.size, int(np.isnan(heat).sum()), heat.size)
        assert np.isnan(p).tolist() == nan_p and np.isnan(h).tolist() == nan_h, (p.tolist(), h.tolist())
        assert np.isnan(total)
        eng.set_layer(layer, *w[layer])
        eng.forward_u8(imgs)
        paf1, heat1 = eng.get_maps()
        assert np.array_equal(paf1, paf0) and np.array_equal(heat1, heat0)
    finally:
        eng.close()


@pytest.mark.parametrize('conv1_wino', [2, 0])
def test_network_nan_pixel_through_the_fused_conv1_launch(native, conv1_wino):
    """One NaN pixel at the corner of image 0 of a float batch of two (forward_f32), conv1_1 + conv1_2 as the fused launch in its Winograd
    (conv1_wino = 2, 64 x 96) and its direct form (0, 184 x 184): the
    conv1_1 values the kernel computes OUTSIDE the image next to that corner are NaN too and are masked to conv1_2's zero padding (every
    conv1_2 output that reads such a ring position also reads a NaN inside the image, so the ring itself is pinned by the bit-exact
    tests of tests/test_gpu_conv.py on finite data and its NaN case is checked by reading the kernel only; here: no NaN leaves the
    image).  The maps are NaN exactly where network_ref's are -- all of image 0: the receptive field of the last stage covers either input
    from any pixel --, and image 1 is bit-equal to the clean run."""
    w, eng, imgs, x = _net(native, 2, (64, 96) if conv1_wino else DIRECT_FUSED[1:])
    try:
        eng.set_option('conv1_wino', conv1_wino)
        eng.forward_f32(x)
        paf0, heat0 = eng.get_maps()
        xn = x.copy()
        xn[0, 0, 0, 0] = np.nan
        eng.profile_reset(); eng.profile_enable(True)
        eng.forward_f32(xn)
        kernels = {e['kernel'] for e in eng.profile()}
        eng.profile_enable(False)
        paf, heat = eng.get_maps()
        assert any(kn.startswith('conv_wino1_') if conv1_wino else 'conv1_fused' in kn for kn in kernels), kernels
        assert not any('conv1_fused' in kn if conv1_wino else kn.startswith('conv_wino1_') for kn in kernels), kernels
        rpaf, rheat = N.forward(w, xn)
        assert np.isnan(rpaf[0]).all() and not np.isnan(rpaf[1]).any()
        assert np.array_equal(np.isnan(paf), np.isnan(rpaf)) and np.array_equal(np.isnan(heat), np.isnan(rheat))
        assert np.array_equal(paf[1], paf0[1]) and np.array_equal(heat[1], heat0[1])
    finally:
        eng.close()
