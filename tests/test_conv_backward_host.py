"""CPU: the host side of pmx_conv2d_backward / pmx_get_loss_grads (include/pose_mi355x.h).  The order-defined twin of the weight-gradient
kernel (tests/conv_wgrad_twin.c) and the NumPy mask / bias-gradient rules (tests/conv_bwd_ref.py) against torch-CPU float64 autograd of
conv2d [+ relu] [+ max_pool2d(2, 2)]; the C ABI surface; the stand-alone program (twin + the host-side weight repacking), plain and with
-fsanitize=address,undefined.  The integer lattice of the exact GPU tests (tests/test_gpu_conv_backward_exact.py): its census floors, torch's
tie and zero behaviour against the stated mask rule, and the order twins of every kernel form on it.  The float64 / float32 reference pair of
a data gradient and the error ratio the GPU tests measure with (conv_bwd_ref.dx_pair, ratio): what the ratio catches that the elementwise
bound TOL * max(1, |ref|max) lets through at the size of a gradient."""
import subprocess

import numpy as np
import pytest

import conv_bwd_ref as R
from conftest import pkg

ENTRIES = ['pmx_conv2d_backward', 'pmx_loss_grad_enable', 'pmx_get_loss_grads']

# (k, B, cin, cout, H, W): small enough that a draw without near-ties exists within a few seeds; odd sizes, a map smaller than the kernel
SHAPES = [(3, 2, 5, 6, 6, 8), (7, 1, 3, 4, 3, 2), (1, 3, 4, 3, 4, 4), (7, 1, 2, 3, 8, 6), (3, 1, 33, 2, 5, 3)]
CASES = [(s, relu, pool) for s in SHAPES for relu, pool in ((0, 0), (1, 0), (1, 1)) if not pool or (s[4] % 2 == 0 and s[5] % 2 == 0)]
MARGIN = 1e-3


def _draw(k, B, cin, cout, H, W, relu, pool, seed0):
    """x, w, b, dy (float32) whose float64 z has no |z| < MARGIN and no pool window whose two largest a differ by less than MARGIN: the
    next seed is drawn until that holds."""
    for seed in range(seed0, seed0 + 200):
        rng = np.random.default_rng(seed)
        x = rng.standard_normal((B, cin, H, W)).astype('f')
        w = (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype('f')
        b = (1.0 + 0.3 * rng.standard_normal(cout)).astype('f')          # most z positive: few windows with nothing above zero
        dy = rng.standard_normal((B, cout, H // 2 if pool else H, W // 2 if pool else W)).astype('f')
        ref = R.autograd64(x, w, b, dy, relu, pool)
        if _margin(ref['z'], relu, pool) >= MARGIN:
            return x, w, b, dy, ref
    raise AssertionError('no draw without near-ties in 200 seeds')


def _margin(z, relu, pool):
    m = np.abs(z).min()
    if pool:
        a = np.maximum(z, 0) if relu else z
        B, c, H, W = a.shape
        win = np.sort(a.reshape(B, c, H // 2, 2, W // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(-1, 4), axis=1)
        m = min(m, (win[:, 3] - win[:, 2]).min())
    return m


@pytest.mark.parametrize('shape,relu,pool', CASES)
def test_twin_and_mask_rule_match_float64_autograd(shape, relu, pool):
    k, B, cin, cout, H, W = shape
    x, w, b, dy, ref = _draw(k, B, cin, cout, H, W, relu, pool, seed0=1000 * k + cin)
    assert _margin(ref['z'], relu, pool) >= MARGIN          # so the comparison below leaves out no element
    g = R.mask_rule(dy, ref['z'].astype('f'), relu, pool)
    dx64, dw64, db64 = R.conv_grads64(g, x, w)
    # the mask rule: the gradient that reaches the convolution is autograd's, element for element
    assert np.allclose(dw64, ref['dw'], rtol=1e-12, atol=1e-13) and np.allclose(db64, ref['db'], rtol=1e-12, atol=1e-13)
    assert np.allclose(dx64, ref['dx'], rtol=1e-12, atol=1e-13)
    bound = R.dw_bound(g, x, w, ref['dw'])
    for s0 in (0, 1, 3):
        dw = R.wgrad_twin(g, x, k, s0)
        err = np.abs(dw.astype(np.float64) - ref['dw'])
        assert (err <= bound).all(), (s0, float((err - bound).max()))
    db = R.db_rule(g)
    assert (np.abs(db.astype(np.float64) - ref['db']) <= 2.0 ** -23 * np.abs(ref['db'])).all()


def test_mask_rule_takes_the_first_of_equal_maxima_and_a_strict_relu():
    z = np.array([[[[1, 1, -2, 0], [1, 0, 0, -1]]]], 'f')          # window 0: three equal maxima; window 1: nothing above zero
    dy = np.array([[[[5, 7]]]], 'f')
    g = R.mask_rule(dy, z, relu=True, pool=True)
    assert np.array_equal(g, np.array([[[[5, 0, 0, 0], [0, 0, 0, 0]]]], 'f'))
    g = R.mask_rule(dy, z, relu=False, pool=True)
    assert np.array_equal(g, np.array([[[[5, 0, 0, 7], [0, 0, 0, 0]]]], 'f'))
    assert np.array_equal(R.mask_rule(z, z, relu=True, pool=False), z * (z > 0))
    import torch
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.max_pool2d(torch.relu(zt), 2, 2).backward(torch.tensor(dy, dtype=torch.float64))
    assert np.array_equal(zt.grad.numpy(), R.mask_rule(dy, z, relu=True, pool=True))


# ---- the integer lattice (conv_bwd_ref.py) ------------------------------------------------------------------------------------------------
LATTICE = [(s, relu, pool) for s in R.LATTICE_TIE_SHAPES for relu, pool in R.LATTICE_VARIANTS]
LATTICE_OTHER = [s for s in R.LATTICE_CASES if s not in R.LATTICE_TIE_SHAPES]          # the option sweep and the forced strips: relu and pool on


@pytest.mark.parametrize('shape,relu,pool', LATTICE + [(s, 1, 1) for s in LATTICE_OTHER])
def test_lattice_census_floors(shape, relu, pool):
    """Every class of ties and zeros that applies to the case holds at least LATTICE_FLOOR members at the case's fixed seed."""
    census = R.lattice_case(shape, relu, pool)[5]
    want = {'zeros'} | ({'tied', 'tied_not_first', 'unique_1', 'unique_2', 'unique_3'} if pool else set()) | ({'dead_windows'} if relu else set()) \
        | ({'zero_selected'} if relu and pool else set())
    assert set(census) == want
    assert min(census.values()) >= R.LATTICE_FLOOR, census


def test_census_counts_a_hand_made_map():
    #                window 0: tied at (0,0), (0,1)   window 1: unique at (1,1)   window 2: nothing above zero, z == 0 first   window 3: tied, first at (1,0)
    z = np.array([[[[2, 2, -1, 0, 0, -1, -3, -3], [1, 0, 0, 3, -2, 0, 1, 1]]]], np.float64)
    dy = np.ones((1, 1, 1, 4), 'f')
    assert R.lattice_census(z, dy, 1, 1) == dict(zeros=5, tied=2, tied_not_first=1, unique_1=0, unique_2=0, unique_3=1, dead_windows=1, zero_selected=1)
    assert R.lattice_census(z, dy, 0, 1) == dict(zeros=5, tied=3, tied_not_first=1, unique_1=0, unique_2=0, unique_3=1)
    assert R.lattice_census(z, dy, 1, 0) == dict(zeros=5, dead_windows=1)
    assert R.lattice_census(z, 0 * dy, 1, 1)['zero_selected'] == 0


@pytest.mark.parametrize('shape,relu,pool', LATTICE)
def test_lattice_autograd_is_the_mask_rule_and_the_twin(shape, relu, pool):
    """torch's CPU max-pool and ReLU backward on ties and exact zeros ARE the stated rule (first of equal maxima, strict z > 0): float64
    autograd of the whole chain equals mask_rule + the plain convolution's autograd exactly, and the order twin of the weight-gradient kernel
    equals it for every strip count -- on the lattice no order rounds."""
    x, w, b, dy, ref, _ = R.lattice_case(shape, relu, pool)
    g = R.mask_rule(dy, ref['z'], relu, pool)
    dx64, dw64, db64 = R.conv_grads64(g, x, w)
    assert np.array_equal(dx64, ref['dx']) and np.array_equal(dw64, ref['dw']) and np.array_equal(db64, ref['db'])
    assert np.array_equal(R.db_rule(g), ref['db'])
    for s0 in (0, 1, 3):
        assert np.array_equal(R.wgrad_twin(g, x, shape[0], s0), ref['dw']), s0


@pytest.mark.parametrize('relu,pool', R.LATTICE_VARIANTS)
def test_identity_weights_make_dx_the_masked_gradient(relu, pool):
    x, w, b, dy, ref, census = R.lattice_case(R.LATTICE_IDENTITY, relu, pool, identity=True)
    g = R.mask_rule(dy, ref['z'], relu, pool)
    assert np.array_equal(ref['dx'], g)
    assert ((ref['dx'] == 0) == (g == 0)).all() and (g == 0).sum() >= R.LATTICE_FLOOR          # closed gates to look at; dy has no zero
    assert min(census.values()) >= 1, census          # (192 windows: every class is there to be seen element for element, not by the hundred)


@pytest.mark.parametrize('shape', R.LATTICE_SWEEP_SHAPES)
def test_lattice_is_exact_in_the_order_of_every_forward_form(shape):
    """The premise of the option sweep on the GPU: the order twins of the direct kernels (plain and split-K) and of the Winograd kernel
    (oracle/conv_fma_ref.py) give the float64 z on the lattice, bit for bit."""
    from oracle import conv_fma_ref
    x, w, b, dy, ref, _ = R.lattice_case(shape, 1, 1)
    for splitk in (1, 2, 3):
        assert np.array_equal(conv_fma_ref.conv_fma(x, w, b, splitk=splitk), ref['z']), splitk
    assert np.array_equal(conv_fma_ref.conv_wino(x, w, b), ref['z'])
    if shape[0] == 7:
        assert np.array_equal(conv_fma_ref.conv_wino(x, w, b, unit_g=1), ref['z'])


def test_flipped_weights_give_the_data_gradient():
    import torch
    rng = np.random.default_rng(5)
    for k, cin, cout in ((3, 4, 5), (7, 2, 3), (1, 6, 2)):
        x = rng.standard_normal((2, cin, 5, 4))
        w = rng.standard_normal((cout, cin, k, k))
        g = rng.standard_normal((2, cout, 5, 4))
        dx64, _, _ = R.conv_grads64(g, x, w)
        wt = R.flip_weights(w)
        assert wt.shape == (cin, cout, k, k)
        dx = torch.nn.functional.conv2d(torch.tensor(g), torch.tensor(wt), padding=k // 2).numpy()
        assert np.allclose(dx, dx64, rtol=1e-12, atol=1e-12)


# ---- the reference pair and the error ratio ----------------------------------------------------------------------------------------------
def test_dx_pair_is_the_autograd_data_gradient():
    rng = np.random.default_rng(8)
    for k, cin, cout in ((3, 5, 6), (7, 3, 4), (1, 6, 2)):
        x = rng.standard_normal((2, cin, 5, 7)).astype('f')
        w = rng.standard_normal((cout, cin, k, k)).astype('f')
        g = rng.standard_normal((2, cout, 5, 7)).astype('f')
        dx64, dx32 = R.dx_pair(g, w)
        ref = R.conv_grads64(g, x, w)[0]
        assert dx64.dtype == dx32.dtype == np.float64 and dx64.shape == dx32.shape == x.shape
        assert np.array_equal(dx64, ref), np.abs(dx64 - ref).max()
        assert np.array_equal(dx32, dx32.astype('f').astype(np.float64)) and not np.array_equal(dx32, dx64)          # float32 values
        r_l2, r_max, e = R.ratio(dx32, dx64, dx32)
        assert (r_l2, r_max) == (1.0, 1.0) and 0 < e < 1e-6
        a64, a32 = R.fwd_pair(x, w, np.arange(cout, dtype='f'), relu=True)
        z64 = R.autograd64(x, w, np.arange(cout, dtype='f'), np.zeros((2, cout, 5, 7)), False, False)['z']
        assert np.array_equal(a64, np.maximum(z64, 0)) and R.ratio(a32, a64, a32)[:2] == (1.0, 1.0)
    with pytest.raises(AssertionError):
        R.ratio(dx64, dx64, dx64)          # a yardstick without error measures nothing
    with pytest.raises(AssertionError):
        R.ratio(dx32, 0 * dx64, dx32)


def test_ratio_catches_what_the_elementwise_bound_lets_through():
    """The data gradient of a 64 -> 64, 3x3 layer at 2 x 16 x 12 for an output gradient of the size the backward chains carry (1e-3), and
    three wrong versions of its float32 result: the weights rounded to bfloat16 (a path of lower precision), the left border column copied
    from its neighbour, one element -- the largest -- half as large again.  The ratio puts each far above the margin; the bound
    |dx - ref| <= 2e-5 * max(1, |ref|max), made for maps of size O(1), passes the first: its floor is an absolute 2e-5 and the whole
    gradient is smaller than that many times over."""
    import torch
    rng = np.random.default_rng(40)
    w = (rng.standard_normal((64, 64, 3, 3)) / np.sqrt(64 * 9)).astype('f')
    g = (1e-3 * rng.standard_normal((2, 64, 16, 12))).astype('f')
    dx64, dx32 = R.dx_pair(g, w)
    assert 1e-4 < np.abs(dx64).max() < 1e-2
    old = lambda dx: np.abs(dx - dx64).max() <= 2e-5 * max(1.0, np.abs(dx64).max())
    assert old(dx32) and R.ratio(dx32, dx64, dx32)[:2] == (1.0, 1.0)
    bf16 = R.dx_pair(g, torch.tensor(w).bfloat16().float().numpy())[1]
    column = dx32.copy()
    column[..., 0] = column[..., 1]
    element = dx32.copy()
    element.reshape(-1)[np.abs(dx64).argmax()] *= 1.5
    passes_old = {}
    for name, wrong in (('bf16', bf16), ('column', column), ('element', element)):
        r_l2, r_max, e = R.ratio(wrong, dx64, dx32)
        passes_old[name] = bool(old(wrong))
        print(name, 'r_l2 %.3g r_max %.3g rel. L2 %.3g, passes the elementwise bound: %s' % (r_l2, r_max, e, passes_old[name]))
        assert r_l2 > R.MARGIN and r_max > R.MARGIN, (name, r_l2, r_max)
    assert passes_old['bf16']


def test_wide_lattice_cases_are_exact():
    """The premise of the GPU test on them: dx is a field of integers below 2^22 (the bound of the lattice: 2 * cout * k * k), so its cast
    to float32 is exact and every fp32 summation order, Winograd's included, gives its bits."""
    for shape in R.LATTICE_WIDE:
        k, cin, cout, H, W, B = shape
        x, w, dy, dx = R.lattice_wide_case(shape)
        assert dx.shape == x.shape == (B, cin, H, W) and w.shape == (cout, cin, 3, 3) and (w != 0).mean() > 0.6
        assert np.array_equal(dx, np.rint(dx)) and 0 < np.abs(dx).max() <= 2 * 512 * 9 < 2 ** 22
        assert np.array_equal(R.dx_pair(dy, w)[1], dx)          # torch's float32 order is exact on it as well


def test_strip_rule():
    assert R.strips_for(3, 46, 32, 32, 3, 5) == (5, 28)              # 138 rows: strips end inside images (28, 56, 84, 112)
    assert R.strips_for(3, 46, 32, 32, 3, 0) == (28, 5)              # automatic: capped at 32 -> 5 rows -> 28 strips
    assert R.strips_for(1, 3, 32, 16, 7, 100) == (3, 1)
    assert R.strips_for(8, 46, 128, 128, 7, 0) == (19, 20)           # 112 units: 19 strips asked -> 20 rows each -> 19 strips
    rng = np.random.default_rng(3)
    g = rng.standard_normal((3, 2, 4, 3)).astype('f')
    x = rng.standard_normal((3, 3, 4, 3)).astype('f')
    a, b = R.wgrad_twin(g, x, 3, 1), R.wgrad_twin(g, x, 3, 5)
    assert not np.array_equal(a, b) and np.allclose(a, b, rtol=1e-4, atol=1e-5)


def test_loss_gradient_formula_is_the_backward_of_mean_squared_error():
    import torch
    rng = np.random.default_rng(11)
    y = rng.standard_normal((2, 38, 6, 8)).astype('f')
    t = rng.standard_normal((2, 38, 6, 8)).astype('f')
    mask = rng.random((2, 6, 8)) < 0.3
    g = R.loss_grad_formula(y, t, mask, 2)
    yt = torch.tensor(y, dtype=torch.float64, requires_grad=True)
    tt = torch.tensor(t, dtype=torch.float64)
    tt = torch.where(torch.tensor(mask)[:, None], yt.detach(), tt)          # :62-63
    torch.nn.functional.mse_loss(yt, tt).backward()
    ref = yt.grad.numpy()
    assert np.abs(g - ref).max() <= 4 * 2.0 ** -24 * np.abs(ref).max()
    sel = np.broadcast_to(mask[:, None], g.shape)
    assert (g[sel] == 0).all() and not np.signbit(g[sel]).any()


def test_backward_entries_declared_exported_and_bound(native):
    """The C ABI surface: the three new symbols are declared in the header, exported by the library and bound with their argument counts."""
    syms = native.header_symbols()
    lib = native.load()
    for s in ENTRIES:
        assert s in syms, s
        assert hasattr(lib, s), s
        assert s in lib._pmx_sig
    assert len(lib._pmx_sig['pmx_conv2d_backward'][1]) == 19
    for m in ('conv2d_backward', 'loss_grad_enable', 'loss_grads'):
        assert callable(getattr(native.Engine, m))
    assert callable(pkg('pose_detector').PoseDetector.loss_gradients)


def test_stand_alone_program_plain_and_sanitized_print_the_same(tmp_path):
    """A program with its own main (twin + the host-side repacking w -> w'), built plainly and with -fsanitize=address,undefined."""
    def run(exe):
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
        return r.stdout
    plain = run(R.build_main(tmp_path, 'wgrad_main', []))
    san = run(R.build_main(tmp_path, 'wgrad_main_san', ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer']))
    assert plain.count('\n') == 18 and plain.encode() == san.encode()
    lines = plain.splitlines()
    assert lines[3].startswith('case 1 strips 3 rows 4')
