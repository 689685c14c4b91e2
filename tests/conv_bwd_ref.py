"""Host references of pmx_conv2d_backward and pmx_get_loss_grads (include/pose_mi355x.h), shared by the host and the GPU tests:
the order-defined twin of the weight-gradient kernel (tests/conv_wgrad_twin.c: fmaf, built here with the host compiler and
-ffp-contract=off), the mask rule (first-argmax, strict z > 0) and the bias-gradient rule in NumPy, the loss-gradient formula in NumPy, and
the float64 autograd references with the error bound of a float32 sum of products; the float64 / float32 reference pairs of a data gradient
and of a forward layer with the error ratio that compares a result with torch's own float32; and the integer lattice on which every fp32
summation order gives the same bits, with the census of the ties and zeros that a lattice case holds."""
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, 'chainer_realtime_multi-person_pose_estimation_amd', 'csrc')
TWIN_SRC = os.path.join(HERE, 'conv_wgrad_twin.c')
MAIN_SRC = os.path.join(HERE, 'conv_wgrad_main.c')
U = 2.0 ** -24          # unit roundoff of float32
MARGIN = 16.0           # ratio(): the error of a kernel form over that of torch's float32 for the same operation on the same inputs (other
                        # summation orders and kernel forms than a direct fp32 sum); a path of lower precision is thousands of times off

_twin = None
_tmp = None


def _cc():
    cc = shutil.which('gcc') or shutil.which('cc')
    assert cc, 'no host C compiler'
    return cc


def twin_lib():
    """The twin as a shared library in a temporary directory (built once per process)."""
    global _twin, _tmp
    if _twin is None:
        _tmp = tempfile.TemporaryDirectory(prefix='conv_wgrad_twin')
        so = os.path.join(_tmp.name, 'conv_wgrad_twin.so')
        r = subprocess.run([_cc(), '-O2', '-ffp-contract=off', '-shared', '-fPIC', '-Wall', '-Wextra', '-Werror', TWIN_SRC, '-o', so, '-lm'],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        lib = C.CDLL(so)
        lib.conv_wgrad_twin_strips.restype = C.c_int
        lib.conv_wgrad_twin_strips.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_int)]
        lib.conv_wgrad_twin.restype = None
        lib.conv_wgrad_twin.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 8 + [C.c_void_p]
        _twin = lib
    return _twin


def build_main(out_dir, name, extra):
    """The stand-alone program (its own main: twin + the host restatement of the weight repacking, tests/conv_bwd_pack.h) -> path of the executable."""
    exe = os.path.join(str(out_dir), name)
    cmd = [_cc(), '-O1', '-g', '-ffp-contract=off', '-Wall', '-Wextra', '-Werror', '-I', CSRC] + list(extra) + [MAIN_SRC, TWIN_SRC, '-o', exe, '-lm']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def strips_for(B, H, cout, cin, ks, s0=0):
    """(strips, rows per strip) the library cuts B * H image rows into when s0 strips are asked for (0: its automatic count)."""
    rows = C.c_int(0)
    return twin_lib().conv_wgrad_twin_strips(B, H, cout, cin, ks, int(s0), C.byref(rows)), rows.value


def wgrad_twin(g, x, ks, s0=0):
    """dw (cout, cin, ks, ks) float32 in the kernel's order for g (B, cout, H, W), x (B, cin, H, W), s0 requested strips (0: automatic)."""
    g = np.ascontiguousarray(g, dtype=np.float32)
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, cout, H, W = g.shape
    cin = x.shape[1]
    assert x.shape == (B, cin, H, W)
    strips, rows = strips_for(B, H, cout, cin, ks, s0)
    dw = np.empty((cout, cin, ks, ks), np.float32)
    twin_lib().conv_wgrad_twin(g.ctypes.data, x.ctypes.data, B, H, W, cout, cin, ks, strips, rows, dw.ctypes.data)
    return dw


def mask_rule(dy, z, relu, pool):
    """g (B, cout, H, W) float32 from dy and the convolution's output z: with pool, dy goes to the FIRST position of each 2 x 2 window, in
    the order (0,0), (0,1), (1,0), (1,1), whose a = relu ? max(z, 0) : z equals the window's maximum; with relu, zero where z > 0 is false."""
    dy = np.asarray(dy, dtype=np.float32)
    z = np.asarray(z, dtype=np.float32)
    B, c, H, W = z.shape
    if pool:
        a = np.maximum(z, np.float32(0)) if relu else z
        win = a.reshape(B, c, H // 2, 2, W // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(B, c, H // 2, W // 2, 4)
        first = np.argmax(win, axis=-1)                     # (np.argmax returns the first of equal maxima)
        sel = np.zeros(win.shape, np.float32)
        np.put_along_axis(sel, first[..., None], 1.0, axis=-1)
        g = (sel * dy[..., None]).reshape(B, c, H // 2, W // 2, 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(B, c, H, W)
    else:
        g = dy.copy()
    if relu:
        g = g * (z > 0)
    return np.ascontiguousarray(g, dtype=np.float32)


def db_rule(g):
    """db (cout,) float32: the float64 sum over (n, y, x), cast."""
    return np.asarray(g, dtype=np.float64).sum(axis=(0, 2, 3)).astype(np.float32)


def flip_weights(w):
    """w'[ci][co][ky][kx] = w[co][ci][ks-1-ky][ks-1-kx]"""
    return np.ascontiguousarray(np.asarray(w).transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])


def loss_grad_formula(y, t, mask, n_batch):
    """F.mean_squared_error's backward with gy = 1 for one branch: y, t (B, C, fh, fw) float32, mask (B, fh, fw) bool (True = ignored):
    c * (y - t) with c = float32(2 / N), N = the element count; +0.0 where the mask is set."""
    y = np.asarray(y, dtype=np.float32)
    t = np.asarray(t, dtype=np.float32)
    assert y.shape == t.shape and y.shape[0] == n_batch
    c = np.float32(2.0 / float(y.size))
    g = (c * (y - t)).astype(np.float32)
    g[np.broadcast_to(np.asarray(mask, dtype=bool)[:, None], g.shape)] = np.float32(0.0)
    return g


# ---- float64 autograd references (torch CPU) -------------------------------------------------------------------------------------------
def autograd64(x, w, b, dy, relu, pool):
    """float64 autograd of conv2d [+ relu] [+ max_pool2d(2, 2)] -> dict(z, dx, dw, db) float64."""
    import torch
    import torch.nn.functional as F
    k = w.shape[-1]
    xt = torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True)
    wt = torch.tensor(np.asarray(w, dtype=np.float64), requires_grad=True)
    bt = torch.tensor(np.asarray(b, dtype=np.float64), requires_grad=True)
    z = F.conv2d(xt, wt, bt, padding=k // 2)
    y = F.relu(z) if relu else z
    if pool:
        y = F.max_pool2d(y, 2, 2)
    y.backward(torch.tensor(np.asarray(dy, dtype=np.float64)))
    return dict(z=z.detach().numpy(), dx=xt.grad.numpy(), dw=wt.grad.numpy(), db=bt.grad.numpy())


def conv_grads64(g, x, w):
    """float64 autograd of the plain convolution for a GIVEN output gradient g -> (dx, dw, db) float64."""
    import torch
    import torch.nn.functional as F
    k = w.shape[-1]
    xt = torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True)
    wt = torch.tensor(np.asarray(w, dtype=np.float64), requires_grad=True)
    bt = torch.zeros(w.shape[0], dtype=torch.float64, requires_grad=True)
    F.conv2d(xt, wt, bt, padding=k // 2).backward(torch.tensor(np.asarray(g, dtype=np.float64)))
    return xt.grad.numpy(), wt.grad.numpy(), bt.grad.numpy()


def _dx(g, w, dtype):
    import torch
    import torch.nn.functional as F
    k = w.shape[-1]
    with torch.no_grad():
        dx = F.conv_transpose2d(torch.tensor(np.asarray(g)).to(dtype), torch.tensor(np.asarray(w)).to(dtype), padding=k // 2)
    return dx.double().numpy()


def dx_pair(g, w):
    """(dx64, dx32) of the plain convolution for a GIVEN output gradient g (B, cout, H, W) and weights w (cout, cin, k, k): torch on the CPU
    in float64 (the reference) and in float32 (the yardstick: the same inputs and operation in the precision the kernels work in), both
    returned as float64."""
    import torch
    return _dx(g, w, torch.float64), _dx(g, w, torch.float32)


def fwd_pair(x, w, b, relu):
    """(a64, a32) of [relu](conv2d(x, w) + b), as dx_pair."""
    import torch
    import torch.nn.functional as F
    out = []
    for dtype in (torch.float64, torch.float32):
        with torch.no_grad():
            a = F.conv2d(torch.tensor(np.asarray(x)).to(dtype), torch.tensor(np.asarray(w)).to(dtype), torch.tensor(np.asarray(b)).to(dtype),
                         padding=w.shape[-1] // 2)
            out.append((F.relu(a) if relu else a).double().numpy())
    return tuple(out)


def ratio(lib, ref64, yard):
    """(r_l2, r_max, e_lib): the error of `lib` against the float64 reference over the error of the yardstick (torch's float32 result of the
    same operation on the same inputs), as L2 norms and as maxima over the whole array, and lib's own relative L2 error.  A yardstick without
    error or a zero reference is refused: the ratio would say nothing."""
    lib, ref64, yard = (np.asarray(a, dtype=np.float64) for a in (lib, ref64, yard))
    assert lib.shape == ref64.shape == yard.shape, (lib.shape, ref64.shape, yard.shape)
    e_lib, e_yard = lib - ref64, yard - ref64
    n_ref, n_yard, m_yard = np.sqrt((ref64 ** 2).sum()), np.sqrt((e_yard ** 2).sum()), np.abs(e_yard).max()
    assert n_ref > 0 and n_yard > 0 and m_yard > 0, (n_ref, n_yard, m_yard)
    n_lib = np.sqrt((e_lib ** 2).sum())
    return n_lib / n_yard, np.abs(e_lib).max() / m_yard, n_lib / n_ref


def dw_bound(g, x, w, dw64):
    """Elementwise bound of |dw - dw64| for ANY summation order of float32 products over K = B * H * W pixels:
    gamma_(K+1) * autograd_dw(|g|, |x|) + 2^-24 * |dw64|, gamma_n = n u / (1 - n u)."""
    B, _, H, W = np.asarray(g).shape
    n = B * H * W + 1
    gamma = n * U / (1.0 - n * U)
    _, dwa, _ = conv_grads64(np.abs(g), np.abs(x), w)
    return gamma * dwa + U * np.abs(dw64)


# ---- the integer lattice ------------------------------------------------------------------------------------------------------------------
# x, w, b in {-1, 0, 1} and dy in {-2, -1, 1, 2}, stored as float32.  Every product is an integer of magnitude <= 2, so z (|z| <= cin k k + 1),
# dx (<= 2 cout k k), dw (<= 2 B H W) and db are integers far below 2^24 and every partial sum of every order is exact: the FMA chains of the
# direct kernels, their split-K slabs, the weight-gradient MFMAs and any strip count give the same bits.  So do the F(2x2, 3x3) Winograd forms:
# the transformed weights are multiples of 1/4 (G has halves), the transformed inputs are sums of four lattice values, and multiples of 1/4
# below 2^22 add exactly.  w keeps only a share `w_density` of its entries: z = b + (a few terms of +-1) is what makes equal maxima, exact
# zeros and windows with nothing above zero frequent enough to count (lattice_census); x stays dense, so every weight gradient is a full sum.
LATTICE_FLOOR = 100          # members that every census class of a lattice case must hold

# (k, cin, cout, H, W, B) -> (seed, w_density): fixed.  Chosen on the CPU from the float64 reference alone: dense where the floors hold
# dense, else thinned until the scarcest class of the shape's windows (B * cout * H * W / 4 of them: only 1140 in the 1x1 / cin 100 case, of
# which the classes below claim most) clears the floor, at a seed at which it does.  A dense 7x7 / cin 16 layer has |z| ~ 20 and ties in 2 %
# of its 1536 windows; with 6 of its 784 taps kept, |z| <= 7 and every class has its hundred.
LATTICE_CASES = {
    (3, 3, 64, 20, 24, 2): (1, 1.0), (3, 70, 64, 14, 10, 2): (6, 0.03), (1, 4, 38, 8, 12, 2): (5, 1.0), (1, 100, 38, 10, 12, 1): (9, 0.045),
    (7, 16, 32, 8, 12, 2): (7, 0.008),
    # the shapes of the forward-option sweep; the third is a 3x3 layer that has a Winograd form, as has the layer of its data gradient
    (3, 64, 64, 16, 24, 2): (3, 0.12), (7, 32, 128, 12, 46, 2): (3, 0.25), (3, 128, 128, 8, 12, 2): (4, 0.03),
    (3, 32, 32, 46, 8, 3): (6, 0.12),                                               # the shape of the forced strips
}
LATTICE_TIE_SHAPES = list(LATTICE_CASES)[:5]
LATTICE_SWEEP_SHAPES = list(LATTICE_CASES)[5:8]
LATTICE_VARIANTS = ((1, 1), (0, 1), (1, 0))          # (relu, pool)
LATTICE_IDENTITY = (1, 32, 32, 4, 6, 1)          # w = I: dx is g itself


# the transposed layers of conv4_1 and conv4_2 at a 5 x 7 and a 6 x 10 map (partial Winograd tiles, 256 and 512 output channels of the data
# gradient's launch), for dx alone: dense weights, no relu, no pool, so no census.  |dx| <= 2 * 512 * 9.  (k, cin, cout, H, W, B) -> seed
LATTICE_WIDE = {(3, 256, 512, 6, 10, 2): 21, (3, 512, 512, 5, 7, 3): 22}


def lattice_inputs(k, cin, cout, H, W, B, pool, seed, w_density=1.0):
    """x, w, b, dy (float32) on the lattice.  dy is drawn last: x, w, b (and so z) are the same with and without pool."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-1, 2, (B, cin, H, W)).astype('f')
    w = (rng.integers(-1, 2, (cout, cin, k, k)) * (rng.random((cout, cin, k, k)) < w_density)).astype('f')
    b = rng.integers(-1, 2, cout).astype('f')
    dy = rng.choice(np.array([-2, -1, 1, 2], 'f'), (B, cout, H // 2 if pool else H, W // 2 if pool else W))
    return x, w, b, dy


def _windows(a):
    """(B, c, H, W) -> (B, c, H / 2, W / 2, 4): the 2 x 2 windows in the order (0,0), (0,1), (1,0), (1,1)"""
    B, c, H, W = a.shape
    return a.reshape(B, c, H // 2, 2, W // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(B, c, H // 2, W // 2, 4)


def lattice_census(z, dy, relu, pool):
    """What a lattice case holds of the values on which the mask rule can go wrong, counted from the float64 z of the reference (H, W even).
    With a = relu ? max(z, 0) : z --
      tied            windows whose maximum of a is attained more than once and is live (> 0 when relu)            } pooled cases
      tied_not_first  ... those whose first maximum is not at (0,0)                                                 }
      unique_1/2/3    windows with a unique maximum at (0,1) / (1,0) / (1,1)                                        }
      zeros           elements with z == 0
      dead_windows    windows with nothing above zero (relu cases)
      zero_selected   elements with z == 0 that the pool selects and whose dy is non-zero (pooled relu cases)
    Only the classes that apply to (relu, pool) are returned."""
    z = np.asarray(z, dtype=np.float64)
    out = {'zeros': int((z == 0).sum())}
    zw = _windows(z)
    aw = np.maximum(zw, 0.0) if relu else zw
    m = aw.max(axis=-1)
    first = aw.argmax(axis=-1)
    count = (aw == m[..., None]).sum(axis=-1)
    if pool:
        tied = (count > 1) & ((m > 0) if relu else True)
        out['tied'] = int(tied.sum())
        out['tied_not_first'] = int((tied & (first != 0)).sum())
        for pos in (1, 2, 3):
            out['unique_%d' % pos] = int(((count == 1) & (first == pos)).sum())
    if relu:
        out['dead_windows'] = int((zw.max(axis=-1) <= 0).sum())
    if relu and pool:
        picked = np.take_along_axis(zw, first[..., None], axis=-1)[..., 0]
        out['zero_selected'] = int(((picked == 0) & (np.asarray(dy) != 0)).sum())
    return out


@functools.lru_cache(maxsize=None)
def lattice_case(shape, relu, pool, identity=False):
    """(x, w, b, dy, ref, census) of a lattice case: the inputs at the shape's fixed seed and density (identity: w = I, seed 1), ref =
    autograd64 on the whole chain cast to float32 (exact: every value is an integer below 2^24), census from ref's float64 z.  Computed
    once per process and shared: callers do not write to it."""
    k, cin, cout, H, W, B = shape
    seed, density = (1, 1.0) if identity else LATTICE_CASES[shape]
    x, w, b, dy = lattice_inputs(k, cin, cout, H, W, B, pool, seed, density)
    if identity:
        assert k == 1 and cin == cout
        w = np.eye(cin, dtype='f').reshape(cin, cin, 1, 1)
    ref64 = autograd64(x, w, b, dy, relu, pool)
    census = lattice_census(ref64['z'], dy, relu, pool)
    ref = {}
    for name, a in ref64.items():
        ref[name] = a.astype('f')
        assert np.array_equal(ref[name].astype(np.float64), a) and np.abs(a).max() < 2.0 ** 22, name
    for a in (x, w, b, dy) + tuple(ref.values()):
        a.setflags(write=False)
    return x, w, b, dy, ref, census


@functools.lru_cache(maxsize=None)
def lattice_wide_case(shape):
    """(x, w, dy, dx) of a LATTICE_WIDE case: dense lattice inputs, dx = float64 autograd of the plain convolution cast to float32 (exact:
    integers below 2^22).  Shared: callers do not write to it."""
    k, cin, cout, H, W, B = shape
    x, w, _, dy = lattice_inputs(k, cin, cout, H, W, B, 0, LATTICE_WIDE[shape])
    dx64 = conv_grads64(dy, x, w)[0]
    dx = dx64.astype('f')
    assert np.array_equal(dx.astype(np.float64), dx64) and np.abs(dx64).max() <= 2 * cout * k * k < 2.0 ** 22
    for a in (x, w, dy, dx):
        a.setflags(write=False)
    return x, w, dy, dx
