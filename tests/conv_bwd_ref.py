"""Host references of pmx_conv2d_backward and pmx_get_loss_grads (include/pose_mi355x.h), shared by the host and the GPU tests:
the order-defined twin of the weight-gradient kernel (tests/conv_wgrad_twin.c: fmaf, built here with the host compiler and
-ffp-contract=off), the mask rule (first-argmax, strict z > 0) and the bias-gradient rule in NumPy, the loss-gradient formula in NumPy, and
the float64 autograd references with the error bound of a float32 sum of products."""
import ctypes as C
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
    """The stand-alone program (its own main: twin + the host-side weight repacking of csrc/conv_bwd_pack.h) -> path of the executable."""
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


def dw_bound(g, x, w, dw64):
    """Elementwise bound of |dw - dw64| for ANY summation order of float32 products over K = B * H * W pixels:
    gamma_(K+1) * autograd_dw(|g|, |x|) + 2^-24 * |dw64|, gamma_n = n u / (1 - n u)."""
    B, _, H, W = np.asarray(g).shape
    n = B * H * W + 1
    gamma = n * U / (1.0 - n * U)
    _, dwa, _ = conv_grads64(np.abs(g), np.abs(x), w)
    return gamma * dwa + U * np.abs(dw64)
