"""CPU: the host side of the full-network training step (include/pose_mi355x.h: pmx_train_step) -- where the floats of conv1_1's
fused-kernel pack come from (csrc/pack_index.h through a stand-alone program, host compiler, -fsanitize=address,undefined) against a NumPy
restatement of the layout; tests/train_full_ref.py in float32 against float64 and against the frozen-trunk run; train_loop's schedule on a
stub detector; the C ABI surface."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import conv_bwd_ref as R
import loss_ref as L
import test_gpu_head_backward as HB
import train_full_ref as TF
import train_ref as TR
from conftest import pkg

HEAD_SCALES = {'conv4_3_CPM': 0.25, 'conv4_4_CPM': 0.25}
FULL_SCALES = dict(HEAD_SCALES, **dict.fromkeys(TR.TRUNK, 0.25))


def test_conv1_pack_index_against_numpy(tmp_path):
    """All 1792 positions.  The restatement: the direct pack of conv1_1 is [tap 9][1 chunk][64][16] with input channel c of tap t at
    k = 3 t + c of conv1_wino_kernel's 27-long dot product; the fused pack is that matrix as [half][k-pair 14][k of the pair][channel 32],
    k = 27 a zero."""
    cc = shutil.which('gcc') or shutil.which('cc')
    assert cc, 'no host C compiler'
    exe = str(tmp_path / 'conv1_pack_main')
    r = subprocess.run([cc, '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', R.CSRC,
                        os.path.join(R.HERE, 'conv1_pack_main.c'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, '64'], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    rows = np.array([[int(float(v)) for v in ln.split()] for ln in r.stdout.splitlines()])
    assert rows.shape == (1792, 3) and np.array_equal(rows[:, 0], np.arange(1792)) and np.array_equal(rows[:, 1], rows[:, 2])
    direct = np.arange(9 * 64 * 16).reshape(9, 64, 16)                       # [tap][n][packed channel]: every float its own index
    k_major = direct[:, :, :3].transpose(0, 2, 1).reshape(27, 64)             # [k = 3 tap + c][n]
    k_major = np.concatenate([k_major, np.full((1, 64), -1)])                 # the 28th k
    want = k_major.reshape(14, 2, 2, 32).transpose(2, 0, 1, 3).reshape(-1)    # [k-pair][k][half][32] -> [half][k-pair][k][32]
    assert np.array_equal(rows[:, 1], want)
    assert (rows[:, 1] < 0).sum() == 64 and len(set(rows[rows[:, 1] >= 0, 1])) == 27 * 64


def _fixture():
    cfg = HB.PRIMARY
    imgs, poses, masks = HB._data(**cfg)
    ts = [L.targets(*L.labels((cfg['H'], cfg['W']), poses[i]), masks[i]) for i in range(cfg['B'])]
    return imgs, tuple(np.stack([t[k] for t in ts]) for k in range(3))


def test_full_reference_float32_against_float64_and_the_frozen_trunk():
    """Five steps of tests/train_full_ref.py on the primary fixture: the float32 run follows the float64 one (the yardstick of the GPU test:
    16 x their largest deviation), the loss falls by >= 1 % per step, step 1 starts from the frozen-trunk run's loss exactly, and at step 5
    the frozen-trunk trajectory is at least 10 tolerances away -- a library that left the trunk alone could not pass the GPU test.
    Recorded: full 1.89924, 0.54946, 0.45180, 0.42494, 0.41017; frozen 1.89924, 0.79100, 0.54842, 0.46462, 0.42268; tolerance 1.6e-5,
    gap at step 5 1.25e-2 (ratio 800)."""
    imgs, targets = _fixture()
    W = pkg('weights').synthetic_weights(0)
    f64, P64 = TF.trajectory(W, imgs, targets, 5, 'float64', FULL_SCALES)
    f32, P32 = TF.trajectory(W, imgs, targets, 5, 'float32', FULL_SCALES)
    h64, _ = TR.trajectory(W, imgs, targets, 5, 'float64', HEAD_SCALES)
    tol = 16 * np.abs(f32 - f64).max()
    print('full float64', f64, 'full float32', f32, 'frozen float64', h64, 'tolerance', tol, 'gap at step 5', abs(h64[4] - f64[4]))
    assert len(P64) == 92 and all(P32[nm][0].dtype == np.float32 and P64[nm][0].dtype == np.float64 for nm in P64)
    assert f64[0] == h64[0]
    assert np.abs(f32 - f64).max() <= 1e-5 * f64[0]          # float32 autograd of a loss of order 1: a few 1e-6 at most
    assert (f64[1:] <= 0.99 * f64[:-1]).all()
    assert abs(h64[4] - f64[4]) >= 10 * tol
    for nm in TR.TRUNK:                                      # the trunk moved, by about alpha per step
        d = np.abs(P64[nm][0] - W[nm][0]).max()
        assert 1e-5 < d < 1e-3, (nm, d)


class StubDetector(object):
    def __init__(self):
        self.calls = []

    def set_trainable(self, trunk=False):
        self.calls.append(('trainable', trunk))

    def set_optimizer(self, alpha=1e-4, **kw):
        assert not kw
        self.calls.append(('alpha', alpha))

    def train_step(self, imgs, poses, masks):
        self.calls.append(('step', imgs))
        return {'main/loss': float(imgs)}


@pytest.mark.parametrize('start,iterations,unfreeze,steps', [(0, 6, 2, ((3, 1e-5), (5, 1e-6))), (3, 7, 2, ((3, 1e-5), (5, 1e-6))),
                                                             (0, 3, 2000, ((100000, 1e-5), (200000, 1e-6))), (4, 6, 4, ((5, 1e-6), (1, 1e-5)))])
def test_train_loop_schedule(start, iterations, unfreeze, steps):
    T = pkg('train')
    det = StubDetector()
    logged = []
    out = T.train_loop(det, ((i, None, None) for i in range(100)), iterations, start=start, unfreeze_at=unfreeze, alpha_steps=steps,
                       on_log=lambda i, r: logged.append((i, r['main/loss'])))
    n = iterations - start
    assert [r['main/loss'] for r in out] == [float(k) for k in range(n)] and logged == [(start + k, float(k)) for k in range(n)]
    want, alpha = [], None
    for k, i in enumerate(range(start, iterations)):
        want.append(('trainable', i >= unfreeze))
        a = 1e-4
        for at, v in sorted(steps):
            a = v if i >= at else a
        if a != alpha:
            want.append(('alpha', a))
            alpha = a
        want.append(('step', k))
    assert det.calls == want
    assert det.calls[0] == ('trainable', start >= unfreeze)          # also a run resumed past the threshold un-freezes at once
    assert T.alpha_at(99999) == 1e-4 and T.alpha_at(100000) == 1e-5 and T.alpha_at(199999) == 1e-5 and T.alpha_at(200000) == 1e-6


def test_train_loop_ends_with_the_batches():
    det = StubDetector()
    assert len(pkg('train').train_loop(det, [(0, None, None), (1, None, None)], 10)) == 2


def test_c_abi_surface(native):
    syms = native.header_symbols()
    lib = native.load()
    assert 'pmx_train_step' in syms and hasattr(lib, 'pmx_train_step') and len(lib._pmx_sig['pmx_train_step'][1]) == 1
    assert callable(native.Engine.train_step)
    PD = pkg('pose_detector').PoseDetector
    assert callable(PD.set_trainable)
    assert PD.REFERENCE_GRAD_SCALES == HEAD_SCALES and PD.REFERENCE_TRUNK_GRAD_SCALES == dict.fromkeys(TR.TRUNK, 0.25)
    assert 'does not exist yet' not in open(native.HEADER).read()
