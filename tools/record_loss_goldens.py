"""Records tests/golden/loss_ref.npz: the reference's own label maps and compute_loss results for the validation-loss tests.

Run once where the reference is present (oracle/_refimport.py::REFERENCE_DIR):  python tools/record_loss_goldens.py
  labels        generate_heatmaps / generate_pafs of the reference's CocoDataLoader (imported verbatim by oracle._refimport)
  compute_loss  the reference's function, taken from train_coco_pose_estimation.py at run time with `ast` and executed over stand-ins for
                its three third-party calls: F.resize_images = oracle._refimport._resize_images, F.mean_squared_error = Chainer's float32
                `diff.ravel().dot(diff) / size`, cuda.to_cpu = identity.  The stage outputs are the net_posenet_stage* goldens of
                tests/golden/ref_checks.npz (the reference's own six stages at 64 x 96).
Only inputs and results are stored; nothing of the reference's text.
"""
import ast
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import _refimport as R          # noqa: E402
from oracle import fixtures                 # noqa: E402
from oracle.postprocess_ref import LIMBS_POINT          # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
SIGMA, WIDTH = 7, 8


class Var(object):
    """stands in for the chainer.Variable F.mean_squared_error returns"""

    def __init__(self, data):
        self.data = np.asarray(data)

    def __add__(self, other):
        return Var(self.data + (other.data if isinstance(other, Var) else other))

    __radd__ = __add__


def mean_squared_error(x0, x1):
    """chainer.functions.mean_squared_error forward on the CPU: diff = (x0 - x1).ravel(); diff.dot(diff) / diff.dtype.type(diff.size)"""
    diff = (R._arr(x0) - R._arr(x1)).ravel()
    return Var(diff.dot(diff) / diff.dtype.type(diff.size))


def reference_compute_loss():
    src = open(os.path.join(R.REFERENCE_DIR, 'train_coco_pose_estimation.py')).read()
    fn = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == 'compute_loss']
    assert len(fn) == 1
    ns = {'F': types.SimpleNamespace(resize_images=R._resize_images, mean_squared_error=mean_squared_error),
          'cuda': types.SimpleNamespace(to_cpu=lambda a: a)}
    exec(compile(ast.Module(body=fn, type_ignores=[]), 'compute_loss', 'exec'), ns)
    return ns['compute_loss']


def axis_people():
    """two people with integer coordinates whose limbs are all horizontal or vertical; person 1: a coincident joint pair, several v = 0"""
    a = {0: (40, 8), 1: (40, 20), 2: (28, 20), 3: (28, 32), 4: (20, 32), 5: (54, 20), 6: (54, 34), 7: (62, 34), 8: (40, 36), 9: (40, 48),
         10: (30, 48), 11: (40, 30), 12: (52, 30), 13: (52, 44), 14: (28, 8), 15: (54, 8), 16: (28, 6), 17: (54, 6)}
    p = np.zeros((2, 18, 3))
    for j, (x, y) in a.items():
        p[0, j] = (x, y, 2)
        p[1, j] = (x + 30, y + 10, 2)
    p[1, 4, :2] = p[1, 3, :2]                # RightHand on RightElbow: generate_constant_paf's "same joint" branch
    for j in (0, 13, 16):
        p[1, j, 2] = 0
    p[0, 7, 2] = 0
    for q in p:
        for ja, jb in LIMBS_POINT:
            assert q[ja, 0] == q[jb, 0] or q[ja, 1] == q[jb, 1]
    return p


def band_margin(shape, poses, width):
    """smallest distance of any pixel's (hor, ver) to a band edge over all limbs of all people (float64, the reference's formulas)"""
    H, W = shape
    gx, gy = np.meshgrid(np.arange(W), np.arange(H))
    m = np.inf
    for pose in poses:
        for ja, jb in LIMBS_POINT:
            a, b = pose[ja], pose[jb]
            if not (a[2] > 0 and b[2] > 0) or np.array_equal(a[:2], b[:2]):
                continue
            dist = np.linalg.norm(b[:2] - a[:2])
            unit = (b[:2] - a[:2]) / dist
            hor = unit[0] * (gx - a[0]) + unit[1] * (gy - a[1])
            ver = -unit[1] * (gx - a[0]) + unit[0] * (gy - a[1])
            m = min(m, np.abs(hor).min(), np.abs(hor - dist).min(), np.abs(np.abs(ver) - width).min())
    return m


def masks_of(h, w):
    m = {'none': None, 'left': np.zeros((h, w), bool), 'all': np.ones((h, w), bool), 'px00': np.zeros((h, w), bool),
         'pxlast': np.zeros((h, w), bool)}
    m['left'][:, :w // 2] = True
    m['px00'][0, 0] = True
    m['pxlast'][h - 1, w - 1] = True
    return m


def main():
    assert R.reference_available()
    _, _, _, gen = R.import_reference()
    compute_loss = reference_compute_loss()
    z = np.load(os.path.join(GOLDEN, 'ref_checks.npz'))
    ys_paf = [R.RefVar(z['net_posenet_stage%d_paf' % s]) for s in range(6)]
    ys_heat = [R.RefVar(z['net_posenet_stage%d_heat' % s]) for s in range(6)]
    cases = {
        'generic3': ((64, 96), fixtures.random_poses(np.random.default_rng(11), 3, 64, 96, drop_prob=0.05)),
        'axis2': ((64, 96), axis_people()),
        'empty': ((64, 96), np.zeros((0, 18, 3))),
        'odd': ((72, 56), fixtures.random_poses(np.random.default_rng(12), 2, 72, 56, drop_prob=0.05)),
    }
    out = {'cases': np.array(sorted(cases)), 'masks': np.array(sorted(masks_of(8, 8))), 'sigma_width': np.array([SIGMA, WIDTH], np.float64)}
    for name, (shape, poses) in cases.items():
        if name in ('generic3', 'odd'):
            margin = band_margin(shape, poses, WIDTH)
            assert margin > 1e-9, (name, margin)          # the PAF flags of these cases do not rest on a near-tie
            print(name, 'band margin %.3g' % margin)
        img = np.zeros(shape + (3,), np.uint8)
        heat = gen.generate_heatmaps(img, poses, SIGMA)
        paf = gen.generate_pafs(img, poses, WIDTH)
        assert heat.dtype == np.float32 and paf.dtype == np.float32 and heat.shape == (19,) + shape and paf.shape == (38,) + shape
        out['%s_hw' % name] = np.array(shape, np.int32)
        out['%s_poses' % name] = poses
        out['%s_paf' % name] = paf
        out['%s_heat' % name] = heat
        if shape != (64, 96):
            continue
        for mname, mask in masks_of(*shape).items():
            m = np.zeros((1,) + shape, bool) if mask is None else mask[None]
            total, paf_log, heat_log = compute_loss(None, ys_paf, ys_heat, paf[None], heat[None], m)
            out['%s_%s_loss' % (name, mname)] = np.array([float(total.data)] + paf_log + heat_log, np.float64)
            print(name, mname, float(total.data))
    path = os.path.join(GOLDEN, 'loss_ref.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    largest = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f != 'loss_ref.npz')
    print(path, size, 'bytes (largest other golden: %d)' % largest)
    assert size <= largest and size <= 1 << 20


if __name__ == '__main__':
    main()
