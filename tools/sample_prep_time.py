"""Times the sample preparation: 32 training samples from 640 x 480 sources at insize 368 (recorded in profiles/sample_prep.json).

  device   Engine.samples_prepare from host arrays to the prepared device buffers, ONE synchronisation at the end of each call
           (upload of the sources included); warm-up calls first, then the median and the spread of `--repeats` calls
  numpy    the NumPy restatement tests/sample_ref.py of the same records, once.  This is a SLOW PYTHON RESTATEMENT, not OpenCV: nothing
           here can time the reference's real cv2 path, so the ratio says nothing about the reference's data-loader workers.

python tools/sample_prep_time.py [--n 32] [--repeats 20] [--warmup 3] [--no-numpy] [--out profiles/sample_prep.json]"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
from conftest import pkg          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=32)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--insize', type=int, default=368)
    ap.add_argument('--no-numpy', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sample_prep.json'))
    a = ap.parse_args()
    native, S = pkg('native'), pkg('samples')
    rng = np.random.default_rng(1)
    imgs = [rng.integers(0, 256, (480, 640, 3), dtype=np.uint8) for _ in range(a.n)]
    masks = [np.zeros((480, 640), bool) for _ in range(a.n)]
    poses = []
    for m in masks:
        m[100:160, 200:300] = True
        p = np.zeros((2, 18, 3), np.int32)
        p[:, :, 0], p[:, :, 1], p[:, :, 2] = rng.integers(150, 500, (2, 18)), rng.integers(80, 420, (2, 18)), 2
        poses.append(p)
    random.seed(0)
    np.random.seed(0)
    recs = [S.draw_augmentation((480, 640), p, a.insize) for p in poses]
    eng = native.Engine(0, max_batch=a.n, max_h=a.insize, max_w=a.insize)
    times = []
    for i in range(a.warmup + a.repeats):
        t0 = time.perf_counter()
        eng.samples_prepare(imgs, masks, recs, a.insize)
        eng.synchronize()
        if i >= a.warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    got_i, got_m = eng.samples_get()
    eng.close()
    res = dict(samples=a.n, source='640x480', insize=a.insize, repeats=a.repeats, warmup=a.warmup,
               device_ms_median=float(np.median(times)), device_ms_min=float(np.min(times)), device_ms_max=float(np.max(times)),
               device_samples_per_s=float(a.n / (np.median(times) * 1e-3)),
               device_note='host arrays -> prepared device buffers, the ctypes marshalling and the upload of the sources included, one synchronisation')
    if not a.no_numpy:
        import sample_ref
        t0 = time.perf_counter()
        want = [sample_ref.prepare(im, m, r, a.insize) for im, m, r in zip(imgs, masks, recs)]
        res['numpy_restatement_ms'] = (time.perf_counter() - t0) * 1e3
        res['numpy_note'] = 'tests/sample_ref.py, a slow Python restatement (whole rotated image, then crop); NOT OpenCV'
        res['bit_exact'] = bool(all(np.array_equal(got_i[k], w[0]) and np.array_equal(got_m[k], w[2]) for k, w in enumerate(want)))
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    out['timing'] = res
    json.dump(out, open(a.out, 'w'), indent=1, sort_keys=True)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
