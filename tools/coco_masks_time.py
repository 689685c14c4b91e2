#!/usr/bin/env python3
"""Time the ignore masks (gen_masks of the reference's gen_ignore_mask.py) of 32 synthetic images of 640 x 480:

  host      the loop `coco.masks_numpy(h, w, parts)` per image: the NumPy functions, which are the device form's contract
  device    ONE `Engine.coco_masks` call with host output (table flattening, staging copy, one launch, two D2H copies, one synchronisation)
  resident  the same call with device-resident output (torch tensors), closed by a synchronisation
  kernel    the launch alone, from the context's per-launch profiler (an event pair around it) in a pass of its own

Legs: 2, 8 and 20 annotations per image; every annotation but the last is one polygon of 20 - 80 vertices around a random centre (classes
keep and miss in turn), the last is a crowd annotation given as run lengths (a filled ellipse).  Seeded inputs; before anything is timed
the device masks are compared with the host's, byte for byte.  Host clock around synchronised work, a warm-up of every shape first, host
and device legs alternate; median, min, max and spread are written as JSON.  `bytes_written` is what the kernel stores (two masks).

    python tools/coco_masks_time.py [--repeats 20] [--host-repeats 2] [--out profiles/coco_masks.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

IMAGES, H, W = 32, 480, 640


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts.min()), max_ms=float(ts.max()),
                spread_pct=float((ts.max() - ts.min()) / np.median(ts) * 100), repeats=len(ts))


def polygon(rng):
    k = int(rng.integers(20, 81))
    cx, cy, r = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(20, 160)
    ang = np.sort(rng.uniform(0, 2 * np.pi, k))
    rad = r * rng.uniform(0.6, 1.0, k)
    return np.round(np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1).reshape(-1), 2)


def crowd_counts(rng):
    yy, xx = np.mgrid[0:H, 0:W]
    cx, cy, a, b = rng.uniform(100, W - 100), rng.uniform(100, H - 100), rng.uniform(40, 200), rng.uniform(40, 150)
    bits = ((((xx - cx) / a) ** 2 + ((yy - cy) / b) ** 2) <= 1).T.reshape(-1)          # column-major
    edges = np.nonzero(np.diff(np.concatenate([[0], bits.astype(np.int8), [0]])))[0]
    runs = np.diff(np.concatenate([[0], edges, [bits.size]]))
    return runs[:-1] if runs[-1] == 0 and runs.size % 2 == 0 else runs


def image_parts(rng, n_ann):
    parts = [(0, a, a % 2, polygon(rng)) for a in range(n_ann - 1)]
    counts = crowd_counts(rng)
    assert counts.sum() == H * W
    return parts + [(1, n_ann - 1, 2, counts.astype(np.uint32))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--host-repeats', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'coco_masks.json'))
    args = ap.parse_args()
    import torch
    torch.cuda.init()                      # torch's HIP runtime before the library's (it cannot initialise after it)
    native, coco = ge._pkg('native'), ge._pkg('coco')
    if native.needs_build():
        native.build()
    eng = native.Engine(0, max_batch=1, max_h=64, max_w=64)          # no weights: the masks need none
    rng = np.random.default_rng(2024)
    sizes = [(H, W)] * IMAGES
    res = dict(images=IMAGES, height=H, width=W, bytes_written=IMAGES * H * W * 2,
               clock='host perf_counter around synchronised work, warm-up of every shape first, host and device legs alternate; '
                     'kernel_ms: event pairs of the per-launch profiler, in a pass of its own', legs={})
    for n_ann in (2, 8, 20):
        parts = [image_parts(rng, n_ann) for _ in range(IMAGES)]
        host = lambda: [coco.masks_numpy(H, W, p) for p in parts]
        device = lambda: eng.coco_masks(sizes, parts)

        def resident():
            out = eng.coco_masks(sizes, parts, device=True)
            eng.synchronize()
            return out
        want = host()
        got, dev = device(), resident()
        for k in range(IMAGES):
            for j in (0, 1):
                assert np.array_equal(got[j][k], want[k][j].astype(bool)) and np.array_equal(dev[j][k].cpu().numpy(), want[k][j]), (n_ann, k, j)
        th, td, tr = [], [], []
        for k in range(args.repeats):
            if k < args.host_repeats:
                t0 = time.perf_counter(); host(); th.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); device(); td.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); resident(); tr.append(time.perf_counter() - t0)
        tables = native.coco_mask_tables(sizes, parts)
        t0 = time.perf_counter()
        for _ in range(args.repeats):
            native.coco_mask_tables(sizes, parts)
        flatten_ms = (time.perf_counter() - t0) / args.repeats * 1e3
        r = dict(annotations_per_image=n_ann, parts=int(len(tables[1])), vertices=int(tables[2].size // 2), run_length_counts=int(tables[3].size),
                 host_loop_of_masks_numpy=stats(th), device_one_call_host_output=stats(td), resident_call_and_synchronise=stats(tr),
                 python_table_flattening_ms=flatten_ms)
        eng.profile_reset(); eng.profile_enable(True)
        for _ in range(args.repeats):
            resident()
        k = [e for e in eng.profile() if e['kernel'] == 'masks_kernel']
        eng.profile_enable(False); eng.profile_reset()
        assert len(k) == 1 and k[0]['launches'] == args.repeats, k
        r['kernel_ms'] = k[0]['avg_ms']
        r['ratio_host_over_device'] = r['host_loop_of_masks_numpy']['median_ms'] / r['device_one_call_host_output']['median_ms']
        r['ratio_host_over_resident'] = r['host_loop_of_masks_numpy']['median_ms'] / r['resident_call_and_synchronise']['median_ms']
        res['legs']['annotations_%d' % n_ann] = r
    eng.close()
    txt = json.dumps(res, indent=1)
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(txt + '\n')
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
