#!/usr/bin/env python3
"""Time the result images (draw_person_pose + addWeighted + face / hand parts) of 32 frames of 640 x 480:

  host      the loop `demo.render(img, poses, parts)` per frame: the NumPy functions, which are the device form's contract
  device    ONE `demo.render_batch` call from host images (image uploads, staging copy, one launch, one D2H copy, one synchronisation)
  resident  the same call on device-resident images with device-resident output (torch tensors), closed by a synchronisation
  kernel    the launch alone, from the context's per-launch profiler (an event pair around it) in a pass of its own

Legs: 1, 5 and 20 people per frame, joints uniform over the frame (long limbs: a pessimistic case for limb length), and `parts`: one
person per frame with a face and both hands (integer key points, as the detectors return them).  Seeded inputs; before anything is timed
the device canvases are compared with the host's, byte for byte.  Host clock around synchronised work, a warm-up of every shape first,
host and device legs alternate; median, min, max and spread are written as JSON.  `bytes_moved` is what the kernel has to move (every
pixel read once and written once), `kernel_share_of_hbm_peak` that over the kernel time and the HBM peak rate.

    python tools/render_time.py [--repeats 20] [--host-repeats 3] [--out profiles/render.json]
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

FRAMES, H, W = 32, 480, 640
HBM_PEAK_BYTES_PER_S = 8e12          # MI355X HBM3E (datasheet)


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts.min()), max_ms=float(ts.max()),
                spread_pct=float((ts.max() - ts.min()) / np.median(ts) * 100), repeats=len(ts))


def people(rng, n):
    p = np.zeros((n, 18, 3))
    p[:, :, 0] = rng.uniform(0, W, (n, 18))
    p[:, :, 1] = rng.uniform(0, H, (n, 18))
    p[:, :, 2] = 2
    return p


def person_parts(rng):
    def part(n, size):
        left, top = int(rng.integers(0, W - size)), int(rng.integers(0, H - size))
        kps = [[int(rng.integers(0, size)), int(rng.integers(0, size)), np.float32(rng.random())] for _ in range(n)]
        return {'bbox': (left, top, left + size, top + size), 'keypoints': kps}
    return {'unit_length': 40.0, 'face': part(70, 120), 'left': part(21, 90), 'right': part(21, 90)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--host-repeats', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'render.json'))
    args = ap.parse_args()
    import torch
    torch.cuda.init()                      # torch's HIP runtime before the library's (it cannot initialise after it)
    native, PD, demo = ge._pkg('native'), ge._pkg('pose_detector'), ge._pkg('demo')
    if native.needs_build():
        native.build()
    det = PD.PoseDetector(device=0)        # no weights: drawing needs none
    eng = det.engine
    rng = np.random.default_rng(2024)
    imgs = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(FRAMES)]
    dev = [torch.from_numpy(im).cuda() for im in imgs]
    torch.cuda.synchronize()
    legs = {'people_1': ([people(rng, 1) for _ in imgs], [[] for _ in imgs]),
            'people_5': ([people(rng, 5) for _ in imgs], [[] for _ in imgs]),
            'people_20': ([people(rng, 20) for _ in imgs], [[] for _ in imgs]),
            'parts': ([people(rng, 1) for _ in imgs], [[person_parts(rng)] for _ in imgs])}
    res = dict(frames=FRAMES, height=H, width=W, bytes_moved=FRAMES * H * W * 3 * 2,
               clock='host perf_counter around synchronised work, warm-up of every shape first, host and device legs alternate; '
                     'kernel_ms: event pairs of the per-launch profiler, in a pass of its own', legs={})
    for name, (poses, parts) in legs.items():
        host = lambda: [demo.render(im, p, q) for im, p, q in zip(imgs, poses, parts)]
        device = lambda: demo.render_batch(det, imgs, poses, parts)

        def resident():
            out = demo.render_batch(det, dev, poses, parts)
            eng.synchronize()
            return out
        want = host()
        for got in (device(), [o.cpu().numpy() for o in resident()]):
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), name
        th, td, tr = [], [], []
        for k in range(args.repeats):
            if k < args.host_repeats:
                t0 = time.perf_counter(); host(); th.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); device(); td.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); resident(); tr.append(time.perf_counter() - t0)
        r = dict(host_loop_of_demo_render=stats(th), device_one_call_from_host_images=stats(td),
                 resident_call_and_synchronise=stats(tr))
        eng.profile_reset(); eng.profile_enable(True)
        for _ in range(args.repeats):
            resident()
        k = [e for e in eng.profile() if e['kernel'] == 'render_tiles_kernel']
        eng.profile_enable(False); eng.profile_reset()
        assert len(k) == 1 and k[0]['launches'] == args.repeats, k
        r['kernel_ms'] = k[0]['avg_ms']
        r['ratio_host_over_device'] = r['host_loop_of_demo_render']['median_ms'] / r['device_one_call_from_host_images']['median_ms']
        r['ratio_host_over_resident'] = r['host_loop_of_demo_render']['median_ms'] / r['resident_call_and_synchronise']['median_ms']
        r['kernel_share_of_hbm_peak'] = res['bytes_moved'] / HBM_PEAK_BYTES_PER_S / (r['kernel_ms'] * 1e-3)
        res['legs'][name] = r
    eng.close()
    txt = json.dumps(res, indent=1)
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(txt + '\n')
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
