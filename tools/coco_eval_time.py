#!/usr/bin/env python3
"""Time COCOeval's per-image step (ranking, OKS, the 3 x 10 matching walks) of 32 and of 256 synthetic images:

  host      the loop `coco.evaluate_image(coco.detections(poses, scores), annotations)` per image: the NumPy functions, which are the
            device form's contract
  device    ONE `Engine.coco_eval` call from host arrays (table flattening, staging copy, one launch, the D2H copies, one synchronisation)
  in_place  ONE `Engine.coco_eval` call on the result records of a post-process, where they lie on the device.  The records come from
            the maps of the golden image e2e_people, installed for every image of the batch (set_maps + postprocess): every record then
            holds the people the post-process finds there (`record_people` in the output), whatever the leg's annotation count
  kernel    the launch alone, from the context's per-launch profiler (an event pair around it) in a pass of its own

Legs: 2, 8 and 20 people and annotations per image; a person is 17 random points in a random box of a 640 x 480 image, its detection the
same points moved by about two pixels, 85 % of the joints found.  Seeded inputs; before anything is timed the device tables are compared
with the host's.  Host clock around synchronised work, a warm-up of every shape first, host and device legs alternate; median, min, max
and spread are written as JSON.

    python tools/coco_eval_time.py [--repeats 20] [--host-repeats 2] [--out profiles/coco_eval.json]
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

H, W = 480, 640
KEYS = ('order', 'scores', 'areas', 'dt_match', 'dt_ig', 'gt_ig')


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts.min()), max_ms=float(ts.max()),
                spread_pct=float((ts.max() - ts.min()) / np.median(ts) * 100), repeats=len(ts))


def image(rng, n, joints):
    anns, poses = [], np.zeros((n, 18, 3))
    for k in range(n):
        w, h = rng.uniform(30, 200), rng.uniform(50, 300)
        x0, y0 = rng.uniform(0, W - w), rng.uniform(0, H - h)
        pts = np.round(np.stack([x0 + rng.uniform(0, w, 17), y0 + rng.uniform(0, h, 17)], axis=1))
        vis = rng.integers(0, 3, 17)
        vis[0] = 2
        rows = np.concatenate([pts * (vis[:, None] > 0), vis[:, None]], axis=1)
        anns.append({'keypoints': [float(v) for v in rows.reshape(-1)], 'area': float(w * h * 0.6), 'bbox': [float(x0), float(y0), float(w), float(h)],
                     'iscrowd': int(k == n - 1 and n > 2), 'num_keypoints': int((vis > 0).sum())})
        found = rng.random(17) < 0.85
        for i, j in enumerate(joints):
            if found[i]:
                poses[k, j] = (pts[i, 0] + rng.normal(0, 2), pts[i, 1] + rng.normal(0, 2), 2)
    return poses, rng.uniform(0.5, 30, n), anns


def same(a, b):
    return (a is None and b is None) or all(np.array_equal(a[k], b[k]) for k in KEYS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--host-repeats', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'coco_eval.json'))
    args = ap.parse_args()
    import torch
    torch.cuda.init()                      # torch's HIP runtime before the library's (it cannot initialise after it)
    native, coco, weights = ge._pkg('native'), ge._pkg('coco'), ge._pkg('weights')
    if native.needs_build():
        native.build()
    joints = [int(j) for j in ge._pkg('entity').params['coco_joint_indices']]
    # the maps the in-place leg's records come from: one forward of the golden image with the head it was recorded with
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'e2e_people.npz'))
    wts = weights.synthetic_weights(int(z['seed']))
    wts['Mconv7_stage6_L1'], wts['Mconv7_stage6_L2'] = (z['head_W1'], z['head_b1']), (z['head_W2'], z['head_b2'])
    net = native.Engine(0, max_batch=1, max_h=368, max_w=368)
    net.set_weights(wts)
    net.forward_u8(z['resized'][None])
    paf, heat = net.get_maps()
    net.close()
    rng = np.random.default_rng(2025)
    res = dict(height=H, width=W,
               clock='host perf_counter around synchronised work, warm-up of every shape first, host and device legs alternate; '
                     'kernel_ms: event pairs of the per-launch profiler, in a pass of its own', legs={})
    for n_images in (32, 256):
        eng = native.Engine(0, max_batch=n_images, max_h=8, max_w=8)          # no weights: set_maps installs the maps
        eng.set_maps(np.repeat(paf, n_images, axis=0), np.repeat(heat, n_images, axis=0))
        eng.postprocess(184, 184, img_len=184)
        rec = eng.results()
        record_people = [int(v) for v in sorted(set(rec['n_people']))]
        for n in (2, 8, 20):
            images = [image(rng, n, joints) for _ in range(n_images)]
            gts = [coco.ground_truths(im[2]) for im in images]
            host = lambda: [coco.evaluate_image(coco.detections(im[0], im[1]), g) for im, g in zip(images, gts)]
            device = lambda: eng.coco_eval(gts, [im[0] for im in images], [im[1] for im in images])
            in_place = lambda: eng.coco_eval(gts)
            want, got = host(), device()
            assert all(same(a, b) for a, b in zip(got, want)), (n_images, n)
            people = [(r['poses'][:r['n_people']], r['scores'][:r['n_people']]) for r in rec]
            assert all(same(a, coco.evaluate_image(coco.detections(*p), g)) for a, p, g in zip(in_place(), people, gts)), (n_images, n)
            th, td, ti = [], [], []
            for k in range(args.repeats):
                if k < args.host_repeats:
                    t0 = time.perf_counter(); host(); th.append(time.perf_counter() - t0)
                t0 = time.perf_counter(); device(); td.append(time.perf_counter() - t0)
                t0 = time.perf_counter(); in_place(); ti.append(time.perf_counter() - t0)
            r = dict(images=n_images, people_and_annotations_per_image=n, record_people=record_people, host_loop_of_evaluate_image=stats(th),
                     device_one_call_from_host_arrays=stats(td), device_one_call_on_records_in_place=stats(ti))
            eng.profile_reset(); eng.profile_enable(True)
            for _ in range(args.repeats):
                device()
            k = [e for e in eng.profile() if e['kernel'] == 'eval_kernel']
            eng.profile_enable(False); eng.profile_reset()
            assert len(k) == 1 and k[0]['launches'] == args.repeats, k
            r['kernel_ms'] = k[0]['avg_ms']
            r['ratio_host_over_device'] = r['host_loop_of_evaluate_image']['median_ms'] / r['device_one_call_from_host_arrays']['median_ms']
            res['legs']['images_%d_people_%d' % (n_images, n)] = r
        eng.close()
    txt = json.dumps(res, indent=1)
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(txt + '\n')
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
