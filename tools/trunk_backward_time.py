#!/usr/bin/env python
"""What retaining the trunk costs and what its backward costs, at 368 x 368, batch 10 (the reference's --batchsize) and 32, in one process
-> profiles/trunk_backward.json (EXPERIMENTS.md E39):
  the hooked forward with pmx_backward_enable 1, 2 and 1 again (mode 2 un-fuses conv1 and the three pools);
  pmx_backward_head and pmx_backward_trunk for the same retained forward;
  per trunk layer dx, dw + combine and mask + db from the per-launch profiler, dw of conv1_2 / conv2_1 / conv2_2 also with "wgrad_strips"
  forced to 32 (pmx_conv2d_backward's cap: what the trunk's own cap bought);
  conv1_1's weight-gradient kernel next to a device-to-device copy of the bytes it must read (g and x).
Each figure is the mean of `iters` enqueues between two events on the context's stream, after `warmup` untimed ones; images on the device.

    python tools/trunk_backward_time.py [--iters N] [--warmup N] [--batches 10,32] [--out PATH]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = 'chainer_realtime_multi-person_pose_estimation_amd'


def timed(eng, fn, iters, warmup):
    for _ in range(warmup):
        fn()
    eng.synchronize()
    eng.timer_start()
    for _ in range(iters):
        fn()
    return eng.timer_stop() / iters


def layer_profile(eng, iters, warmup):
    """{label: mean ms per launch group} of pmx_backward_trunk from the per-launch profiler"""
    for _ in range(warmup):
        eng.backward_trunk()
    eng.synchronize()
    eng.profile_enable(True)
    eng.profile_reset()
    for _ in range(iters):
        eng.backward_trunk()
    eng.synchronize()
    prof = {}
    for p in eng.profile():
        if p['layer'].startswith('bwd_'):
            prof[p['layer']] = prof.get(p['layer'], 0.0) + p['total_ms'] / iters
    eng.profile_enable(False)
    return prof


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--batches', default='10,32')
    ap.add_argument('--size', type=int, default=368)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'trunk_backward.json'))
    args = ap.parse_args()
    import torch
    native = importlib.import_module(PKG + '.native')
    weights = importlib.import_module(PKG + '.weights').synthetic_weights(0)
    H = W = args.size
    out = []
    for B in [int(v) for v in args.batches.split(',')]:
        rng = np.random.default_rng(B)
        imgs = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
        poses = []
        for _ in range(B):
            p = np.zeros((2, 18, 3))
            p[:, :, 0] = rng.uniform(2, W - 2, (2, 18))
            p[:, :, 1] = rng.uniform(2, H - 2, (2, 18))
            p[:, :, 2] = rng.integers(0, 3, (2, 18))
            poses.append(p)
        masks = np.zeros((B, H, W), bool)
        masks[0, 40:200, 60:300] = True
        eng = native.Engine(0, max_batch=B, max_h=H, max_w=W)
        eng.set_weights(weights)
        dev = torch.from_numpy(imgs).cuda()
        torch.cuda.synchronize()

        def forward():
            eng.forward_u8(device_ptr=dev.data_ptr(), shape=(B, H, W))
        eng.loss_set_poses(poses, H, W, masks, 7, 8)
        eng.loss_enable(True)
        eng.loss_grad_enable(True)
        eng.backward_enable(1)
        mode1 = timed(eng, forward, args.iters, args.warmup)
        eng.backward_enable(False)
        eng.backward_enable(2)
        mode2 = timed(eng, forward, args.iters, args.warmup)
        head = timed(eng, eng.backward_head, args.iters, args.warmup)
        trunk = timed(eng, eng.backward_trunk, args.iters, args.warmup)
        layers = layer_profile(eng, args.iters, args.warmup)
        eng.set_option('wgrad_strips', 32)
        capped = layer_profile(eng, args.iters, args.warmup)
        eng.set_option('wgrad_strips', 0)
        eng.backward_enable(False)
        eng.backward_enable(1)
        mode1_again = timed(eng, forward, args.iters, args.warmup)          # the session's drift
        eng.backward_enable(False)
        # the bytes conv1_1's kernel must read, copied device to device
        nbytes = B * H * W * (64 + 16) * 4
        src = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
        dst = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
        src.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.warmup):
            dst.copy_(src)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.iters):
            dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        copy_ms = e0.elapsed_time(e1) / args.iters
        conv1_dw = layers.get('bwd_dw:conv1_1', float('nan'))
        e = dict(batch=B, h=H, w=W, iters=args.iters, warmup=args.warmup, forward_mode1_ms=mode1, forward_mode2_ms=mode2,
                 forward_mode1_again_ms=mode1_again, retention_cost_ms=mode2 - mode1, retention_cost_percent=100.0 * (mode2 - mode1) / mode1,
                 backward_head_ms=head, backward_trunk_ms=trunk, trunk_over_head=trunk / head, layers_ms=layers,
                 dw_with_32_strips_ms={k: capped[k] for k in ('bwd_dw:conv1_2', 'bwd_dw:conv2_1', 'bwd_dw:conv2_2') if k in capped},
                 conv1_wgrad_ms=conv1_dw, conv1_copy_bytes=nbytes, conv1_copy_ms=copy_ms, conv1_wgrad_over_copy=conv1_dw / copy_ms)
        out.append(e)
        print(json.dumps(e), flush=True)
        eng.close()
        del dev, src, dst
    with open(args.out, 'w') as f:
        json.dump(dict(device='MI355X', note='hooked forward = loss and loss-gradient launches included; mode 1 retains the head, mode 2 the trunk as '
                       'well (conv1 unfused, three un-pooled launches + the pool kernel); layers_ms: per-launch profiler groups of '
                       'pmx_backward_trunk (bwd_g = mask or pool scatter + db, bwd_dw = weight gradient + combine, bwd_dx = data gradient); '
                       'the copy is a device-to-device copy of the g and x bytes of conv1_1', entries=out), f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
