#!/usr/bin/env python
"""One hooked forward (loss + loss gradients) with retention off, the same with retention on (pmx_backward_enable) and pmx_backward_head, at
368 x 368, batch 10 (the reference's --batchsize) and 32, in one process -> profiles/head_backward.json.  Each figure is the mean of
`iters` enqueues between two events on the context's stream, after `warmup` untimed ones; the images are on the device.
--grad-precision 2 times the head backward with f16 dw / dx of its 3x3 / 7x7 layers (engine option "grad_precision"), `both` the fp32 chain,
the f16 chain and the fp32 chain again in the same process (backward_head_ms, backward_head_f16_ms, backward_head_again_ms: the last is the
session's drift).  --census adds the range census of every head layer's g (Engine.g_census) at loss_scale_log2 0 and at --loss-scale-log2,
of the f16 chain's g where an f16 mode was asked for (2, both), else of the fp32 chain's (census_grad_precision in the output).

    python tools/head_backward_time.py [--iters N] [--warmup N] [--batches 10,32] [--grad-precision 0|2|both] [--loss-scale-log2 K]
                                       [--census] [--out PATH]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--batches', default='10,32')
    ap.add_argument('--size', type=int, default=368)
    ap.add_argument('--grad-precision', choices=['0', '2', 'both'], default='0')
    ap.add_argument('--loss-scale-log2', type=int, default=10, help='the loss scale of the f16 runs and of the second census')
    ap.add_argument('--census', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'head_backward.json'))
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
        plain = timed(eng, forward, args.iters, args.warmup)
        eng.backward_enable(True)
        kept = timed(eng, forward, args.iters, args.warmup)
        modes = {'0': [0], '2': [2], 'both': [0, 2, 0]}[args.grad_precision]
        backs = []
        for gp in modes:
            eng.set_option('grad_precision', gp)
            eng.set_option('loss_scale_log2', args.loss_scale_log2 if gp else 0)
            forward()                                              # (the loss gradients at this mode's scale)
            backs.append(timed(eng, eng.backward_head, args.iters, args.warmup))
        back = backs[0]
        census = {}
        census_gp = 0 if args.grad_precision == '0' else 2      # (the g of a layer comes from the dx of its consumers: the chain matters)
        for k in ([0, args.loss_scale_log2] if args.census else []):
            eng.set_option('grad_precision', census_gp)
            eng.set_option('loss_scale_log2', k)
            forward()
            eng.backward_head()
            census['k%d' % k] = {nm: eng.g_census(nm) for nm in eng.head_layers()}
        eng.set_option('grad_precision', 0)
        eng.set_option('loss_scale_log2', 0)
        eng.backward_enable(False)
        plain2 = timed(eng, forward, args.iters, args.warmup)          # retention off again: the session's drift
        e = dict(batch=B, h=H, w=W, iters=args.iters, warmup=args.warmup, forward_hooked_ms=plain, forward_retaining_ms=kept,
                 backward_head_ms=back, forward_hooked_again_ms=plain2, backward_over_forward=back / plain,
                 retention_cost_ms=kept - plain, retention_cost_percent=100.0 * (kept - plain) / plain)
        if args.grad_precision == '2':
            e.update(grad_precision=2, loss_scale_log2=args.loss_scale_log2)
        if args.grad_precision == 'both':
            e.update(backward_head_f16_ms=backs[1], backward_head_again_ms=backs[2], f16_over_fp32=backs[1] / backs[0],
                     loss_scale_log2=args.loss_scale_log2)
        if census:
            e.update(census=census, census_grad_precision=census_gp)
        out.append(e)
        print(json.dumps({k: v for k, v in e.items() if k != 'census'}), flush=True)
        eng.close()
        del dev
    with open(args.out, 'w') as f:
        json.dump(dict(device='MI355X', note='hooked forward = loss and loss-gradient launches included; retaining = the same with '
                       'pmx_backward_enable on (stage pairs unfused, one copy of 64 channels per stage); backward_head = the 82 layers after '
                       'conv4_2 (data, weight and bias gradients)', entries=out), f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
