#!/usr/bin/env python
"""What one training iteration costs, at 368 x 368, batch 10 (the reference's --batchsize) and 32, in one process ->
profiles/train_step.json (the head step) or, with --full, profiles/train_step_full.json (the step over all 92 layers: the engine in
backward mode 2, legs (a) and (b) with pmx_backward_trunk and pmx_train_step, the copy yardstick over the 92 layers' parameters, the packs
in existence and the packer launches a step makes; the head step's legs (a) and (b) are measured in the same process, interleaved with
the full ones, and (d) is left out).  --no-host leaves (d) out of a head run as well.  Legs, alternated `rounds` times, each figure the mean of `iters` enqueues between two events on the context's
stream after `warmup` untimed ones (images on the device):
  (a) hooked retaining forward + pmx_backward_head
  (b) the same + pmx_train_step_head
  (c) the Adam launch alone and the packers alone, from the per-launch profiler's labels train_step|adam and train_step|pack (a run of its
      own: the profiler's events slow everything else down), and a device-to-device hipMemcpyAsync that moves the same bytes as the Adam
      launch (28 per parameter: a copy of 14 bytes per parameter, read once and written once) -- the yardstick of its bandwidth
  (d) the host route the step replaces, by wall clock: every gradient fetched, Adam in NumPy, 82 x pmx_set_layer, and the next forward +
      backward, which rebuilds the derived packs (one-off launches of the device packers)

--grad-precision 2 runs every leg with f16 head gradients (engine option "grad_precision" 2, loss scale 2^K folded into every layer's
gradient scale); `both` measures legs (a) and (b) in both modes in the same process, alternated round by round (f16_* beside the fp32
figures; (c) and (d) stay fp32, but from the first f16 round on every step, the fp32 ones included, also rewrites the 58 f16 packs of the
transposed layers: packs_in_existence and pack_launches_per_step count them).

    python tools/train_step_time.py [--full] [--no-host] [--iters N] [--warmup N] [--rounds N] [--batches 10,32]
                                    [--grad-precision 0|2|both] [--loss-scale-log2 K] [--out PATH]"""
import argparse
import ctypes
import importlib
import json
import os
import sys
import time

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


def numpy_adam(w, m, v, g, scale, t, alpha=1e-4, beta1=0.9, beta2=0.999, eps=1e-8):
    f = np.float32
    a_t = f(alpha * np.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t))
    g = g * f(scale)
    m += f(1.0 - beta1) * (g - m)
    v += f(1.0 - beta2) * (g * g - v)
    return w - a_t * m / (np.sqrt(v) + f(eps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--batches', default='10,32')
    ap.add_argument('--size', type=int, default=368)
    ap.add_argument('--out', default=None)
    ap.add_argument('--full', action='store_true', help='the step over all 92 layers (backward mode 2)')
    ap.add_argument('--no-host', action='store_true', help='leave out (d), the host route')
    ap.add_argument('--grad-precision', choices=['0', '2', 'both'], default='0')
    ap.add_argument('--loss-scale-log2', type=int, default=10, help='the loss scale of the f16 legs')
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, 'profiles', 'train_step_full.json' if args.full else 'train_step.json')
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
        eng.loss_set_poses(poses, H, W, masks, 7, 8)
        eng.loss_enable(True)
        eng.loss_grad_enable(True)
        eng.backward_enable(2 if args.full else True)
        eng.train_enable(True)
        head = eng.head_layers()
        scales = {'conv4_3_CPM': 0.25, 'conv4_4_CPM': 0.25}
        if args.full:
            scales.update(dict.fromkeys(eng.TRUNK_LAYERS, 0.25))
        stepped = (list(eng.TRUNK_LAYERS) if args.full else []) + head

        def set_mode(gp):          # the gradients' precision, the loss scale and its inverse in every stepped layer's scale
            k = args.loss_scale_log2 if gp else 0
            eng.set_option('grad_precision', gp)
            eng.set_option('loss_scale_log2', k)
            for nm in stepped:
                eng.train_set_grad_scale(nm, scales.get(nm, 1.0) * 2.0 ** -k)
        set_mode(2 if args.grad_precision == '2' else 0)
        n_params = sum(int(np.prod(eng.layer_shape(nm))) + eng.layer_shape(nm)[0] for nm in stepped)

        def head_a():
            eng.forward_u8(device_ptr=dev.data_ptr(), shape=(B, H, W))
            eng.backward_head()

        def head_b():
            head_a()
            eng.train_step_head()

        def leg_a():
            head_a()
            if args.full:
                eng.backward_trunk()

        def leg_b():
            leg_a()
            eng.train_step() if args.full else eng.train_step_head()
        a_ms, b_ms, ha_ms, hb_ms, fa_ms, fb_ms = [], [], [], [], [], []
        for _ in range(args.rounds):
            a_ms.append(timed(eng, leg_a, args.iters, args.warmup))
            b_ms.append(timed(eng, leg_b, args.iters, args.warmup))
            if args.grad_precision == 'both':
                set_mode(2)
                fa_ms.append(timed(eng, leg_a, args.iters, args.warmup))
                fb_ms.append(timed(eng, leg_b, args.iters, args.warmup))
                set_mode(0)
            if args.full:          # the head step in mode 2, interleaved
                ha_ms.append(timed(eng, head_a, args.iters, args.warmup))
                hb_ms.append(timed(eng, head_b, args.iters, args.warmup))
        # (c) the two parts of the step by the profiler's labels, and the copy that moves the same bytes
        eng.profile_enable(1)
        for _ in range(args.warmup):
            leg_b()
        eng.synchronize()
        eng.profile_reset()
        for _ in range(args.iters):
            leg_b()
        eng.synchronize()
        prof = {(p['layer'], p['kernel']): p for p in eng.profile()}
        eng.profile_enable(0)
        adam_ms, pack_ms = prof[('train_step', 'adam')]['avg_ms'], prof[('train_step', 'pack')]['avg_ms']
        src = torch.empty(14 * n_params, dtype=torch.uint8, device='cuda')
        dst = torch.empty_like(src)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        copies = []
        for i in range(args.warmup + args.iters):
            e0.record()
            dst.copy_(src)          # contiguous, same type, same device: hipMemcpyAsync device to device
            e1.record()
            e1.synchronize()
            if i >= args.warmup:
                copies.append(e0.elapsed_time(e1))
        del src, dst
        copy_ms = float(np.mean(copies))
        def exists(nm, k):          # (the size query of pmx_get_pack: PMX_ERR_CAPACITY where the pack exists, PMX_ERR_STATE where not)
            n = ctypes.c_size_t(0)
            if k == 't_f16':        # (the f16 pack of the transposed layer has an entry of its own)
                return eng.lib.pmx_get_transposed_f16_pack(eng._ctx, nm.encode(), None, 0, ctypes.byref(n)) == 5
            return eng.lib.pmx_get_pack(eng._ctx, nm.encode(), eng.PACKS[k], None, 0, ctypes.byref(n)) == 5
        # (the f16 packs of the transposed layers exist from the first f16 backward on: in mode `both` the fp32 legs of the later rounds, and
        #  the profiled step of (c), rewrite them as well -- one more packer launch, counted here)
        kinds = {k: sum(exists(nm, k) for nm in stepped) for k in ('w', 'wino', 't_w', 't_wino', 'f16', 't_f16')}
        fused = int(args.full and exists('conv1_1', 'wino'))
        launches = (int(kinds['w'] > 0) + int(kinds['t_w'] > 0) + int(kinds['f16'] + kinds['t_f16'] > 0) +
                    int(kinds['wino'] - fused + kinds['t_wino'] > 0) + fused)
        extra = dict(packs_in_existence=kinds, pack_launches_per_step=launches, adam_launches_per_step=1)
        if args.grad_precision != '0':
            extra.update(grad_precision=args.grad_precision, loss_scale_log2=args.loss_scale_log2)
        if fa_ms:
            fa, fb = float(np.mean(fa_ms)), float(np.mean(fb_ms))
            extra.update(f16_forward_backward_ms=fa, f16_forward_backward_rounds_ms=fa_ms, f16_with_step_ms=fb, f16_with_step_rounds_ms=fb_ms,
                         f16_step_cost_ms=fb - fa)
        if args.full:
            ha, hb = float(np.mean(ha_ms)), float(np.mean(hb_ms))
            extra.update(head_forward_backward_ms=ha, head_forward_backward_rounds_ms=ha_ms, head_with_step_ms=hb, head_with_step_rounds_ms=hb_ms,
                         head_step_cost_ms=hb - ha)
        # (d) the host route, by wall clock
        eng.train_enable(False)
        state = {nm: [np.zeros(eng.layer_shape(nm), 'f'), np.zeros(eng.layer_shape(nm), 'f'), np.zeros(eng.layer_shape(nm)[0], 'f'),
                      np.zeros(eng.layer_shape(nm)[0], 'f')] for nm in head}
        cur = {nm: [a.copy() for a in weights[nm]] for nm in head}
        leg_a()
        eng.synchronize()
        host, parts = [], []
        for t in (() if args.full or args.no_host else (1, 2)):
            t0 = time.perf_counter()
            grads = {nm: eng.layer_grad(nm) for nm in head}
            t1 = time.perf_counter()
            for nm in head:
                mw, vw, mb, vb = state[nm]
                cur[nm][0] = numpy_adam(cur[nm][0], mw, vw, grads[nm][0], scales.get(nm, 1.0), t)
                cur[nm][1] = numpy_adam(cur[nm][1], mb, vb, grads[nm][1], scales.get(nm, 1.0), t)
            t2 = time.perf_counter()
            for nm in head:
                eng.set_layer(nm, cur[nm][0], cur[nm][1])
            t3 = time.perf_counter()
            leg_a()
            eng.synchronize()
            t4 = time.perf_counter()
            host.append(1e3 * (t4 - t0))
            parts.append(dict(fetch_ms=1e3 * (t1 - t0), numpy_adam_ms=1e3 * (t2 - t1), set_layer_ms=1e3 * (t3 - t2),
                              forward_backward_rebuilding_ms=1e3 * (t4 - t3)))
        a, b = float(np.mean(a_ms)), float(np.mean(b_ms))
        e = dict(batch=B, h=H, w=W, iters=args.iters, warmup=args.warmup, rounds=args.rounds, full=bool(args.full), parameters=n_params,
                 **extra)
        e.update(**{'head_parameters' if not args.full else 'network_parameters': n_params},
                 forward_backward_ms=a, forward_backward_rounds_ms=a_ms, with_step_ms=b, with_step_rounds_ms=b_ms,
                 step_cost_ms=b - a, step_cost_percent=100.0 * (b - a) / a,
                 adam_launch_ms=adam_ms, packers_ms=pack_ms, adam_bytes=28 * n_params, adam_gb_per_s=28e-6 * n_params / adam_ms,
                 copy_same_bytes_ms=copy_ms, copy_runs_ms=copies, copy_gb_per_s=28e-6 * n_params / copy_ms, adam_over_copy_rate=copy_ms / adam_ms,
                 host_route_ms=host, host_route_parts=parts)
        out.append(e)
        print(json.dumps(e), flush=True)
        eng.close()
        del dev
    with open(args.out, 'w') as f:
        json.dump(dict(device='MI355X', note=('--full: (a) and (b) with pmx_backward_trunk and pmx_train_step in backward mode 2, head_* the head '
                                              'step\'s (a) and (b) in the same process; ' if args.full else '') +
                       '(a) forward_backward = hooked retaining forward + pmx_backward_head; (b) with_step = the same + '
                       'pmx_train_step_head; (c) adam_launch / packers = the per-launch profiler\'s labels train_step|adam, train_step|pack; '
                       'copy_same_bytes = hipMemcpyAsync device to device of 14 bytes per parameter (28 moved); (d) host_route = wall clock of '
                       'gradient fetch + NumPy Adam + 82 x pmx_set_layer + the next forward + backward', entries=out), f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
