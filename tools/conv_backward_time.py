#!/usr/bin/env python
"""The three parts of pmx_conv2d_backward (data gradient, weight gradient, mask + bias gradient) at real layer shapes, batch 8 and 32, next
to the FORWARD of the same layer (pmx_conv2d) in the same process -> profiles/conv_backward.json.  For the weight-gradient kernel also the
FLOP it issues to the matrix cores (every MFMA, channel padding included) over the 157.3 TFLOP/s fp32-MFMA peak.

--grad-precision 2 (or both): the 3x3 / 7x7 layers also under option "grad_precision" = 2 (f16 operands, fp32 sums), from the same process,
the fp32 and f16 columns side by side -> profiles/conv_backward_f16.json; the f16 weight gradient's issued FLOP over the 2.52 PFLOP/s f16 peak.
Every measurement step runs under an alarm of its own (--step-timeout seconds): a step that hangs ends the process.

    python tools/conv_backward_time.py [--iters N] [--out PATH] [--grad-precision {0,2,both}]"""
import argparse
import importlib
import json
import os
import signal
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = 'chainer_realtime_multi-person_pose_estimation_amd'
PEAK = 157.3e12
PEAK_F16 = 2.52e15

# name, k, cin, cout, H, W, relu
LAYERS = [('conv4_2', 3, 512, 512, 46, 46, 1), ('Mconv2_stage2', 7, 128, 128, 46, 46, 1), ('Mconv1_stage2', 7, 185, 128, 46, 46, 1),
          ('Mconv7_stage2_L1', 1, 128, 38, 46, 46, 0)]


def strips(B, H, cout, cin, ks):
    """(strips, rows) of the automatic rule (include/pose_mi355x.h; tests/conv_wgrad_twin.c::conv_wgrad_twin_strips)"""
    per = {7: 1, 3: 2, 1: 4}[ks]
    nci, nco = (cin + 31) // 32, (cout + 31) // 32
    units = (nci + per - 1) // per * ks * nco
    s = min((2048 + units - 1) // units, 32, B * H)
    rows = (B * H + s - 1) // s
    return (B * H + rows - 1) // rows, rows


def issued_flop(B, H, W, cout, cin, ks):
    s, rows = strips(B, H, cout, cin, ks)
    pairs = sum((min(rows, B * H - i * rows) * W + 1) // 2 for i in range(s))
    return 4096.0 * ((cout + 31) // 32) * ((cin + 31) // 32) * ks * ks * pairs          # 32 x 32 x 2 x 2 FLOP per MFMA


def strips_f16(B, H, cout, cin, ks, waves=4096):
    """(strips, rows) of the f16 kernel's automatic rule (csrc/wgrad_strips.h: pmx_wgrad_f16_strips)"""
    per = 1 if ks == 7 else 2
    nci, nco = (cin + 31) // 32, (cout + 31) // 32
    blocks = (nco + 3) // 4 * ks * ((nci + per - 1) // per)
    s = min((waves + 4 * blocks - 1) // (4 * blocks), 32, B * H)
    rows = (B * H + s - 1) // s
    return (B * H + rows - 1) // rows, rows


def issued_flop_f16(B, H, W, cout, cin, ks):
    """Every v_mfma_f32_32x32x16_f16 of the launch: one per (16-pixel group of an image row, co tile, ci tile of the blocks, tap)."""
    per = 1 if ks == 7 else 2
    nci, nco = (cin + 31) // 32, (cout + 31) // 32
    return 32768.0 * nco * ((nci + per - 1) // per * per) * ks * ks * B * H * ((W + 15) // 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'conv_backward.json'))
    ap.add_argument('--batches', default='8,32')
    ap.add_argument('--grad-precision', default='0', choices=('0', '2', 'both'))
    ap.add_argument('--step-timeout', type=int, default=120)
    args = ap.parse_args()
    f16 = args.grad_precision != '0'
    if f16 and args.out == ap.get_default('out'):
        args.out = os.path.join(ROOT, 'profiles', 'conv_backward_f16.json')

    def step(fn):          # (no handler installed: an alarm that fires ends the process, also inside a library call)
        signal.alarm(args.step_timeout)
        try:
            return fn()
        finally:
            signal.alarm(0)
    native = importlib.import_module(PKG + '.native')
    eng = native.Engine(0, max_batch=1, max_h=64, max_w=64)
    rng = np.random.default_rng(0)
    out = []
    for B in [int(v) for v in args.batches.split(',')]:
        for name, k, cin, cout, H, W, relu in LAYERS:
            x = rng.standard_normal((B, cin, H, W)).astype('f')
            w = (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype('f')
            b = rng.standard_normal(cout).astype('f')
            dy = rng.standard_normal((B, cout, H, W)).astype('f')
            if f16 and k == 1:
                continue
            _, fwd = step(lambda: eng.conv2d(x, w, b, relu=bool(relu), iters=args.iters))
            r = step(lambda: eng.conv2d_backward(x, w, b, dy, relu=bool(relu), want=('dx', 'dw', 'db'), iters=args.iters))
            flop = 2.0 * B * H * W * cout * cin * k * k
            iss = issued_flop(B, H, W, cout, cin, k)
            s, rows = strips(B, H, cout, cin, k)
            e = dict(layer=name, ksize=k, cin=cin, cout=cout, h=H, w=W, batch=B, relu=relu, iters=args.iters,
                     forward_ms=fwd, dx_ms=r['ms'][0], dw_ms=r['ms'][1], mask_db_ms=r['ms'][2],
                     wgrad_strips=s, wgrad_rows_per_strip=rows, conv_flop=flop, dw_issued_flop=iss,
                     dw_fraction_of_fp32_mfma_peak=iss / (r['ms'][1] * 1e-3) / PEAK,
                     forward_fraction_of_fp32_mfma_peak_algorithmic=flop / (fwd * 1e-3) / PEAK)
            if f16:
                eng.set_option('grad_precision', 2)
                try:
                    h = step(lambda: eng.conv2d_backward(x, w, b, dy, relu=bool(relu), want=('dx', 'dw', 'db'), iters=args.iters))
                finally:
                    eng.set_option('grad_precision', 0)
                s16, rows16 = strips_f16(B, H, cout, cin, k)
                iss16 = issued_flop_f16(B, H, W, cout, cin, k)
                e.update(dx_f16_ms=h['ms'][0], dw_f16_ms=h['ms'][1], wgrad_f16_strips=s16, wgrad_f16_rows_per_strip=rows16,
                         dw_f16_issued_flop=iss16, dw_f16_fraction_of_f16_mfma_peak=iss16 / (h['ms'][1] * 1e-3) / PEAK_F16,
                         dw_f16_over_fp32=h['ms'][1] / r['ms'][1], dx_f16_over_fp32=h['ms'][0] / r['ms'][0])
            out.append(e)
            print(json.dumps(e), flush=True)
    eng.close()
    with open(args.out, 'w') as f:
        json.dump(dict(device='MI355X', peak_fp32_mfma_flops=PEAK, peak_f16_mfma_flops=PEAK_F16, note='dw_ms includes the combine launch; the fractions of dw count every '
                       'issued MFMA (channel padding included), the forward fraction is algorithmic FLOP (Winograd forms issue fewer)',
                       entries=out), f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
