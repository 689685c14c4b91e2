#!/usr/bin/env python
"""The three parts of pmx_conv2d_backward (data gradient, weight gradient, mask + bias gradient) at real layer shapes, batch 8 and 32, next
to the FORWARD of the same layer (pmx_conv2d) in the same process -> profiles/conv_backward.json.  For the weight-gradient kernel also the
FLOP it issues to the matrix cores (every MFMA, channel padding included) over the 157.3 TFLOP/s fp32-MFMA peak.

    python tools/conv_backward_time.py [--iters N] [--out PATH]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = 'chainer_realtime_multi-person_pose_estimation_amd'
PEAK = 157.3e12

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'conv_backward.json'))
    ap.add_argument('--batches', default='8,32')
    args = ap.parse_args()
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
            _, fwd = eng.conv2d(x, w, b, relu=bool(relu), iters=args.iters)
            r = eng.conv2d_backward(x, w, b, dy, relu=bool(relu), want=('dx', 'dw', 'db'), iters=args.iters)
            flop = 2.0 * B * H * W * cout * cin * k * k
            iss = issued_flop(B, H, W, cout, cin, k)
            s, rows = strips(B, H, cout, cin, k)
            e = dict(layer=name, ksize=k, cin=cin, cout=cout, h=H, w=W, batch=B, relu=relu, iters=args.iters,
                     forward_ms=fwd, dx_ms=r['ms'][0], dw_ms=r['ms'][1], mask_db_ms=r['ms'][2],
                     wgrad_strips=s, wgrad_rows_per_strip=rows, conv_flop=flop, dw_issued_flop=iss,
                     dw_fraction_of_fp32_mfma_peak=iss / (r['ms'][1] * 1e-3) / PEAK,
                     forward_fraction_of_fp32_mfma_peak_algorithmic=flop / (fwd * 1e-3) / PEAK)
            out.append(e)
            print(json.dumps(e), flush=True)
    eng.close()
    with open(args.out, 'w') as f:
        json.dump(dict(device='MI355X', peak_fp32_mfma_flops=PEAK, note='dw_ms includes the combine launch; the fractions of dw count every '
                       'issued MFMA (channel padding included), the forward fraction is algorithmic FLOP (Winograd forms issue fewer)',
                       entries=out), f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
