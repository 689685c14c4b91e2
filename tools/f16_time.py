#!/usr/bin/env python
"""The opt-in f16 inference mode (option "precision" = 2) against the fp32 default, one process, the two interleaved: frames/s at batch 32
and ms per image at batches 1 and 8 (368 x 368, the bench's calibrated synthetic frames, device-resident), detect_precise on a 482 x 642
frame, the per-layer profile in f16 mode with the dominant kernel's fraction of the f16 dense peak, and how far the f16 results are from
the fp32 ones on the same frames (map error, peaks, people).  usage: f16_time.py [out.json] (default profiles/f16_mode.json)"""
import importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
native = importlib.import_module(bench.PKG + '.native')
weights_mod = importlib.import_module(bench.PKG + '.weights')
PD = importlib.import_module(bench.PKG + '.pose_detector')

F16_PEAK_TFLOPS = 2516.6        # MI355X dense f16 MFMA: 256 CUs x 2.4 GHz x 4 SIMDs x 32768 FLOP / 32 cycles
S, MAP = 368, 320
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'f16_mode.json')

eng = native.Engine(0, max_batch=32, max_h=S, max_w=S)
wts = weights_mod.synthetic_weights(0)
eng.set_weights(wts)
eng.forward_u8(np.random.default_rng(1234).integers(0, 256, (1, S, S, 3), dtype=np.uint8))
paf, heat = eng.get_maps()
wts = weights_mod.calibrate_head(wts, paf[0], heat[0])
eng.set_weights({k: wts[k] for k in ('Mconv7_stage6_L1', 'Mconv7_stage6_L2')})
imgs = np.random.default_rng(1).integers(0, 256, (32, S, S, 3), dtype=np.uint8)
d_imgs = torch.from_numpy(imgs).to('cuda:0')
torch.cuda.synchronize()


def step(B):
    eng.detect_batch(device_ptr=d_imgs.data_ptr(), shape=(B, S, S), map_h=MAP, map_w=MAP)
    return eng.results()


def timed(B, n):
    for _ in range(2):
        step(B)
    t0 = time.perf_counter()
    for _ in range(n):
        step(B)
    return (time.perf_counter() - t0) / n * 1e3


res = {'what': __doc__.split('usage')[0].strip(), 'f16_peak_tflops': F16_PEAK_TFLOPS, 'modes': {}}
ms = {0: {}, 2: {}}
for rnd in range(3):                    # interleaved rounds, best of each
    for mode in (0, 2):
        eng.set_option('precision', mode)
        for B, n in ((32, 5), (8, 10), (1, 20)):
            v = timed(B, n)
            ms[mode][B] = min(ms[mode].get(B, 1e9), v)
for mode in (0, 2):
    res['modes']['f16' if mode else 'f32'] = {
        'batch32_ms': ms[mode][32], 'batch32_fps': 32e3 / ms[mode][32],
        'batch8_ms_per_image': ms[mode][8] / 8, 'batch1_ms_per_image': ms[mode][1]}
res['speedup_batch32'] = ms[0][32] / ms[2][32]

# agreement on the 32 frames: maps, peaks, people
outs = {}
for mode in (0, 2):
    eng.set_option('precision', mode)
    r = step(32)
    p, h = eng.get_maps()
    outs[mode] = (p, h, [eng.peaks(b) for b in range(32)], [int(x) for x in r['n_people']])
scale = max(float(np.abs(outs[0][0]).max()), float(np.abs(outs[0][1]).max()), 1.0)
map_err = max(float(np.abs(outs[2][0] - outs[0][0]).max()), float(np.abs(outs[2][1] - outs[0][1]).max())) / scale
peaks_same = sum(int(a.shape == b.shape and np.array_equal(a[:, [0, 1, 2, 4]], b[:, [0, 1, 2, 4]])) for a, b in zip(outs[2][2], outs[0][2]))
n_peaks = [(len(a), len(b)) for a, b in zip(outs[2][2], outs[0][2])]
res['agreement_batch32'] = {
    'map_err_rel': map_err, 'frames': 32, 'frames_identical_peak_list': peaks_same,
    'peaks_f16_total': sum(a for a, _ in n_peaks), 'peaks_f32_total': sum(b for _, b in n_peaks),
    'frames_same_people_count': sum(int(a == b) for a, b in zip(outs[2][3], outs[0][3])),
    'people_f16_total': sum(outs[2][3]), 'people_f32_total': sum(outs[0][3])}

# per-layer profile of one batch-32 forward in f16 mode
eng.set_option('precision', 2)
step(32)
eng.profile_reset(); eng.profile_enable(True)
step(32)
prof = eng.profile()
eng.profile_enable(False)
rows = sorted(prof, key=lambda e: -e['total_ms'])
res['profile_f16_batch32'] = rows
conv = [e for e in rows if e['kernel'].startswith('conv_f16')]
dom = [e for e in conv if e['kernel'] == 'conv_f16_7x7']
t7 = sum(e['total_ms'] for e in dom)
res['dominant_kernel'] = {
    'kernel': 'conv_f16_7x7', 'ms': t7, 'share_of_profiled_ms': t7 / sum(e['total_ms'] for e in rows),
    'issued_tflops': sum(e['issued_flop_per_launch'] * e['launches'] for e in dom) / t7 / 1e9,
    'algorithmic_tflops': sum(e['flop_per_launch'] * e['launches'] for e in dom) / t7 / 1e9}
res['dominant_kernel']['fraction_of_f16_peak'] = res['dominant_kernel']['issued_tflops'] / F16_PEAK_TFLOPS
res['f16_3x3_ms'] = sum(e['total_ms'] for e in conv if e['kernel'] == 'conv_f16_3x3')
eng.close()

# detect_precise on one 482 x 642 frame
frame = np.random.default_rng(7).integers(0, 256, (482, 642, 3), dtype=np.uint8)
prec = {}
for prc in ('f32', 'f16'):
    det = PD.PoseDetector(weights=wts, device=0, precise=True, precision=prc)
    det(frame)
    best = 1e9
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        poses, _ = det(frame)
        best = min(best, (time.perf_counter() - t0) * 1e3)
    prec[prc] = {'ms': best, 'people': len(poses)}
    det.engine.close()
res['detect_precise_482x642'] = prec
json.dump(res, open(out_path, 'w'), indent=1)
print(json.dumps({k: v for k, v in res.items() if k != 'profile_f16_batch32'}, indent=1))
