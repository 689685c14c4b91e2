#!/usr/bin/env python
"""detect_precise over a COCO-like stream of mixed-size frames (the size classes of bench.mixed_sizes_mode), ms per image for n = 1, 4, 8, 16:
  (a) one detect_precise per image (default options: four prioritised lanes; maps not fetched, as in bench.precise_mode),
  (b) the image-list path (every (image, scale) pair a segment of one forward on one stream: pmx_detect_precise_images),
  (c) the same-size batch-of-8 path on 482 x 642 frames (yardstick),
in fp32 and in f16 mode, with bench.precise_mode's synthetic weights and calibrated head.  Every shape is warmed up first; (a) and (b)
alternate within one process over --repeats repetitions (min / median / max reported).  Each GPU_MAX_HW_QUEUES setting (2 and 4) runs in
a fresh child process with the variable passed explicitly; it is never changed inside a process.  Also a per-kernel profile (pmx_profile_*)
of one (b) call at n = 8 in fp32.
usage: precise_images_time.py [--out profiles/precise_images.json] [--repeats 3]"""
import argparse, importlib, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

CLASSES = [(480, 640), (640, 480), (427, 640), (375, 500), (640, 640), (426, 640), (480, 640), (333, 500), (500, 375), (640, 427)]
NS = (1, 4, 8, 16)


def child(repeats):
    import bench
    PD = importlib.import_module(bench.PKG + '.pose_detector')
    W = importlib.import_module(bench.PKG + '.weights')
    H, Wd = 482, 642
    frame = np.random.default_rng(55).integers(0, 256, (H, Wd, 3), dtype=np.uint8)
    wts = W.synthetic_weights(0)
    det = PD.PoseDetector(weights=wts, device=0, max_size=(744, 984))
    cal = PD.resize_cubic_u8(frame, int(np.ceil(Wd * 368 / min(H, Wd))), int(np.ceil(H * 368 / min(H, Wd))))
    cal, _ = det.pad_image(cal, 8, (104, 117, 123))
    det.engine.forward_u8(cal[None])
    paf0, heat0 = det.engine.get_maps()
    det.engine.close()
    wts = W.calibrate_head(wts, paf0[0], heat0[0], heat_s=0.2, heat_t=-0.2, paf_s=1.2)
    rng = np.random.default_rng(7)
    sizes = [CLASSES[int(rng.integers(0, len(CLASSES)))] for _ in range(max(NS))]
    stream = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in sizes]
    same8 = [frame] + [np.random.default_rng(56 + i).integers(0, 256, (H, Wd, 3), dtype=np.uint8) for i in range(7)]
    out = {'GPU_MAX_HW_QUEUES': os.environ.get('GPU_MAX_HW_QUEUES'), 'frames': ['%dx%d' % s for s in sizes], 'precisions': {}}

    def per_image(fn, n):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) / n * 1e3

    for prec in ('f32', 'f16'):
        da = PD.PoseDetector(weights=wts, device=0, max_size=(744, 984), precision=prec)        # (a): one call per image
        db = PD.PoseDetector(weights=wts, device=0, precision=prec)                           # (b): the image-list path
        dc = PD.PoseDetector(weights=wts, device=0, max_size=(744, 984), precision=prec)        # (c): same-size batch of 8
        run_a = lambda n: [_quiet(lambda im=im: da._detect_precise_device(im, fetch_maps=False)) for im in stream[:n]]
        run_b = lambda n: _quiet(lambda: db._detect_precise_mixed(stream[:n], False, True))
        run_c = lambda: _quiet(lambda: dc.detect_precise_batch(same8, return_exceptions=True))
        for n in NS:                                   # warm-up: every shape, every context at its final capacity
            run_a(n); run_b(n)
        run_c()
        a = {n: [] for n in NS}
        b = {n: [] for n in NS}
        c = []
        for _ in range(repeats):
            for n in NS:
                a[n].append(per_image(lambda: run_a(n), n))
                b[n].append(per_image(lambda: run_b(n), n))
            c.append(per_image(run_c, 8))
        st = lambda v: {'min': min(v), 'median': float(np.median(v)), 'max': max(v), 'runs': v}
        res = {'one_call_per_image_ms': {str(n): st(a[n]) for n in NS}, 'image_list_ms': {str(n): st(b[n]) for n in NS},
               'same_size_batch8_482x642_ms': st(c),
               'image_list_calls': {str(n): len(PD.precise_chunks([1] * n, 1 << 60, min(n, db.precise_images_per_call))) for n in NS},
               'speedup_list_vs_one_call': {str(n): float(np.median(a[n]) / np.median(b[n])) for n in NS}}
        if prec == 'f32':
            db.engine.profile_reset(); db.engine.profile_enable(1)
            run_b(8)
            prof = db.engine.profile()
            db.engine.profile_enable(False)
            by = {}
            for p in prof:
                k = bench.rocprof_kernel(p['kernel']) if p['kernel'].startswith('conv') else p['kernel']
                e = by.setdefault(k, [0.0, 0])
                e[0] += p['total_ms']; e[1] += p['launches']
            tot = sum(v[0] for v in by.values())
            res['profile_n8'] = {'kernel_ms_total': tot, 'kernel_ms_per_image': tot / 8,
                                 'by_kernel': [{'kernel': k, 'ms': v[0], 'launches': v[1], 'share': v[0] / tot}
                                               for k, v in sorted(by.items(), key=lambda kv: -kv[1][0])]}
        out['precisions'][prec] = res
        for d in (da, db, dc):
            d.engine.close()
    return out


def _quiet(fn):
    try:
        return fn()
    except IndexError:               # (the reference raises it too on a third subset match, pose_detector.py:197)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'precise_images.json'))
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--child', default=None)
    a = ap.parse_args()
    if a.child:
        json.dump(child(a.repeats), open(a.child, 'w'), indent=1)
        return 0
    runs = {}
    for q in ('2', '4'):
        tmp = a.out + '.hwq%s.tmp' % q
        env = dict(os.environ, GPU_MAX_HW_QUEUES=q)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', tmp, '--repeats', str(a.repeats)], env=env, timeout=900)
        if r.returncode:
            print('child with GPU_MAX_HW_QUEUES=%s failed: %d' % (q, r.returncode))
            return r.returncode
        runs[q] = json.load(open(tmp))
        os.remove(tmp)
    summary = {}
    for prec in ('f32', 'f16'):
        m = lambda q, key, n: runs[q]['precisions'][prec][key][str(n)]['median']
        summary[prec] = {
            'image_list_ms_hwq2_vs_hwq4_rel_diff': {str(n): abs(m('2', 'image_list_ms', n) - m('4', 'image_list_ms', n)) / m('4', 'image_list_ms', n) for n in NS},
            'one_call_ms_hwq2_vs_hwq4_rel_diff': {str(n): abs(m('2', 'one_call_per_image_ms', n) - m('4', 'one_call_per_image_ms', n)) / m('4', 'one_call_per_image_ms', n)
                                                  for n in NS},
            'hwq4_n8': {'one_call_per_image_ms': m('4', 'one_call_per_image_ms', 8), 'image_list_ms': m('4', 'image_list_ms', 8),
                        'same_size_batch8_ms': runs['4']['precisions'][prec]['same_size_batch8_482x642_ms']['median']}}
    res = {'tool': 'tools/precise_images_time.py', 'repeats': a.repeats, 'summary': summary, 'by_hw_queues': runs}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, 'w'), indent=1)
    print(json.dumps(summary, indent=1))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
