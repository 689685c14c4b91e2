#!/usr/bin/env python3
"""Time the face / hand chain of the reference demo (demo.py:30-55) on the dinner golden image with all of its people:

  (a) serial   the chain exactly as demo.py orders it: per person get_unit_length, crop_face -> FaceDetector, crop_hands -> HandDetector
               (left, then right), one network call per crop
  (b) batched  face_hand_detector.detect_person_parts: one detect_boxes call per detector
  (c) boxes    FaceDetector.detect_boxes alone at n = 1, 2, 4, 8, 16, 32 boxes (the dinner face boxes, repeated)

  (d) batch    32 frames at once (`--legs d`, written to profiles/face_hand_batch.json): (d1) a loop of detect_person_parts over the
               frames against (d2) ONE detect_people_parts call, alternating in one process, detectors with max_batch = 32; two
               workloads: "mixed" cycles the images and golden poses of e2e_person / e2e_people / e2e_dinner, "single_person" is 32
               copies of the dinner image with dinner pose 1 alone (one face crop and one left-hand crop per frame)

Host clock around synchronised work (every call returns host results), a warm-up of every shape first, `--repeats` timed runs;
median, min, max and the spread are written as JSON.  Weights: tests/golden/e2e_dinner.npz (posenet) and the synthetic facenet /
handnet seeds of tests/golden/demo_chain_dinner.npz.

    python tools/face_hand_chain_time.py [--repeats 20] [--out profiles/face_hand_chain.json] [--only b]
    python tools/face_hand_chain_time.py --legs d [--repeats 20] [--out profiles/face_hand_batch.json] [--only d2]

`--only b` / `--only d2` runs (b) / (d2, mixed workload) once after a warm-up and nothing else (for a `rocprofv3 --kernel-trace --stats`
run of its own).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import __graft_entry__ as ge  # noqa: E402

PD, FH, W = ge._pkg('pose_detector'), ge._pkg('face_hand_detector'), ge._pkg('weights')


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts.min()), max_ms=float(ts.max()),
                spread_pct=float((ts.max() - ts.min()) / np.median(ts) * 100), repeats=len(ts))


def timed(fn, repeats):
    fn()                                   # warm-up of this shape
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return stats(out)


def batch_workloads(load_e2e, det, frames=32):
    """{name: (imgs, poses_per_image)} of leg (d); the golden poses need no pose network"""
    gs = [load_e2e(n) for n in ('e2e_person', 'e2e_people', 'e2e_dinner')]
    mixed = ([gs[i % 3]['img'] for i in range(frames)], [gs[i % 3]['poses'] for i in range(frames)])
    dinner = gs[2]
    pose = np.array(dinner['poses'][1:2], copy=True)
    unit = det.get_unit_length(pose[0])
    hb = det.hand_bboxes(pose[0], unit)
    assert det.face_bbox(pose[0], unit) is not None and hb['left'] is not None and hb['right'] is None
    return {'mixed': mixed, 'single_person': ([dinner['img']] * frames, [pose] * frames)}


def leg_d(args, load_e2e):
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'demo_chain_dinner.npz'))
    det = object.__new__(PD.PoseDetector)            # host helpers only
    fdet = FH.FaceDetector('facenet', weights=W.synthetic_weights(int(z['face_seed']), 'facenet'), device=0, max_batch=32)
    hdet = FH.HandDetector('handnet', weights=W.synthetic_weights(int(z['hand_seed']), 'handnet'), device=0, max_batch=32)
    loads = batch_workloads(load_e2e, det)

    def d1(imgs, poses):
        return [FH.detect_person_parts(det, fdet, hdet, im, p) for im, p in zip(imgs, poses)]

    def d2(imgs, poses):
        return FH.detect_people_parts(det, fdet, hdet, imgs, poses)

    if args.only == 'd2':
        d2(*loads['mixed'])
        d2(*loads['mixed'])
        return 0
    res = dict(frames=32, max_batch=32, clock='host perf_counter around synchronised calls, warm-up of every shape first, legs alternate',
               workloads={})
    for name, (imgs, poses) in loads.items():
        for _ in range(2):                           # warm-up of every shape of both legs (the engines grow to 32 in d2)
            parts = d2(imgs, poses)
            d1(imgs, poses)
        t1, t2 = [], []
        for _ in range(args.repeats):
            t0 = time.perf_counter(); d1(imgs, poses); t1.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); d2(imgs, poses); t2.append(time.perf_counter() - t0)
        r = dict(face_crops=sum(p['face'] is not None for ps in parts for p in ps),
                 hand_crops=sum((p['left'] is not None) + (p['right'] is not None) for ps in parts for p in ps),
                 d1_loop_of_detect_person_parts=stats(t1), d2_detect_people_parts=stats(t2))
        r['ratio_d1_over_d2'] = r['d1_loop_of_detect_person_parts']['median_ms'] / r['d2_detect_people_parts']['median_ms']
        res['workloads'][name] = r
    txt = json.dumps(res, indent=1)
    print(txt)
    out = args.out or os.path.join(ROOT, 'profiles', 'face_hand_batch.json')
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        f.write(txt + '\n')
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--only', default=None, choices=['b', 'd2'])
    ap.add_argument('--legs', default='abc', choices=['abc', 'd'])
    args = ap.parse_args()
    from test_reference_network import load_e2e
    if args.legs == 'd' or args.only == 'd2':
        return leg_d(args, load_e2e)
    g = load_e2e('e2e_dinner')
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'demo_chain_dinner.npz'))
    img = g['img']
    det = PD.PoseDetector(weights=g['weights'], device=0)
    poses, _ = det(img)
    fdet = FH.FaceDetector('facenet', weights=W.synthetic_weights(int(z['face_seed']), 'facenet'), device=0)
    hdet = FH.HandDetector('handnet', weights=W.synthetic_weights(int(z['hand_seed']), 'handnet'), device=0)
    # serial detectors of their own: batch-1 engines, as the reference's
    fdet1 = FH.FaceDetector('facenet', weights=W.synthetic_weights(int(z['face_seed']), 'facenet'), device=0)
    hdet1 = FH.HandDetector('handnet', weights=W.synthetic_weights(int(z['hand_seed']), 'handnet'), device=0)

    def serial():
        for pose in np.array(poses, copy=True):
            unit = det.get_unit_length(pose)
            face, bbox = det.crop_face(img, pose, unit)
            if face is not None:
                fdet1(face)
            hands = det.crop_hands(img, pose, unit)
            for side in ('left', 'right'):
                if hands[side] is not None:
                    hdet1(hands[side]['img'], hand_type=side)

    def batched():
        return FH.detect_person_parts(det, fdet, hdet, img, poses)

    if args.only == 'b':
        batched()
        batched()
        return 0
    parts = batched()
    n_face = sum(p['face'] is not None for p in parts)
    n_hand = sum((p['left'] is not None) + (p['right'] is not None) for p in parts)
    res = dict(image='e2e_dinner', people=len(poses), face_crops=n_face, hand_crops=n_hand,
               clock='host perf_counter around synchronised calls, warm-up of every shape first')
    res['a_serial'] = timed(serial, args.repeats)
    res['b_detect_person_parts'] = timed(batched, args.repeats)
    res['ratio_a_over_b'] = res['a_serial']['median_ms'] / res['b_detect_person_parts']['median_ms']
    face_boxes = [p['face']['bbox'] for p in parts if p['face'] is not None]
    res['c_detect_boxes_facenet'] = {}
    for n in (1, 2, 4, 8, 16, 32):
        boxes = [face_boxes[i % len(face_boxes)] for i in range(n)]
        r = timed(lambda: fdet.detect_boxes(img, boxes), args.repeats)
        r['ms_per_box'] = r['median_ms'] / n
        res['c_detect_boxes_facenet'][str(n)] = r
    # one face crop through the serial path, for the per-box comparison
    face0 = det.crop_image(img, face_boxes[0])
    res['c_serial_one_face_call'] = timed(lambda: fdet1(face0), args.repeats)
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(txt + '\n')
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
