#!/usr/bin/env python
"""Per-step figures of a `rocprofv3 --kernel-trace --output-format csv` run of `bench.py --gpus 1 --steps K --warmup W` for the two
half-batch chains (option "batch_chains"; EXPERIMENTS.md): the step time, the summed duration of the launches that leave CUs idle
(unit-mode tails, their combine, the post-process) and the time during which two or more kernels are in flight at once -- in the
one-chain form nothing overlaps, in the two-chain form that is the time the chains share the chip.

    python tools/chain_trace.py TRACE_kernel_trace.csv --steps 20 --chains 1 --out profiles/batch_chains_before.json

A step starts with its conv1 launch (one per chain); the timed steps are the last K of the trace."""
import argparse
import csv
import json
import re

UNDERFILLED = [('unit_tails', r'conv_wino_kernel<\d, 0, 1, [03]>'), ('tail_combine', r'conv_wino_tail_reduce_kernel'),
               ('postprocess', r'\bpp_(clear|peaks|peaks_fast|sort|limbs|group)_kernel')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('csv')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--chains', type=int, default=1, help='conv1 launches per step (2 when the batch runs as two chains)')
    ap.add_argument('--out', required=True)
    ap.add_argument('--note', default='')
    a = ap.parse_args()
    rows = []
    with open(a.csv, newline='') as f:
        for r in csv.DictReader(f):
            rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name']))
    rows.sort()
    marks = [i for i, r in enumerate(rows) if re.search(r'conv1_(wino|fused)_kernel', r[2])]
    need = a.steps * a.chains
    assert len(marks) >= need, (len(marks), need)
    first = marks[-need]
    win = rows[first:]
    t0, t1 = win[0][0], max(r[1] for r in win)
    per = {name: 0.0 for name, _ in UNDERFILLED}
    count = {name: 0 for name, _ in UNDERFILLED}
    busy = 0.0
    for s, e, k in win:
        busy += e - s
        for name, pat in UNDERFILLED:
            if re.search(pat, k):
                per[name] += e - s
                count[name] += 1
    # time with >= 1 and >= 2 kernels in flight (sweep over the start / end stamps)
    ev = sorted([(s, 1) for s, _, _ in win] + [(e, -1) for _, e, _ in win])
    depth, last, any_ns, two_ns = 0, t0, 0, 0
    for t, d in ev:
        if depth >= 1:
            any_ns += t - last
        if depth >= 2:
            two_ns += t - last
        depth += d
        last = t
    ms = lambda ns: round(ns / 1e6 / a.steps, 4)
    out = {
        'source': 'rocprofv3 --kernel-trace of bench.py --gpus 1 --steps %d (no counters in the same run)' % a.steps,
        'note': a.note,
        'steps': a.steps, 'launches_per_step': round(len(win) / a.steps, 2),
        'step_ms': ms(t1 - t0),
        'kernel_ms_per_step_summed': ms(busy),
        'gpu_busy_ms_per_step': ms(any_ns),
        'overlap_ms_per_step': ms(two_ns),
        'underfilled_ms_per_step': {k: ms(v) for k, v in per.items()},
        'underfilled_launches_per_step': {k: round(v / a.steps, 2) for k, v in count.items()},
        'underfilled_total_ms_per_step': ms(sum(per.values())),
        'last_round_skew_of_plain_launches': 'unmeasured: a kernel trace has no per-block data',
    }
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
