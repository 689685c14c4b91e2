#!/usr/bin/env python
"""ms of Engine creation (pmx_create: every fixed-size buffer of a context) and of close (pmx_destroy: every buffer freed), the bench's
context size (batch 32, 368 x 368), median and range of 10 after one warm-up.  usage: context_create_time.py"""
import importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import bench
native = importlib.import_module(bench.PKG + '.native')
t_new, t_close = [], []
for i in range(11):
    t0 = time.perf_counter(); eng = native.Engine(0, max_batch=32, max_h=368, max_w=368); eng.synchronize()
    t1 = time.perf_counter(); eng.close(); t2 = time.perf_counter()
    if i: t_new.append((t1 - t0) * 1e3); t_close.append((t2 - t1) * 1e3)
print(json.dumps({'create_ms': {'median': float(np.median(t_new)), 'min': min(t_new), 'max': max(t_new)},
                  'close_ms': {'median': float(np.median(t_close)), 'min': min(t_close), 'max': max(t_close)}}))
