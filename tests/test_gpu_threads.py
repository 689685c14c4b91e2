"""GPU: one context per host thread (include/pose_mi355x.h).  Contexts on their own threads -- ctypes releases the GIL for every library
call, so the calls really overlap -- give bit for bit what the same call scripts (context_scripts.py) give serially in the main thread:
pose contexts side by side, on their own streams and on a torch stream per thread; a pose, a facenet and a render context while a fourth
thread creates and destroys contexts; pmx_last_error per thread; and a fresh process whose first GPU work is two threads at once.

Threads are plain threading.Threads behind a Barrier; an exception in a thread is re-raised by the test; every join has a time limit sized
from the serial run and a thread still alive then fails the test.  Every loop has a small fixed count."""
import json
import os
import subprocess
import sys
import threading
import time
import traceback

import numpy as np
import pytest

import context_scripts as CS
from conftest import ROOT
from test_gpu_context_lifetime import PARENT_DRIFT

pytestmark = pytest.mark.gpu

ROUNDS = 3
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'threads_child.py')


@pytest.fixture(scope='module', autouse=True)
def _torch_runtime_first():
    """torch brings its own HIP runtime; it initialises only while the library's has not opened the device yet in this process (run alone,
    this module would otherwise create its engines first).  With torch first, the library and torch share one runtime, and a torch stream's
    handle is a stream of the library's runtime too."""
    import torch
    torch.cuda.init()


@pytest.fixture(scope='module')
def pose_w(native):
    return CS.pose_weights(native)


@pytest.fixture(scope='module')
def face_w():
    return CS.face_weights()


def _serial(native, cfg, weights, script):
    """(the script's result, seconds it took with the context's setup) in the calling thread"""
    t0 = time.perf_counter()
    eng = native.Engine(0, **cfg)
    try:
        if weights is not None:
            eng.set_weights(weights)
        out = script(eng)
    finally:
        eng.close()
    return out, time.perf_counter() - t0


@pytest.fixture(scope='module')
def refs(native, pose_w, face_w):
    """the serial runs in the main thread: {kind: result}, and the seconds of the slowest"""
    out, secs = {}, 0.0
    for kind, cfg, w, script in (('pose', CS.POSE, pose_w, CS.pose_script), ('face', CS.FACE, face_w, CS.face_script),
                                 ('render', CS.RENDER, None, CS.render_script)):
        out[kind], t = _serial(native, cfg, w, script)
        secs = max(secs, t)
    assert int(out['pose']['batch2.0.info'][1]) > 0 and len(out['pose']['precise.peaks']) > 0          # (peaks: the records say something)
    assert CS.same(_serial(native, CS.POSE, pose_w, CS.pose_script)[0], out['pose']) is None          # (and the script is reproducible)
    return out, secs


def _limit(serial_seconds, n_threads, rounds=ROUNDS):
    """join limit: five times what the threads' work takes one after the other, and a floor for a loaded machine"""
    return 30.0 + 5.0 * serial_seconds * n_threads * rounds


def run_threads(targets, limit):
    """targets: callables taking the shared barrier.  Starts them behind it, joins each within `limit` seconds in all, fails on a thread
    that is still alive, re-raises the first exception of a thread."""
    barrier = threading.Barrier(len(targets))
    errors = []

    def wrap(fn):
        try:
            barrier.wait(timeout=limit)
            fn(barrier)
        except BaseException as e:      # noqa: B902 (whatever it is, the test must see it)
            errors.append((e, traceback.format_exc()))
            barrier.abort()

    threads = [threading.Thread(target=wrap, args=(fn,), daemon=True) for fn in targets]
    deadline = time.monotonic() + limit
    for t in threads:
        t.start()
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    alive = [k for k, t in enumerate(threads) if t.is_alive()]
    assert not alive, 'threads %r still running after %.0f s' % (alive, limit)
    first = [e for e in errors if not isinstance(e[0], threading.BrokenBarrierError)] or errors
    if first:
        print(first[0][1])
        raise first[0][0]


def _rounds(eng, script, want, what, barrier, limit, rounds=ROUNDS):
    for r in range(rounds):
        barrier.wait(timeout=limit)
        diff = CS.same(script(eng), want)
        assert diff is None, '%s, round %d: %s' % (what, r, diff)


# ---- B1. pose contexts side by side ---------------------------------------------------------------------------------------------------
# the four kernel-form switches of a context ("same bits" in the header; both LDS floors below the 160 KB a kernel may be granted)
FORM_SWITCHES = (('pp_generic', 1), ('cubic_rows', 0), ('conv_v5_lds', 64 * 1024), ('conv_min_lds', 60 * 1024))


@pytest.mark.parametrize('n, own_stream, switches', [(2, True, False), (2, False, False), (4, True, False), (4, False, False), (2, True, True)],
                         ids=['2-own_streams', '2-torch_streams', '4-own_streams', '4-torch_streams', '2-own_streams-form_switches'])
def test_pose_contexts_on_their_own_threads(native, pose_w, refs, n, own_stream, switches):
    """switches: thread 1 sets FORM_SWITCHES on ITS context while thread 0 runs at the defaults -- both forms of the peaks kernel, of the
    cubic resize and of the direct kernels' LDS floors side by side in one process, both equal to the serial default reference"""
    import torch
    torch.cuda.init()
    ref, secs = refs
    limit = _limit(secs, n)

    def worker(k):
        def run(barrier):
            eng = native.Engine(0, **CS.POSE)
            try:
                eng.set_weights(pose_w)
                if not own_stream:
                    stream = torch.cuda.Stream()
                    assert stream.cuda_stream != 0
                    eng.set_stream(stream.cuda_stream)
                if switches and k == 1:
                    for key, value in FORM_SWITCHES:
                        eng.set_option(key, value)
                _rounds(eng, CS.pose_script, ref['pose'], 'thread %d of %d' % (k, n), barrier, limit)
                eng.set_stream(0)
            finally:
                eng.close()
        return run

    run_threads([worker(k) for k in range(n)], limit)


# ---- B2. mixed work, and contexts destroyed under the others --------------------------------------------------------------------------
def test_mixed_contexts_while_another_thread_creates_and_destroys(native, pose_w, face_w, refs):
    """pmx_destroy runs hipDeviceSynchronize and hipFree under the other threads' launches.  Afterwards the device has all its memory
    back: the free-memory reading agrees with the one before within test_gpu_context_lifetime's PARENT_DRIFT."""
    import torch
    ref, secs = refs
    limit = _limit(secs, 4)
    small_ref, _ = _serial(native, dict(max_batch=2, max_h=96, max_w=128), pose_w, CS.pose_script)

    def scripted(cfg, w, script, want, what):
        def run(barrier):
            eng = native.Engine(0, **cfg)
            try:
                if w is not None:
                    eng.set_weights(w)
                _rounds(eng, script, want, what, barrier, limit)
            finally:
                eng.close()
        return run

    def churn(barrier):
        for r in range(ROUNDS):
            barrier.wait(timeout=limit)
            got, _ = _serial(native, dict(max_batch=2, max_h=96, max_w=128), pose_w, CS.pose_script)
            diff = CS.same(got, small_ref)
            assert diff is None, 'created and destroyed, round %d: %s' % (r, diff)

    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info(0)[0]
    run_threads([scripted(CS.POSE, pose_w, CS.pose_script, ref['pose'], 'pose thread'),
                 scripted(CS.FACE, face_w, CS.face_script, ref['face'], 'face thread'),
                 scripted(CS.RENDER, None, CS.render_script, ref['render'], 'render thread'), churn], limit)
    torch.cuda.synchronize()
    after = torch.cuda.mem_get_info(0)[0]
    print('free device memory: %d bytes before, %d after, drift %d (allowed %d)' % (before, after, abs(after - before), PARENT_DRIFT))
    assert abs(after - before) <= PARENT_DRIFT, (before, after)


# ---- B3. pmx_last_error is thread-local -----------------------------------------------------------------------------------------------
def test_last_error_is_per_thread(native, pose_w):
    """Thread A makes host-side argument errors (refused before anything is enqueued) while thread B runs forwards: A reads its own
    messages, B's calls succeed and B never sees A's text."""
    limit = 60.0
    cfg = dict(max_batch=2, max_h=96, max_w=128)
    want, _ = _serial(native, cfg, pose_w, CS.pose_script)
    ok_img = CS.u8(301, 1, 64, 96)
    seen_a, seen_b = [], []

    def thread_a(barrier):
        eng = native.Engine(0, **cfg)
        try:
            eng.set_weights(pose_w)
            for i in range(10):
                barrier.wait(timeout=limit)
                for imgs, code, text in ((CS.u8(302, 1, 60, 64), 1, 'multiples of 8 (got 60 x 64)'), (CS.u8(303, 3, 64, 96), 5, 'batch 3 outside 1..2')):
                    with pytest.raises(native.PmxError) as err:
                        eng.forward_u8(imgs)
                    seen_a.append((err.value.code, str(err.value)))
                    assert err.value.code == code and text in str(err.value), (i, err.value.code, str(err.value))
                    assert text in eng.lib.pmx_last_error().decode()
            diff = CS.same(CS.pose_script(eng), want)
            assert diff is None, 'the context of the failing calls afterwards: %s' % diff
        finally:
            eng.close()

    def thread_b(barrier):
        eng = native.Engine(0, **cfg)
        try:
            eng.set_weights(pose_w)
            eng.forward_u8(ok_img)
            first = eng.get_maps()
            for i in range(10):
                barrier.wait(timeout=limit)
                for _ in range(2):
                    eng.forward_u8(ok_img)
                    seen_b.append(eng.lib.pmx_last_error().decode())
                got = eng.get_maps()
                seen_b.append(eng.lib.pmx_last_error().decode())
                assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1]), i
        finally:
            eng.close()

    run_threads([thread_a, thread_b], limit)
    assert len(seen_a) == 20 and len(seen_b) == 30
    assert not any('multiples of 8' in m or 'outside 1..' in m for m in seen_b), seen_b


# ---- B4. first use in a fresh process --------------------------------------------------------------------------------------------------
def test_first_gpu_work_of_a_process_in_two_threads(native, refs):
    """tests/threads_child.py: a fresh child process (never an exec) whose first GPU work is a pose thread and a face thread at once"""
    ref, secs = refs
    want = {'pose': CS.digests(ref['pose']), 'face': CS.digests(ref['face'])}
    r = subprocess.run([sys.executable, CHILD], capture_output=True, text=True, timeout=120 + 20 * secs, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert sorted(got) == ['face', 'pose']
    for kind in got:
        bad = [k for k in want[kind] if got[kind].get(k) != want[kind][k]]
        assert sorted(got[kind]) == sorted(want[kind]) and not bad, (kind, bad)
