"""GPU: the stream contract of a context (include/pose_mi355x.h: "calls on a context are stream-ordered and asynchronous unless stated";
pmx_set_stream puts a context on a stream of the caller's).

A1: every call family gives the same bits on a caller's torch stream as on the context's own.  A2: the stream may change between the halves
of a sequence, and travels with Engine.state().  A3: a call is ordered AFTER the caller's producer on that stream with no host
synchronisation in between -- the input buffer holds a decoy, and on the stream a long delay, the copy of the real input and the library
call are enqueued; the results must be those of the real input.  A4: the caller's consumer on that stream is ordered after the call's device
outputs (prefilled with a sentinel).  A5: the control -- the same chain with the context left on its own stream does return the decoy's
canvas, so A3 and A4 can tell.  A6: calls enqueued back to back behind unfinished work, with no host synchronisation between them, are
each drawn from their own tables -- the per-call staging block (csrc/pmx_ctx.h: Staging) is reused by the second call and regrown by the
third while the first is still queued.

The delay is a chain of torch matmuls on the stream, timed with torch events inside every chain: at least 20 x the device time of the call
under test, itself measured on the context's own stream (pmx_timer_*).  An unordered reader therefore certainly arrives first."""
import contextlib
import ctypes as C
import math

import numpy as np
import pytest

import context_scripts as CS
from conftest import pkg

pytestmark = pytest.mark.gpu

FACTOR = 20             # delay >= FACTOR x the call's device time (asserted); the chain asks for twice that
MIN_DELAY_MS = 20.0     # and never less than this: the host needs a moment to enqueue the call behind the delay
SENTINEL = 0xA5


@pytest.fixture(scope='module', autouse=True)
def _torch_runtime_first():
    """torch brings its own HIP runtime; it initialises only while the library's has not opened the device yet in this process (run alone,
    this module would otherwise create its engines first).  With torch first, the library and torch share one runtime, and a torch stream's
    handle is a stream of the library's runtime too."""
    import torch
    torch.cuda.init()


@pytest.fixture(scope='module')
def torch():
    import torch
    torch.cuda.init()
    return torch


class Delay(object):
    """torch work on a stream that takes a known time: n products of two 4096 x 4096 matrices"""

    def __init__(self, torch, S):
        self.torch = torch
        g = torch.Generator(device='cuda').manual_seed(1)
        self.a = torch.randn(4096, 4096, device='cuda', generator=g) / 64
        self.b = torch.randn(4096, 4096, device='cuda', generator=g) / 64
        self.c = torch.empty_like(self.a)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(S):
            self._mm(24)                                     # library start-up and the clock ramp
            e0.record()
            self._mm(8)
            e1.record()
        S.synchronize()
        self.ms_per = e0.elapsed_time(e1) / 8

    def _mm(self, n):
        for _ in range(n):
            self.torch.mm(self.a, self.b, out=self.c)

    def enqueue(self, ms):
        """on torch's current stream"""
        self._mm(max(4, int(math.ceil(ms / self.ms_per))))


@pytest.fixture(scope='module')
def S(torch):
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0               # (torch's default stream has the handle 0, which pmx_set_stream reads as "own stream")
    return s


@pytest.fixture(scope='module')
def delay(torch, S):
    return Delay(torch, S)


@contextlib.contextmanager
def on_stream(eng, stream):
    assert stream.cuda_stream != 0
    eng.set_stream(stream.cuda_stream)
    try:
        yield
    finally:
        eng.set_stream(0)


@pytest.fixture(scope='module')
def pose_w(native):
    return CS.pose_weights(native)


@pytest.fixture(scope='module')
def pose(native, pose_w):
    e = native.Engine(0, **CS.POSE)
    e.set_weights(pose_w)
    yield e
    e.close()


@pytest.fixture(scope='module')
def face(native):
    e = native.Engine(0, **CS.FACE)
    e.set_weights(CS.face_weights())
    yield e
    e.close()


@pytest.fixture(scope='module')
def rend(native):
    e = native.Engine(0, **CS.RENDER)
    yield e
    e.close()


def _equal(got, want, what):
    diff = CS.same(got, want)
    assert diff is None, '%s: %s' % (what, diff)
    for k in want:
        assert np.array_equal(got[k], want[k]), (what, k)


# ---- A1. the same bits on a caller's stream -----------------------------------------------------------------------------------------
def fam_detect_batch(eng):
    """detect_batch from host uint8, batch 2; the records after growth from tiny capacities"""
    eng.set_capacities(peaks_per_joint=2, subsets=2, people=1)
    try:
        eng.detect_batch(CS.u8(101, 2, 64, 96), map_h=64, map_w=96)
        out = CS.records(eng.results())
        assert eng.capacities()['peaks_per_joint'] > 2 and int(out['0.info'][1]) > 0
        out['peaks0'], out['peaks1'] = eng.peaks(0), eng.peaks(1)
        out['paf'], out['heat'] = eng.get_maps()
    finally:
        eng.set_capacities(128, 128, 64)
    return out


def fam_resized(eng):
    """forward_u8_resized to 64 x 96 from two source sizes back to back (the resize tables are rewritten), then the second size again (its
    tables are on the device)"""
    out = {}
    for k, (h, w) in enumerate([(50, 70), (60, 90), (60, 90)]):
        eng.forward_u8_resized(CS.u8(110 + k, 2, h, w), 64, 96)
        out['paf%d' % k], out['heat%d' % k] = eng.get_maps()
        out['resized%d' % k] = eng.get_resized(64, 96)
    return out


def fam_images(eng):
    eng.detect_images([CS.u8(21, 60, 90), CS.u8(22, 96, 128), CS.u8(23, 50, 70)], [(64, 96), (96, 128), (64, 96)], [(60, 90), (96, 128), (50, 70)])
    out = CS.records(eng.results())
    for i in range(3):
        out['paf%d' % i], out['heat%d' % i] = eng.image_maps(i)
    return out


def fam_precise(eng):
    """the begin / add_scale x 4 / finish / postprocess sequence on four lanes, and detect_precise_images on two sizes"""
    CS.precise_sequence(eng, CS.u8(31, 48, 64))
    out = {'seq.' + k: v for k, v in CS.records(eng.results()).items()}
    out['seq.peaks'] = eng.peaks(0)
    eng.detect_precise_images([CS.u8(32, 40, 56), CS.u8(33, 48, 40)], [[(20, 28), (40, 56)], [(24, 20), (48, 40)]])
    out.update({'img.' + k: v for k, v in CS.records(eng.results()).items()})
    for i in range(2):
        out['img.paf%d' % i], out['img.heat%d' % i] = eng.precise_image_maps(i)
    return out


FACE_BOXES6 = [(5, 5, 60, 70, 0, 0), (10, 20, 80, 90, 1, 1), (-10, 40, 50, 120, 0, 0)]


def fam_face(eng):
    """keypoints_boxes with three boxes at max_batch 2 (two chunks), and keypoints_boxes_images over two images"""
    out = CS.face_script(eng)
    out['kp.images'] = eng.keypoints_boxes_images([CS.u8(52, 100, 120), CS.u8(53, 90, 110)], FACE_BOXES6, 0.05)
    return out


def _sample_inputs():
    S = pkg('samples')
    imgs = [CS.u8(71, 24, 40), CS.u8(72, 96, 72)]
    rng = np.random.default_rng(73)
    poses = []
    for n in (2, 1):
        p = np.zeros((n, 18, 3))
        p[:, :, 0], p[:, :, 1] = rng.uniform(2, 62, (n, 18)), rng.uniform(2, 62, (n, 18))
        p[:, :, 2] = rng.integers(0, 3, (n, 18))
        poses.append(p)
    return imgs, [S.SampleRecord.val(im.shape[:2], 64) for im in imgs], poses


def fam_samples(eng):
    imgs, recs, poses = _sample_inputs()
    mask = np.zeros((24, 40), bool)
    mask[3:9, 5:20] = True
    eng.samples_prepare(imgs, [mask, None], recs, 64)
    total, paf, heat = eng.validate_samples(poses)
    got_i, got_m = eng.samples_get()
    assert np.isfinite(total) and got_m.any()
    return dict(total=np.float64(total), paf=paf, heat=heat, imgs=got_i, masks=got_m)


@pytest.mark.parametrize('family', [fam_detect_batch, fam_resized, fam_images, fam_precise], ids=lambda f: f.__name__)
def test_pose_family_same_bits_on_a_callers_stream(pose, S, family):
    want = family(pose)
    with on_stream(pose, S):
        got = family(pose)
    _equal(got, want, family.__name__)
    _equal(family(pose), want, family.__name__ + ' (back on the own stream)')


def test_face_boxes_same_bits_on_a_callers_stream(face, S):
    want = fam_face(face)
    assert np.isfinite(want['face.kp']).all() and want['face.kp'].shape[0] == 3
    with on_stream(face, S):
        got = fam_face(face)
    _equal(got, want, 'face boxes')


def test_render_same_bits_on_a_callers_stream(rend, S):
    want = CS.render_script(rend)
    imgs = CS.render_inputs()[0]
    assert all((want['render.%d' % i] != im).any() for i, im in enumerate(imgs))          # (something was drawn)
    with on_stream(rend, S):
        got = CS.render_script(rend)
    _equal(got, want, 'render')


def test_samples_same_bits_on_a_callers_stream(native, pose_w, S):
    e = native.Engine(0, max_batch=2, max_h=64, max_w=64)
    try:
        e.set_weights(pose_w)
        want = fam_samples(e)
        with on_stream(e, S):
            got = fam_samples(e)
        _equal(got, want, 'samples')
    finally:
        e.close()


def _train_modules():
    import test_gpu_train_step_full as TF
    return TF


def _train_run(native, streams=(), switch=False):
    """The mode-2 training fixture: an f16 forward (the lazy f16 packs exist), forward + backward, a full step; then the weights, the
    maps of the next forward and of an f16 forward -- whose lazy pack builder waits on busy_stream.  streams: () = the own stream; (S,) =
    all on S; (S1, S2) with switch = S1 until backward_trunk, S2 from train_step on."""
    TF = _train_modules()
    e = TF._engine(native)
    try:
        if streams:
            e.set_stream(streams[0].cuda_stream)
        out = {}
        out['f16.paf'], out['f16.heat'] = TF._forward(e, precision=2)
        fb = TF._fb(e)
        out['loss'] = np.concatenate([[fb['total']], fb['paf'], fb['heat']])
        if switch:
            e.set_stream(streams[1].cuda_stream)
        e.train_step()
        for name, (W, b) in e.get_weights().items():
            out['w.' + name], out['b.' + name] = W, b
        out['next.paf'], out['next.heat'] = TF._forward(e)
        out['next16.paf'], out['next16.heat'] = TF._forward(e, precision=2)
        e.set_stream(0)
    finally:
        e.close()
    return out


@pytest.fixture(scope='module')
def train_ref(native):
    ref = _train_run(native)
    start = _train_modules()._weights()
    assert any(not np.array_equal(ref['w.' + nm], start[nm][0]) for nm in start)          # (the step moved the weights)
    assert not np.array_equal(ref['next.paf'], ref['f16.paf'])
    return ref


def test_training_step_same_bits_on_a_callers_stream(native, train_ref, S):
    _equal(_train_run(native, (S,)), train_ref, 'training on a caller\'s stream')


# ---- A2. switching streams between the halves of a sequence ---------------------------------------------------------------------------
def test_forward_and_postprocess_on_different_streams(pose, torch, S):
    imgs = CS.u8(120, 2, 96, 128)
    pose.forward_u8(imgs)
    pose.postprocess(80, 112, img_len=112)
    want = CS.records(pose.results())
    assert int(want['0.info'][1]) > 0
    S2 = torch.cuda.Stream()
    try:
        pose.set_stream(S.cuda_stream)
        pose.forward_u8(imgs)
        pose.set_stream(S2.cuda_stream)
        pose.postprocess(80, 112, img_len=112)
        pose.set_stream(0)
        got = CS.records(pose.results())
    finally:
        pose.set_stream(0)
    _equal(got, want, 'forward on S1, post-process on S2, results on the own stream')


def test_stream_switch_between_backward_and_step(native, train_ref, torch, S):
    S2 = torch.cuda.Stream()
    got = _train_run(native, (S, S2), switch=True)
    _equal(got, train_ref, 'set_stream between backward_trunk and train_step')


# ---- A3 / A4. ordering against the caller's work on the stream, no host synchronisation -----------------------------------------------
class Chain(object):
    """The delay-and-decoy chain of one entry.  bufs: the device buffers the library call reads; real / decoy: host arrays for them."""

    def __init__(self, torch, S, delay, real, decoy):
        self.torch, self.S, self.delay = torch, S, delay
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')
        self.real, self.decoy = [dev(a) for a in real], [dev(a) for a in decoy]
        self.bufs = [torch.empty_like(t) for t in self.real]
        self.call_ms = None
        torch.cuda.synchronize()

    def fill(self, which):
        for b, t in zip(self.bufs, which):
            b.copy_(t)
        self.torch.cuda.synchronize()

    def reference(self, eng, run, read):
        """on the context's own stream, everything synchronised: the results of the real input and of the decoy, and the call's device
        time (the second of two runs: the first pays for tables and lazy packs)"""
        self.fill(self.decoy)
        want_decoy = read(run(self.bufs))
        self.fill(self.real)
        read(run(self.bufs))
        eng.synchronize()
        eng.timer_start()
        out = run(self.bufs)
        self.call_ms = eng.timer_stop()
        want_real = read(out)
        assert CS.same(want_real, want_decoy) is not None, 'the decoy gives the same results as the real input: the check would mean nothing'
        return want_real, want_decoy

    def enqueue(self, run, after=None):
        """decoy in the buffers (complete); then on S: delay, copy of the real input, the call, `after` -- and no synchronisation"""
        torch = self.torch
        self.fill(self.decoy)
        self.ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.S):
            self.ev[0].record()
            self.delay.enqueue(max(2 * FACTOR * self.call_ms, MIN_DELAY_MS))
            self.ev[1].record()
            for b, t in zip(self.bufs, self.real):
                b.copy_(t, non_blocking=True)
            out = run(self.bufs)
            return out if after is None else after(out)

    def check_delay(self, what):
        """after a synchronisation: the delay this chain actually had"""
        self.S.synchronize()
        ms = self.ev[0].elapsed_time(self.ev[1])
        print('%s: call %.3f ms on the own stream, delay %.1f ms on the caller\'s (%.0f x)' % (what, self.call_ms, ms, ms / self.call_ms))
        assert ms >= FACTOR * self.call_ms, (what, ms, self.call_ms)


def _ordered(chain, eng, S, run, read, what):
    want_real, want_decoy = chain.reference(eng, run, read)
    with on_stream(eng, S):
        got = read(chain.enqueue(run))
        chain.check_delay(what)
    assert CS.same(got, want_decoy) is not None, what + ': the call read the DECOY (it ran before the caller\'s copy on the stream)'
    _equal(got, want_real, what)


def _maps(eng):
    paf, heat = eng.get_maps()
    return dict(paf=paf, heat=heat)


def test_forward_u8_device_input_waits_for_the_producer(pose, torch, S, delay):
    chain = Chain(torch, S, delay, [CS.u8(201, 2, 64, 96)], [CS.u8(202, 2, 64, 96)])
    run = lambda bufs: pose.forward_u8(device_ptr=bufs[0].data_ptr(), shape=(2, 64, 96))
    _ordered(chain, pose, S, run, lambda _: _maps(pose), 'forward_u8(device_ptr)')


def _resized_run(eng):
    def run(bufs):
        eng._check(eng.lib.pmx_forward_u8_resized(eng._ctx, C.c_void_p(bufs[0].data_ptr()), 2, 50, 70, 64, 96, 1))
        eng._B, eng._fhw = 2, (8, 12)
    return run


def test_forward_u8_resized_device_input_waits_for_the_producer(pose, torch, S, delay):
    """(the second and later calls with one pair of sizes only enqueue: the resize tables are on the device)"""
    chain = Chain(torch, S, delay, [CS.u8(203, 2, 50, 70)], [CS.u8(204, 2, 50, 70)])
    read = lambda _: dict(_maps(pose), resized=pose.get_resized(64, 96))
    _ordered(chain, pose, S, _resized_run(pose), read, 'forward_u8_resized(on_device)')


def _detect_read(eng):
    def read(_):
        out = CS.records(eng.results())
        out.update(_maps(eng))
        return out
    return read


def test_detect_batch_device_input_and_snapshot_on_the_callers_stream(pose, native, torch, S, delay):
    """A3 for detect_batch(device_ptr), and A4 for results_snapshot: its destination, prefilled with a sentinel, is cloned by the caller on
    the stream right behind the call; the clone holds the records results() returns afterwards."""
    chain = Chain(torch, S, delay, [CS.u8(205, 2, 96, 128)], [CS.u8(206, 2, 96, 128)])
    run = lambda bufs: pose.detect_batch(device_ptr=bufs[0].data_ptr(), shape=(2, 96, 128), map_h=80, map_w=112)
    want_real, want_decoy = chain.reference(pose, run, _detect_read(pose))
    assert int(want_real['0.info'][1]) > 0
    nbytes = 2 * native.result_dtype(pose.capacities()['people']).itemsize
    dst = torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device='cuda:0')

    def after(_):
        pose.results_snapshot(0, dst.data_ptr(), nbytes)
        return dst.clone()

    with on_stream(pose, S):
        clone = chain.enqueue(run, after)
        S.synchronize()                                  # (the caller's stream only; the context is not asked)
        snap = clone.cpu().numpy()
        chain.check_delay('detect_batch(device_ptr) + results_snapshot')
        assert pose.snapshot_wait(0)[3] is False
        res = pose.results()
        got = _detect_read(pose)(None)
    assert not (snap == SENTINEL).all(), 'the caller\'s clone on the stream ran before the snapshot copy: it holds the sentinel'
    assert snap.tobytes() == res.tobytes(), 'the clone of the snapshot differs from results()'
    assert CS.same(got, want_decoy) is not None, 'detect_batch read the DECOY'
    _equal(got, want_real, 'detect_batch(device_ptr)')


def test_forward_u8_images_device_input_waits_for_the_producer(pose, torch, S, delay):
    sizes = [(64, 96), (96, 128), (64, 96)]
    flat = lambda seed: np.concatenate([CS.u8(seed + i, h, w).reshape(-1) for i, (h, w) in enumerate(sizes)])
    hw = np.ascontiguousarray(sizes, dtype=np.int32)
    chain = Chain(torch, S, delay, [flat(210)], [flat(220)])

    def run(bufs):
        pose._check(pose.lib.pmx_forward_u8_images(pose._ctx, C.c_void_p(bufs[0].data_ptr()), hw.ctypes.data_as(C.c_void_p), 3, 1))

    def read(_):
        out = {}
        for i, (h, w) in enumerate(sizes):
            out['paf%d' % i], out['heat%d' % i] = pose.image_maps(i, h // 8, w // 8)
        return out

    _ordered(chain, pose, S, run, read, 'forward_u8_images(on_device)')


def test_samples_prepare_device_input_waits_for_the_producer(native, torch, S, delay):
    imgs, recs, _ = _sample_inputs()
    decoys = [CS.u8(230 + i, *im.shape[:2]) for i, im in enumerate(imgs)]
    chain = Chain(torch, S, delay, imgs, decoys)
    e = native.Engine(0, max_batch=2, max_h=64, max_w=64)

    def run(bufs):
        arr = (native.PmxSample * 2)()
        for s, b, im in zip(arr, bufs, imgs):
            s.bgr, s.src_h, s.src_w = b.data_ptr(), im.shape[0], im.shape[1]
        e._check(e.lib.pmx_samples_prepare(e._ctx, C.cast(arr, C.c_void_p), 2, 64, 1))
        e._samples = (2, 64)

    def read(_):
        got_i, got_m = e.samples_get()
        return dict(imgs=got_i, masks=got_m)

    try:
        _ordered(chain, e, S, run, read, 'samples_prepare(on_device)')
    finally:
        e.close()


def test_keypoints_boxes_images_device_input_waits_for_the_producer(face, torch, S, delay):
    chain = Chain(torch, S, delay, [CS.u8(52, 100, 120), CS.u8(53, 90, 110)], [CS.u8(54, 100, 120), CS.u8(55, 90, 110)])
    run = lambda bufs: face.keypoints_boxes_images(bufs, FACE_BOXES6, 0.05)
    _ordered(chain, face, S, run, lambda kp: dict(kp=kp), 'keypoints_boxes_images(device tensors)')


def _render_chain(torch, S, delay):
    imgs, poses, parts = CS.render_inputs()
    decoys = [CS.u8(240 + i, *im.shape[:2]) for i, im in enumerate(imgs)]
    return Chain(torch, S, delay, imgs, decoys), poses, parts


def _canvases(out):
    return {'canvas%d' % i: t.cpu().numpy() for i, t in enumerate(out)}


def test_render_device_tensors_wait_for_the_producer(rend, torch, S, delay):
    chain, poses, parts = _render_chain(torch, S, delay)
    run = lambda bufs: rend.render(bufs, poses, parts, blend=True)

    def read(out):
        rend.synchronize()
        return _canvases(out)

    _ordered(chain, rend, S, run, read, 'render(device tensors)')


def _render_into(native, eng, bufs, poses, parts, out):
    """pmx_render itself, device images -> the caller's device buffer `out`"""
    p, n_people, part_arr, n_parts, kps = native.render_args(bufs, poses, parts, True)
    arr, on_device, keep = eng._box_images(bufs)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    eng._check(eng.lib.pmx_render(eng._ctx, arr, len(bufs), 1, ptr(p), ptr(n_people), part_arr, n_parts, ptr(kps), 1, C.c_void_p(out.data_ptr()), 1))


def test_render_canvases_are_ready_for_the_callers_consumer(native, rend, torch, S, delay):
    """A4: the device canvases, prefilled with a sentinel, are cloned by the caller on the stream right behind the call; only the caller's
    stream is synchronised."""
    chain, poses, parts = _render_chain(torch, S, delay)
    total = sum(t.numel() for t in chain.real)
    out = torch.full((total,), SENTINEL, dtype=torch.uint8, device='cuda:0')
    flat = lambda d: np.concatenate([d[k].reshape(-1) for k in sorted(d)])
    run = lambda bufs: rend.render(bufs, poses, parts, blend=True)
    want_real, want_decoy = chain.reference(rend, run, lambda o: (rend.synchronize(), _canvases(o))[1])
    want_real, want_decoy = flat(want_real), flat(want_decoy)
    torch.cuda.synchronize()

    def call(bufs):
        _render_into(native, rend, bufs, poses, parts, out)
        return out.clone()

    with on_stream(rend, S):
        clone = chain.enqueue(call)
        S.synchronize()
        got = clone.cpu().numpy()
        chain.check_delay('render into the caller\'s buffer + clone')
    assert not (got == SENTINEL).all(), 'the clone ran before the render: it holds the sentinel'
    assert not np.array_equal(got, want_decoy), 'the render read the DECOY images'
    assert np.array_equal(got, want_real)


# ---- A6. calls back to back behind unfinished work: each is drawn from its own tables ---------------------------------------------------
def _back_to_back(native, torch, S, delay, chain, calls, what):
    """calls: A, B, C, each (engine, chain.bufs) -> the call's device outputs, which live in buffers of the caller's.  A has the larger
    tables; B, smaller and different, reuses the staging block, so only the wait for A's copy keeps A's tables from being rewritten under
    it; C, larger than A, regrows both halves of the block.  The reference of each is the same call alone on a fresh context.  Then ONE
    context, whose block a first A has sized (a growing A would wait for the stream itself), on the caller's stream: the delay, the copy
    of the real inputs, A, B, C -- and one synchronisation of the stream."""
    read = lambda out: {'out%d' % i: t.cpu().numpy() for i, t in enumerate(out)}
    chain.fill(chain.real)
    want = []
    for call in calls:
        e = native.Engine(0, **CS.RENDER)
        try:
            out = call(e, chain.bufs)
            e.synchronize()
            want.append(read(out))
            if call is calls[-1]:                            # the device time of the three calls, on this context's own stream
                e.timer_start()
                for c in calls:
                    c(e, chain.bufs)
                chain.call_ms = e.timer_stop()
        finally:
            e.close()
    flat = [b''.join(w[k].tobytes() for k in sorted(w)) for w in want]
    assert len(set(flat)) == 3, what + ': two of the three calls give the same bytes: the check would mean nothing'
    e = native.Engine(0, **CS.RENDER)
    try:
        calls[0](e, chain.bufs)
        e.synchronize()
        with on_stream(e, S):
            outs = chain.enqueue(lambda bufs: [call(e, bufs) for call in calls])
            chain.check_delay(what)                          # (synchronises the stream: the one synchronisation)
            got = [read(out) for out in outs]
    finally:
        e.close()
    for name, g, w in zip('ABC', got, want):
        _equal(g, w, '%s: call %s' % (what, name))


def _people(seed, n, h, w):
    rng = np.random.default_rng(seed)
    p = np.zeros((n, 18, 3))
    p[:, :, 0], p[:, :, 1] = rng.uniform(-3, w + 3, (n, 18)), rng.uniform(-3, h + 3, (n, 18))
    p[:, :, 2] = np.where(rng.random((n, 18)) < 0.2, 0, 2)
    return p


def test_renders_back_to_back_are_each_drawn_from_their_own_tables(native, torch, S, delay):
    """A: two images of 30 x 40 and 24 x 33 with 12 people; B: the 30 x 40 image with one person; C: three images with 40 people"""
    sizes = [(30, 40), (24, 33), (28, 36)]
    chain = Chain(torch, S, delay, [CS.u8(250 + i, h, w) for i, (h, w) in enumerate(sizes)], [CS.u8(260 + i, h, w) for i, (h, w) in enumerate(sizes)])

    def call(seed, people):
        poses = [_people(seed + i, n, *sizes[i]) for i, n in enumerate(people)]
        return lambda e, bufs: e.render(bufs[:len(people)], poses, blend=True)

    _back_to_back(native, torch, S, delay, chain, [call(270, (7, 5)), call(280, (1,)), call(290, (15, 12, 13))], 'render x 3')


def _polygons(seed, h, w, n):
    """n polygon parts of 3 .. 8 vertices in and around the image, one annotation each: miss, miss, crowd, ..."""
    rng = np.random.default_rng(seed)
    return [(0, i, 2 if i % 3 == 2 else 1, np.round(rng.uniform(-0.2, 1.2, (int(rng.integers(3, 9)), 2)) * [w, h], 1).reshape(-1)) for i in range(n)]


def test_coco_masks_back_to_back_are_each_drawn_from_their_own_tables(native, torch, S, delay):
    """A: two images of 17 x 33 and 40 x 21 with ten polygons and one run-length part; B: a 17 x 33 image with one triangle; C: three
    images with thirty polygons"""
    A = [(17, 33), (40, 21)], [_polygons(300, 17, 33, 6) + [(1, 6, 1, np.array([100, 50, 200, 211], np.uint32))], _polygons(301, 40, 21, 4)]
    B = [(17, 33)], [[(0, 0, 1, [2, 2, 30, 4, 10, 15])]]
    C = [(17, 33), (40, 21), (25, 47)], [_polygons(310, 17, 33, 12), _polygons(311, 40, 21, 9), _polygons(312, 25, 47, 9)]
    nbytes = lambda sizes, parts: sum(t.nbytes for t in native.coco_mask_tables(sizes, parts))
    assert nbytes(*B) + 4 * 64 < nbytes(*A) and nbytes(*A) + 4 * 64 < nbytes(*C)          # (the four tables are padded to 64 bytes each)
    chain = Chain(torch, S, delay, [], [])
    call = lambda sizes, parts: lambda e, _: [m for masks in e.coco_masks(sizes, parts, device=True) for m in masks]
    _back_to_back(native, torch, S, delay, chain, [call(*A), call(*B), call(*C)], 'coco_masks x 3')


# ---- A2 (continued). the stream travels with the state ----------------------------------------------------------------------------------
def test_state_carries_the_stream_into_a_larger_context(native, pose_w, torch, S, delay):
    """Engine.state() / load_state() into a larger context (the path PoseDetector._grow takes): the grown context is on the caller's stream
    without being told, and passes the ordering check there."""
    small = native.Engine(0, max_batch=1, max_h=64, max_w=96)
    big = native.Engine(0, max_batch=2, max_h=64, max_w=96)
    try:
        small.set_weights(pose_w)
        chain = Chain(torch, S, delay, [CS.u8(201, 2, 64, 96)], [CS.u8(202, 2, 64, 96)])
        run = lambda bufs: big.forward_u8(device_ptr=bufs[0].data_ptr(), shape=(2, 64, 96))
        small.set_stream(S.cuda_stream)
        small.copy_state_to(big)
        assert big._stream_ptr == S.cuda_stream
        big.set_stream(0)
        want_real, want_decoy = chain.reference(big, run, lambda _: _maps(big))
        small.copy_state_to(big)                             # the stream comes with the state, not from a set_stream of the test's
        chain.enqueue(run)
        got = _maps(big)
        chain.check_delay('forward_u8(device_ptr) on a context grown from one on the caller\'s stream')
        assert CS.same(got, want_decoy) is not None, 'the grown context read the DECOY: it is not on the stream of the state it loaded'
        _equal(got, want_real, 'grown context')
    finally:
        for e in (small, big):
            e.set_stream(0)
            e.close()


# ---- A5. the control: the method can tell ---------------------------------------------------------------------------------------------
def test_control_a_context_left_on_its_own_stream_reads_the_decoy(native, torch, S, delay):
    """The A3 chain for render with the context NOT on the caller's stream and no synchronisation: the render overtakes the delay and draws
    on the decoy.  Four contexts created one after the other, because streams that share a hardware queue serialise and one context's stream
    may be ordered behind S by accident; at least one of the four must return the decoy's canvases.  (Reading a buffer that is written
    later is harmless.)"""
    chain, poses, parts = _render_chain(torch, S, delay)
    engines = [native.Engine(0, **CS.RENDER) for _ in range(4)]
    try:
        run0 = lambda bufs: engines[0].render(bufs, poses, parts, blend=True)
        want_real, want_decoy = chain.reference(engines[0], run0, lambda o: (engines[0].synchronize(), _canvases(o))[1])
        seen = []
        for k, e in enumerate(engines):
            out = chain.enqueue(lambda bufs: e.render(bufs, poses, parts, blend=True))
            torch.cuda.synchronize()
            got = _canvases(out)
            chain.check_delay('control, context %d' % k)
            seen.append('decoy' if CS.same(got, want_decoy) is None else 'real' if CS.same(got, want_real) is None else 'other')
        print('control: the canvases of the four contexts left on their own streams: %s' % ', '.join(seen))
        assert 'decoy' in seen, 'none of four unordered contexts read the decoy: the delay-and-decoy method cannot tell here (%s)' % seen
    finally:
        for e in engines:
            e.close()
