"""CPU: the f16 mode's emulation helpers (tests/f16_emulation.py), the host's f16 rounding (csrc/f16_round.h, through the stand-alone
program tests/f16_round_main.c) and the detectors' precision= keyword."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import f16_emulation as E
from conftest import pkg


def test_round_equals_numpy_float16_in_range():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(100000) * s for s in (1e-6, 1e-3, 1.0, 1e2, 1e4)]).astype(np.float32)
    x = x[np.abs(x) <= E.F16_MAX]
    assert np.array_equal(E.f16_round(x), x.astype(np.float16).astype(np.float32))
    # ties go to even
    assert E.f16_round(np.float32(1 + 2 ** -11)) == np.float32(1.0)
    assert E.f16_round(np.float32(1 + 3 * 2 ** -11)) == np.float32(1 + 2 ** -9)


def test_round_saturates():
    x = np.array([65504, 65519, 65520, 7e4, 1e30, np.inf, -65520, -1e30, -np.inf], np.float32)
    want = np.array([65504] * 6 + [-65504] * 3, np.float32)
    assert np.array_equal(E.f16_round(x), want)
    assert np.isnan(E.f16_round(np.float32(np.nan)))


@pytest.mark.parametrize('ks,pool,relu', [(3, False, True), (7, False, False), (3, True, True)])
def test_emulated_conv_of_representable_operands_is_fp64_conv(ks, pool, relu):
    rng = np.random.default_rng(ks)
    x = E.f16_round(rng.uniform(-2, 2, (2, 20, 12, 14)))
    W = E.f16_round(rng.standard_normal((24, 20, ks, ks)) * 0.1)
    b = rng.uniform(-0.5, 0.5, 24).astype(np.float32)
    got = E.conv_f16(x, W, b, relu=relu, pool=pool)
    with torch.no_grad():
        y = F.conv2d(torch.from_numpy(x).double(), torch.from_numpy(W).double(), padding=ks // 2).float()
        if pool:
            y = F.max_pool2d(y, 2, 2)
        y = y + torch.from_numpy(b).view(1, -1, 1, 1)
        if relu:
            y = F.relu(y)
    assert np.array_equal(got, y.numpy())


def _f16_values():
    """float32 test values around every one of the 65536 f16 bit patterns: the value, its float32 neighbours, the midpoint to the next f16
    value away from zero (65504's: 65520, where the saturation begins) and that midpoint's float32 neighbours; then the saturation
    range and beyond, +-inf, +-0, float32 subnormals and NaNs of both signs, quiet and signalling."""
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    v = bits.view(np.float16).astype(np.float32)
    finite = np.isfinite(v)
    nxt = np.where((bits & 0x7fff) == 0x7bff, np.copysign(np.float32(65536), v), (bits + np.uint16(1)).view(np.float16).astype(np.float32))
    with np.errstate(invalid='ignore', over='ignore'):
        mid = ((v.astype(np.float64) + nxt.astype(np.float64)) / 2).astype(np.float32)
    assert np.array_equal(mid[finite].astype(np.float64) * 2, v[finite].astype(np.float64) + nxt[finite])      # the midpoints are exact
    up, down = np.float32(np.inf), np.float32(-np.inf)
    vals = [v, np.nextafter(v[finite], up), np.nextafter(v[finite], down), mid[finite], np.nextafter(mid[finite], up), np.nextafter(mid[finite], down)]
    edge = np.array([65504, 65505, 65512, 65519, 65519.996, 65520, 65520.004, 65536, 7e4, 1e30, 3.4028235e38, np.inf, 0.0,
                     1e-45, 1e-40, 2.0 ** -26, 2.0 ** -25, 2.0 ** -24, 2.0 ** -14], np.float32)
    vals += [edge, -edge, np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff], np.uint32).view(np.float32)]
    return np.concatenate(vals).astype(np.float32)


def test_host_rounding_equals_numpy_float16_everywhere(tmp_path):
    """f16_rn_sat (the weight packer's rounding, hand-written subnormal and tie branches included) bit for bit against numpy.float16
    conversion after the saturation rule of f16_emulation.f16_round; NaNs compare as NaN.  The program is built with the host compiler
    under the address and undefined-behaviour sanitizers."""
    cc = shutil.which('gcc') or shutil.which('cc')
    assert cc, 'no host C compiler'
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / 'f16_round_main')
    r = subprocess.run([cc, '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                        '-I', pkg('native').CSRC, os.path.join(here, 'f16_round_main.c'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    x = _f16_values()
    r = subprocess.run([exe], input=x.tobytes(), capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.frombuffer(r.stdout, np.uint16)
    assert got.shape == x.shape
    want = E.f16_round(x).astype(np.float16).view(np.uint16)
    nan = np.isnan(x)
    assert nan.sum() >= 2046 + 5 and np.isnan(got[nan].view(np.float16)).all()
    assert np.array_equal(got[~nan], want[~nan]), x[~nan][got[~nan] != want[~nan]][:10]
    # what the values reach: every finite f16 pattern is an answer, and no infinity is
    assert len(np.unique(got[~nan])) == 2 * 0x7c00 and not np.isinf(got.view(np.float16)).any()
    assert 'f16_round.h' in pkg('native').HEADERS


@pytest.mark.parametrize('kind', ['a', 'b', 'c', 'd'])
@pytest.mark.parametrize('ks,cin', [(3, 16), (3, 48), (7, 16), (7, 48)])
def test_emulation_is_exact_on_the_lattice(kind, ks, cin):
    """The premise of the GPU's zero-tolerance lattice tests (f16_emulation.lattice_case): on these operands the float64 sum, a float32
    sum and conv_f16 agree bit for bit, in 'a' .. 'c' every activation / weight of the small side is an f16 subnormal, and in 'b' .. 'd'
    the rounding of the unrounded side is visible."""
    x, W, b = E.lattice_case(kind, ks, cin, seed=ks * 100 + cin)
    xr, Wr = x.astype(np.float16).astype(np.float32), W.astype(np.float16).astype(np.float32)
    outs = []
    for dt in (torch.float64, torch.float32):
        with torch.no_grad():
            y = F.conv2d(torch.from_numpy(xr).to(dt), torch.from_numpy(Wr).to(dt), padding=ks // 2).float() + torch.from_numpy(b).view(1, -1, 1, 1)
        outs.append(y.numpy())
    got = E.conv_f16(x, W, b)
    assert np.array_equal(got, outs[0]) and np.array_equal(got, outs[1]) and np.array_equal(got, E.conv_f16(x, W, b, acc='f32'))
    # the worst case of the derivation: |sum| + |bias| stays below 2^24 units of the grid every product lies on
    unit, worst = (2.0 ** -10, cin * ks * ks * 2 * 2) if kind == 'd' else (2.0 ** -16, cin * ks * ks * 1023 * 4 * 2.0 ** -16)
    assert worst + float(np.abs(b).max()) < unit * 2 ** 24
    assert np.array_equal(got.astype(np.float64) / unit, np.round(got.astype(np.float64) / unit)) and np.abs(got).max() > 0.01
    if kind != 'd':
        small = np.abs(Wr if kind == 'b' else xr)
        assert small.max() < 2.0 ** -14 and (small > 0).mean() > 0.99
    if kind == 'a':
        assert np.array_equal(xr, x) and np.array_equal(Wr, W)
    else:
        raw, rounded = (W, Wr) if kind == 'b' else (x, xr)
        assert (rounded != raw).mean() > (0.99 if kind == 'd' else 0.4) and not np.array_equal(got, E.conv_f16(x, W, b, rounded=False))


def _stub(monkeypatch, PD):
    made = []
    monkeypatch.setattr(PD.PoseDetector, '_make_engine', lambda self, *a: made.append(a))
    return made


def test_pose_detector_accepts_f16(monkeypatch):
    PD = pkg('pose_detector')
    made = _stub(monkeypatch, PD)
    det = PD.PoseDetector(precision='f16')
    assert det._precision == 'f16' and made
    assert pkg('native').PRECISIONS['f16'] == 2


def test_pose_detector_rejects_unknown_precision(monkeypatch):
    PD = pkg('pose_detector')
    _stub(monkeypatch, PD)
    with pytest.raises(ValueError) as e:
        PD.PoseDetector(precision='fp8')
    for p in ('f32', 'f16', 'bf16x3'):
        assert repr(p) in str(e.value)


def test_keypoint_detectors_accept_f16(monkeypatch):
    FH = pkg('face_hand_detector')
    monkeypatch.setattr(FH._KeypointDetector, '_make_engine', lambda self, *a: None)
    for cls in (FH.FaceDetector, FH.HandDetector):
        assert cls(precision='f16')._precision == 'f16'
        with pytest.raises(ValueError):
            cls(precision='fp8')


def test_cli_takes_precision(monkeypatch):
    PD = pkg('pose_detector')
    seen = {}

    class Stop(Exception):
        pass

    def fake(self, *a, **k):
        seen.update(k)
        raise Stop()
    monkeypatch.setattr(PD.PoseDetector, '__init__', fake)
    with pytest.raises(Stop):
        PD.main(['posenet', 'w.npz', '--img', 'x.png', '--precision', 'f16'])
    assert seen['precision'] == 'f16'
