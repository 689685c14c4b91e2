"""CPU: the f16 mode's emulation helpers (tests/f16_emulation.py) and the detectors' precision= keyword."""
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
