"""CPU: the host side of the f16 head gradients and the static loss scale -- PoseDetector.set_gradient_precision's argument checks, the
arithmetic of folding 2^-k into a gradient scale, the agreement of header, library and binding on the new entries, and the NumPy twin of
the range census (tests/grad_census_ref.py) at the edges of the f16 range."""
import re

import numpy as np
import pytest

import grad_census_ref as census_ref
from conftest import pkg


def _bare_detector():
    PD = pkg('pose_detector')
    det = PD.PoseDetector.__new__(PD.PoseDetector)          # host helper only; no engine
    det.engine = None
    det._train_on = False
    return det


# ---- 11. argument checking ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scale', [3, 0, 2.0 ** 25, 0.5, -2, 1.5, float('nan'), float('inf'), None, 'two'])
def test_loss_scales_that_are_refused(scale):
    det = _bare_detector()
    with pytest.raises(ValueError) as e:
        det.set_gradient_precision('f16', loss_scale=scale)
    assert 'power of two' in str(e.value)
    assert not hasattr(det, '_loss_scale_log2')          # nothing was stored


@pytest.mark.parametrize('precision', ['bf16x3', 'f64', 2, None, 'F16'])
def test_gradient_precisions_that_are_refused(precision):
    det = _bare_detector()
    with pytest.raises(ValueError) as e:
        det.set_gradient_precision(precision)
    assert "'f32' or 'f16'" in str(e.value)


def test_accepted_settings_are_stored_on_the_detector():
    det = _bare_detector()
    for k in range(25):
        det.set_gradient_precision('f16', loss_scale=2 ** k)
        assert (det._grad_precision, det._loss_scale_log2) == ('f16', k)
    det.set_gradient_precision('f16', loss_scale=1024.0)
    assert det._loss_scale_log2 == 10
    det.set_gradient_precision()
    assert (det._grad_precision, det._loss_scale_log2) == ('f32', 0)


def test_settings_reach_every_engine_and_every_trainable_layer():
    """What _new_engine and _start_training do with the setting, on a recording stand-in for the engine: both options, and the scale of
    every trainable layer times 2^-k -- 82 layers, 92 in mode 2 -- while optimizer_state's '/scale' would stay the user's (_grad_scales)."""
    native = pkg('native')

    class Recorder(object):
        TRUNK_LAYERS = native.Engine.TRUNK_LAYERS

        def __init__(self):
            self.options, self.scales = {}, {}

        def set_option(self, key, value):
            self.options[key] = value

        def head_layers(self):
            return ['conv4_3_CPM', 'conv4_4_CPM'] + ['head%d' % i for i in range(80)]

        def train_set_grad_scale(self, name, scale):
            self.scales[name] = scale

    det = _bare_detector()
    det._grad_scales = {'conv4_3_CPM': 0.25, 'conv4_4_CPM': 0.25}
    for mode2, count in ((False, 82), (True, 92)):
        det.engine, det._mode2, det._train_on = Recorder(), mode2, True
        det.set_gradient_precision('f16', loss_scale=1024)
        assert det.engine.options == {'grad_precision': 2, 'loss_scale_log2': 10}
        assert len(det.engine.scales) == count
        assert det.engine.scales['conv4_3_CPM'] == 0.25 * 2.0 ** -10 and det.engine.scales['head7'] == 2.0 ** -10
        assert det._grad_scales == {'conv4_3_CPM': 0.25, 'conv4_4_CPM': 0.25}
        fresh = Recorder()
        det._apply_gradient_settings(fresh)
        assert fresh.options == {'grad_precision': 2, 'loss_scale_log2': 10}


# ---- 12. the scale-folding arithmetic ---------------------------------------------------------------------------------------------------------
def test_folding_the_loss_scale_into_a_gradient_scale_is_exact():
    """scale * 2^-k in float32, as the library rounds the double it is handed: exact for every k, so (2^k g) * (scale * 2^-k) is g * scale
    with one rounding, the same as without a loss scale."""
    g = np.float32(1.2345678e-5)
    for k in range(25):
        for user in (0.25, 1.0, 0.1):
            folded = np.float32(user * 2.0 ** -k)                       # what pmx_train_set_grad_scale stores
            assert np.float32(0.25) * np.float32(2.0 ** -k) == np.float32(0.25 * 2.0 ** -k)
            assert float(folded) * 2.0 ** k == float(np.float32(user))   # the user's float32 scale, shifted exactly
            assert (g * np.float32(2.0 ** k)) * folded == g * np.float32(user)


# ---- 13. header, library and binding agree ------------------------------------------------------------------------------------------------------
def test_new_entries_in_header_library_and_binding(native):
    lib = native.load()
    syms = native.header_symbols()
    for name in ('pmx_backward_g_census', 'pmx_get_loss_grad_scale', 'pmx_get_transposed_f16_pack'):
        assert name in syms and name in lib._pmx_sig and hasattr(lib, name), name
    assert len(lib._pmx_sig['pmx_backward_g_census'][1]) == 3 and len(lib._pmx_sig['pmx_get_loss_grad_scale'][1]) == 2
    for method in ('g_census', 'loss_grad_scale_log2', 'get_pack', 'set_option'):
        assert callable(getattr(native.Engine, method)), method
    assert native.Engine.PACKS['t_f16'] == 7 and sorted(native.Engine.PACKS.values()) == list(range(8))
    assert native.Engine.CENSUS == census_ref.KEYS
    hdr = re.sub(r'\s+\*\s+', ' ', open(native.HEADER).read())
    for text in ('"loss_scale_log2"', 'pack 7 of the Python binding', 'pmx_backward_head (the values are named like "precision")',
                 'counts[0] = elements with g != 0'):
        assert text in hdr, text
    assert 'pmx_conv2d_backward only' not in hdr
    PD = pkg('pose_detector').PoseDetector
    for method in ('set_gradient_precision', 'gradient_range'):
        assert callable(getattr(PD, method)), method


# ---- 14. the census classifier at the f16 edges --------------------------------------------------------------------------------------------------
def test_census_classifier_at_the_f16_edges():
    f = np.float32
    above = np.nextafter(f(2.0 ** -25), f(1))
    cases = [                      # value -> the classes it belongs to
        (f(2.0 ** -25), {'nonzero', 'flushed'}),                   # the tie between 0 and 2^-24 goes to the even one: zero
        (above, {'nonzero', 'subnormal'}),                         # ... its successor rounds up to 2^-24
        (f(2.0 ** -24), {'nonzero', 'subnormal'}),                 # the smallest f16 subnormal
        (f(2.0 ** -14), {'nonzero'}),                              # the smallest normal
        (f(65504), {'nonzero'}),                                   # the largest finite f16
        (f(65520), {'nonzero', 'saturated'}),
        (f(np.inf), {'nonzero', 'saturated'}),
        (f(np.nan), {'nonzero', 'nan'}),
        (f(0), set()), (f(-0.0), set()),
        (f(1023 * 2.0 ** -24), {'nonzero', 'subnormal'}),          # the largest subnormal
        (np.nextafter(f(2.0 ** -14), f(0)), {'nonzero'}),          # just below the smallest normal: rounds up to it
    ]
    for v, want in cases:
        for sign in (1, -1):
            got = {k for k, m in census_ref.classify(np.array([sign * v], np.float32)).items() if m[0]}
            assert got == want, (float(v), sign, got, want)
    arr = np.array([v for v, _ in cases] + [-v for v, _ in cases], np.float32)
    counts = census_ref.census(arr)
    assert counts == {k: 2 * sum(k in want for _, want in cases) for k in census_ref.KEYS}
