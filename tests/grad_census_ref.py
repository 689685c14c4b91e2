"""NumPy twin of the gradient range census (include/pose_mi355x.h: pmx_backward_g_census; native.Engine.g_census).  Helper of
tests/test_grad_precision_host.py and tests/test_gpu_head_backward_f16.py, not collected itself."""
import numpy as np

from f16_emulation import f16_round

KEYS = ('nonzero', 'flushed', 'subnormal', 'saturated', 'nan')
F16_MIN_NORMAL = 2.0 ** -14
F16_MAX = 65504.0


def classify(g):
    """Boolean arrays by class for float32 g, with r = f16(g) (round to nearest even, saturating): nonzero g != 0 (a NaN is not zero);
    flushed g != 0 and r == 0; subnormal 0 < |r| < 2^-14; saturated |g| > 65504 (infinities included); nan."""
    g = np.asarray(g, dtype=np.float32)
    with np.errstate(invalid='ignore'):
        r = np.abs(f16_round(g))
        nz = g != 0
        return dict(nonzero=nz, flushed=nz & (r == 0), subnormal=(r > 0) & (r < F16_MIN_NORMAL), saturated=np.abs(g) > F16_MAX, nan=np.isnan(g))


def census(g):
    """{class: count} of classify(g), Python ints"""
    return {k: int(v.sum()) for k, v in classify(g).items()}
