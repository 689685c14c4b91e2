"""NumPy twin of the library's Adam contract (include/pose_mi355x.h, "THE CONTRACT"; csrc/pmx_train.hip::adam_one): every line ONE float32
operation rounded to nearest (NumPy's float32 +, -, *, /, sqrt are IEEE operations), plus the float64 evaluation of Chainer's AdamRule
(eta = 1, weight_decay_rate = 0) it restates, and a first-order bound on the difference between the two."""
import math

import numpy as np

F = np.float32
U = 2.0 ** -24          # unit round-off of float32
DEFAULTS = dict(alpha=1e-4, beta1=0.9, beta2=0.999, eps=1e-8)


def alpha_t64(t, alpha=1e-4, beta1=0.9, beta2=0.999):
    """Chainer's AdamRule.lr for eta = 1 at step t (after the increment), in double, in the library's association."""
    return alpha * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)


def alpha_t(t, alpha=1e-4, beta1=0.9, beta2=0.999):
    return F(alpha_t64(t, alpha, beta1, beta2))


def step32(w, m, v, grad, scale, t, alpha=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, a_t=None):
    """The contract on float32 arrays of one layer -> (w, m, v) after step t (a_t: a given float32 alpha_t instead of step t's)."""
    w, m, v, grad = [np.asarray(a, F) for a in (w, m, v, grad)]
    a_t = alpha_t(t, alpha, beta1, beta2) if a_t is None else F(a_t)
    omb1, omb2, eps = F(1.0 - beta1), F(1.0 - beta2), F(eps)
    with np.errstate(under='ignore', over='ignore'):
        g = grad * F(scale)
        d = g - m
        dm = omb1 * d
        m = m + dm
        q = g * g
        e = q - v
        dv = omb2 * e
        v = v + dv
        r = np.sqrt(v)
        s = r + eps
        am = a_t * m
        u = am / s
        w = w - u
    assert w.dtype == m.dtype == v.dtype == F
    return w, m, v


def step64(w, m, v, grad, scale, t, alpha=1e-4, beta1=0.9, beta2=0.999, eps=1e-8):
    """Chainer's formula in float64 (AdamRule.update_core_cpu after GradientScaling): m += (1 - b1)(g - m); v += (1 - b2)(g g - v);
    w -= lr m / (sqrt(v) + eps)."""
    w, m, v, grad = [np.asarray(a, np.float64) for a in (w, m, v, grad)]
    g = grad * float(scale)
    m = m + (1.0 - beta1) * (g - m)
    v = v + (1.0 - beta2) * (g * g - v)
    w = w - alpha_t64(t, alpha, beta1, beta2) * m / (np.sqrt(v) + eps)
    return w, m, v


def bound32(w, m, v, grad, scale, t, alpha=1e-4, beta1=0.9, beta2=0.999, eps=1e-8):
    """|w32 - w64| <= this, element by element, for float32 inputs (exact in both evaluations).  Absolute errors through the thirteen
    roundings of step32 plus the four rounded constants (scale is taken exact only if it is a float32), u = 2^-24, first order in u with
    1.001 for the higher orders; x' are step64's values:
        g   = grad * scale       1 rounding (+ scale's)           E(g)  = 2 u |g|
        d   = g - m              1                                E(d)  = E(g) + u |d|
        dm  = omb1 * d           1 + omb1's rounding              E(dm) = omb1 E(d) + 2 u |dm|
        m'  = m + dm             1                                E(m') = E(dm) + u |m'|
        q   = g * g              1, g twice                       E(q)  = 2 |g| E(g) + u q
        e   = q - v              1                                E(e)  = E(q) + u |e|
        dv  = omb2 * e           1 + omb2's                       E(dv) = omb2 E(e) + 2 u |dv|
        v'  = v + dv             1                                E(v') = E(dv) + u v'
        r   = sqrt(v')           1; |sqrt a - sqrt b| <= |a - b| / sqrt(a)      E(r) = E(v') / sqrt(v') + u r      (0 where v' = 0 = E(v'))
        s   = r + eps            1 + eps's                        E(s)  = E(r) + u eps + u s
        am  = alpha_t * m'       1 + alpha_t's                    E(am) = alpha_t E(m') + 2 u |am|
        x   = am / s             1                                E(x)  = E(am) / s + |am| E(s) / s^2 + u |x|
        w'  = w - x              1                                E(w') = E(x) + u |w'|"""
    w, m, v, grad = [np.asarray(a, np.float64) for a in (w, m, v, grad)]
    a_t, omb1, omb2 = alpha_t64(t, alpha, beta1, beta2), 1.0 - beta1, 1.0 - beta2
    g = grad * float(scale)
    Eg = 2 * U * np.abs(g)
    d = g - m
    Ed = Eg + U * np.abs(d)
    dm = omb1 * d
    Edm = omb1 * Ed + 2 * U * np.abs(dm)
    m1 = m + dm
    Em = Edm + U * np.abs(m1)
    q = g * g
    Eq = 2 * np.abs(g) * Eg + U * q
    e = q - v
    Ee = Eq + U * np.abs(e)
    dv = omb2 * e
    Edv = omb2 * Ee + 2 * U * np.abs(dv)
    v1 = v + dv
    Ev = Edv + U * np.abs(v1)
    r = np.sqrt(v1)
    Er = np.where(v1 > 0, Ev / np.where(v1 > 0, r, 1.0), np.sqrt(Ev)) + U * r
    s = r + eps
    Es = Er + U * eps + U * s
    am = a_t * m1
    Eam = a_t * Em + 2 * U * np.abs(am)
    x = am / s
    Ex = Eam / s + np.abs(am) * Es / (s * s) + U * np.abs(x)
    w1 = w - x
    return 1.001 * (Ex + U * np.abs(w1))
