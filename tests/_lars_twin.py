"""numpy twins of the LARS update (dorknet_amd/optimisers/LARS.py, dk_lars_norms_multi_f32 and
dk_lars_multi_f32) for one tensor.

The definition (You, Gitman, Ginsburg 2017, in the momentum form of the reference's
optimisers/SGDMomentum.py:33-39), with adapt = (the tensor's key is in adapt_params):

    wn = (float) sqrt(sum_i (double) w_i^2);   gn = (float) sqrt(sum_i (double) g_i^2)
    ratio = 1
    if adapt and wn > 0 and gn > 0:  ratio = (trust * wn) / ((gn + wd * wn) + eps)
    g' = g + wd * w                  only if adapt and wd != 0
    step = (-lr) * ratio
    d = step * g' + mom * v;   w = w + d;   v = d

The scalars are formed in Python double.  In the fp32 twin each is rounded to fp32 once
(np.float32(x)) and every operation is one correctly rounded fp32 operation, in the order written;
the fp64 twin is the same expression over float64 values with the double scalars.
"""
import math

import numpy as np

from tests._optim_twin import ieee_host


def norm_f64(a):
    """The l2 norm of one tensor in fp64 (numpy's own summation order)."""
    return math.sqrt(float(np.sum(np.asarray(a, np.float64) ** 2)))


def _ratio(wn, gn, trust, wd, eps, adapt, f):
    if not (adapt and wn > 0 and gn > 0):
        return f(1.0)
    return (f(trust) * wn) / ((gn + f(wd) * wn) + f(eps))


def trust_ratio(wn, gn, trust, wd, eps, adapt=True):
    """stats[4t+2] given the stored fp32 norms stats[4t] and stats[4t+1]; an np.float32."""
    wn, gn = np.float32(wn), np.float32(gn)
    with ieee_host(), np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        r = _ratio(wn, gn, trust, wd, eps, adapt, np.float32)
    assert isinstance(r, np.float32)
    return r


def trust_ratio_f64(wn, gn, trust, wd, eps, adapt=True):
    return _ratio(np.float64(wn), np.float64(gn), trust, wd, eps, adapt, np.float64)


def _update(W, g, v, lr, mom, wd, ratio, adapt, f):
    if adapt and float(wd) != 0.0:
        g = g + f(wd) * W
    step = f(-float(lr)) * f(ratio)
    d = step * g + f(mom) * v
    return W + d, d


def lars_update(W, g, v, lr, mom, wd, ratio, adapt=True):
    """One step for one fp32 tensor given its ratio (the stored fp32 stats[4t+2], or trust_ratio's);
    returns (W, v), both np.float32."""
    for a in (W, g, v):
        assert isinstance(a, np.ndarray) and a.dtype == np.float32, "the fp32 twin takes np.float32 arrays"
    with ieee_host(), np.errstate(over="ignore", under="ignore", invalid="ignore"):
        out = _update(W, g, v, lr, mom, wd, np.float32(ratio), adapt, np.float32)
    assert all(a.dtype == np.float32 for a in out)
    return out


def lars_update_f64(W, g, v, lr, mom, wd, ratio, adapt=True):
    W, g, v = (np.asarray(a, np.float64) for a in (W, g, v))
    return _update(W, g, v, lr, mom, wd, np.float64(ratio), adapt, np.float64)


def lars_step_f64(W, g, v, lr, mom, trust, wd, eps, adapt=True):
    """The whole rule in fp64 for one tensor, norms included: (W, v, ratio)."""
    W, g, v = (np.asarray(a, np.float64) for a in (W, g, v))
    ratio = trust_ratio_f64(norm_f64(W), norm_f64(g), trust, wd, eps, adapt)
    return (*_update(W, g, v, lr, mom, wd, ratio, adapt, np.float64), ratio)
