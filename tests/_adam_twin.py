"""numpy twins of the Adam / AdamW update (dorknet_amd/optimisers/Adam.py, dk_adam_multi_f32) for one
tensor, and of the global-norm clip scale and the in-place scale (optimisers/clip.py).

The definition (torch.optim.Adam / AdamW, non-amsgrad, decoupled decay), with t the 1-based step:

    omb1 = 1 - beta1;  omb2 = 1 - beta2;  neg_step = -(lr / (1 - beta1**t));  sbc2 = sqrt(1 - beta2**t)
    keep = 1 - lr * weight_decay
    g' = s * g                          only with a clip scale s
    w  = keep * w                       only for a decayed tensor and weight_decay != 0
    m  = beta1 * m + omb1 * g';   v = beta2 * v + omb2 * (g' * g')
    den = sqrt(v) / sbc2 + eps;   w = w + neg_step * (m / den)

The scalars are formed in Python double.  In the fp32 twin each is rounded to fp32 once
(np.float32(x)) and every array operation is one correctly rounded fp32 operation, in the order
written; the fp64 twin is the same expression over float64 arrays with the double scalars.
"""
import math

import numpy as np

from tests._optim_twin import ieee_host


def scalars(lr, beta1, beta2, weight_decay, t):
    """(omb1, omb2, neg_step, sbc2, keep) in Python double."""
    lr, beta1, beta2, weight_decay = float(lr), float(beta1), float(beta2), float(weight_decay)
    return 1 - beta1, 1 - beta2, -(lr / (1 - beta1 ** t)), math.sqrt(1 - beta2 ** t), 1 - lr * weight_decay


def _update(W, g, m, v, lr, beta1, beta2, eps, weight_decay, t, decay, scale, f):
    omb1, omb2, neg_step, sbc2, keep = (f(x) for x in scalars(lr, beta1, beta2, weight_decay, t))
    beta1, beta2, eps = f(beta1), f(beta2), f(eps)
    if scale is not None:
        g = f(scale) * g
    if decay and float(weight_decay) != 0.0:
        W = keep * W
    m = beta1 * m + omb1 * g
    v = beta2 * v + omb2 * (g * g)
    den = np.sqrt(v) / sbc2 + eps
    W = W + neg_step * (m / den)
    return W, m, v


def adam_update(W, g, m, v, lr, beta1, beta2, eps, weight_decay, t, decay=True, scale=None):
    """One step for one fp32 tensor; returns (W, m, v), all np.float32.  A square that overflows gives
    v = inf and a step of +-0; numpy's warnings about it are silenced."""
    for a in (W, g, m, v):
        assert isinstance(a, np.ndarray) and a.dtype == np.float32, "the fp32 twin takes np.float32 arrays"
    with ieee_host(), np.errstate(over="ignore", under="ignore", invalid="ignore"):
        out = _update(W, g, m, v, lr, beta1, beta2, eps, weight_decay, t, decay, scale, np.float32)
    assert all(a.dtype == np.float32 for a in out)
    return out


def adam_update_f64(W, g, m, v, lr, beta1, beta2, eps, weight_decay, t, decay=True, scale=None):
    W, g, m, v = (np.asarray(a, np.float64) for a in (W, g, m, v))
    return _update(W, g, m, v, lr, beta1, beta2, eps, weight_decay, t, decay, scale, np.float64)


def clip_scale(norm, max_norm):
    """out[1] of dk_grad_norm_multi_f32 given the stored fp32 norm out[0]: min(1, max_norm / (norm + 1e-6)),
    one fp32 rounding per operation; 1 when max_norm is None, <= 0 or infinite (measure only)."""
    f = np.float32
    if max_norm is None or not math.isfinite(max_norm) or max_norm <= 0:
        return f(1.0)
    with ieee_host(), np.errstate(over="ignore"):
        q = f(max_norm) / (f(norm) + f(1e-6))
    return q if q < f(1.0) else f(1.0)


def norm_f64(arrays):
    """The global l2 norm in fp64 (numpy's own summation order)."""
    return math.sqrt(sum(float(np.sum(np.asarray(a, np.float64) ** 2)) for a in arrays))


def scale_update(g, s):
    """dk_grad_scale_multi_f32 for one tensor: f32(s) * g, one rounding."""
    assert g.dtype == np.float32
    with ieee_host(), np.errstate(over="ignore", under="ignore"):
        return np.float32(s) * g
