"""numpy twins of the reference's SGD, SGD-momentum and RMSProp updates for one tensor, written as the
reference writes them (optimisers/SGD.py:20-24, SGDMomentum.py:33-39, RMSProp.py:28-36): np.float32 arrays meet
Python-float scalars, so every array operation is one correctly rounded fp32 operation and each
scalar is rounded to fp32 once, where it meets the array.  ``1 - decay`` is formed in Python
double; the square is ``g * g`` (np.power(g, 2) is the same product); 1e-5 is a Python float.
The fp64 versions are the same expressions over float64 arrays.

(oracle/ref.py holds the oracle's own sgd_momentum_update, without the gradient scale or the fp32 and
denormal guards; the oracle is frozen, so these live here.)
"""
import contextlib
import ctypes
import ctypes.util

import numpy as np

EPS = 1e-5


def _f32(*arrays):
    for a in arrays:
        assert isinstance(a, np.ndarray) and a.dtype == np.float32, "the fp32 twins take np.float32 arrays"


def host_keeps_denormals():
    a = np.array([1e-20], np.float32)
    return float((a * a)[0]) != 0.0 and float((a * a * np.float32(1e10))[0]) != 0.0


@contextlib.contextmanager
def ieee_host():
    """The calling thread's default floating-point environment for the duration: denormals kept.
    A shared library linked with -ffast-math (oracle/lib/libdorknet_oracle.so is, as the reference's
    setup.py builds its kernels) switches the loading thread to flush-to-zero / denormals-are-zero
    when it is loaded, and numpy then squares 1e-20 to 0 where IEEE fp32 (and the GPU) gives a
    denormal.  fesetenv(FE_DFL_ENV) clears both; the previous environment is put back on exit."""
    if host_keeps_denormals():
        yield
        return
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    saved = ctypes.create_string_buffer(64)  # fenv_t: 32 bytes on x86-64, 8 on aarch64
    libm.fegetenv.argtypes = libm.fesetenv.argtypes = [ctypes.c_void_p]
    libm.fegetenv(saved)
    libm.fesetenv(ctypes.c_void_p(-1))  # FE_DFL_ENV
    try:
        assert host_keeps_denormals(), "the host still flushes denormals: the fp32 twin would not be IEEE"
        yield
    finally:
        libm.fesetenv(saved)


def sgd_update(W, g, lr):
    """SGD.update_weights for one tensor; returns W."""
    _f32(W, g)
    lr = float(lr)
    with ieee_host():
        dx = -lr * g
        return W + dx


def sgd_momentum_update(W, g, v, lr, mom, gscale=1.0):
    """SGDMomentum.update_weights (optimisers/SGDMomentum.py:33-39) for one tensor, after the gradient
    scale of dk_sgd_momentum_multi_f32 (applied unless it is exactly 1); returns (W, v)."""
    _f32(W, g, v)
    lr, mom, gscale = float(lr), float(mom), float(gscale)
    with ieee_host(), np.errstate(under="ignore"):
        if gscale != 1.0:
            g = gscale * g
        dx = -lr * g + mom * v
        return W + dx, dx


def rmsprop_update(W, g, c, lr, decay):
    """RMSProp.update_weights for one tensor; returns (W, c).  A square that overflows fp32 gives
    c = inf and a step of +-0, as in the reference; numpy's warnings about it are silenced."""
    _f32(W, g, c)
    lr, decay = float(lr), float(decay)
    with ieee_host(), np.errstate(over="ignore", under="ignore", invalid="ignore"):
        c = decay * c + (1 - decay) * (g * g)
        dx = -lr * g / np.sqrt(c + EPS)
        return W + dx, c


def sgd_update_f64(W, g, lr):
    W, g = np.asarray(W, np.float64), np.asarray(g, np.float64)
    return W + -float(lr) * g


def rmsprop_update_f64(W, g, c, lr, decay):
    W, g, c = (np.asarray(a, np.float64) for a in (W, g, c))
    lr, decay = float(lr), float(decay)
    c = decay * c + (1 - decay) * (g * g)
    dx = -lr * g / np.sqrt(c + EPS)
    return W + dx, c
