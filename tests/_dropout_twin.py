"""numpy restatement of DropoutLayer's mask rule (TEST INFRASTRUCTURE ONLY); DESIGN.md section 20.

The reference has no dropout; the rule is dorknet_amd's own, pinned so that the kernels
(dorknet_amd/csrc/dropout.hip) can be compared bit for bit:

  * generator: Philox4x32-10 (Salmon et al., Random123): multipliers 0xD2511F53 / 0xCD9E8D57, Weyl
    constants 0x9E3779B9 / 0xBB67AE85, ten rounds;
  * element i = first_index + (linear index in storage order: NHWC bytes, row-major rows) belongs to
    block b = i >> 3; counter = (b & 0xffffffff, b >> 32, step & 0xffffffff, lane), key =
    (seed & 0xffffffff, seed >> 32); with j = i & 7 the element's 16-bit field is output word j >> 1,
    low half for even j, high half for odd j;
  * T = floor(p * 65536); the element is kept iff field >= T; scale = fp32(65536 / (65536 - T));
  * y = keep ? x * scale : +0.0, one fp32 rounding; bf16 storage: the fp32 product rounded to nearest
    even once.  A dropped element is +0.0 whatever x was.
"""
from __future__ import annotations

import numpy as np

from oracle.net import OLayer

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xffffffff)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four, key: two 32-bit words (integers or equal-shaped integer arrays) -> the four
    output words as a uint32 array of shape (4,) + the words' shape."""
    c = [np.asarray(v, dtype=np.uint64) & _MASK for v in counter]
    k = [np.asarray(v, dtype=np.uint64) & _MASK for v in key]
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]  # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ k[0], p1 & _MASK, (p0 >> _S32) ^ c[3] ^ k[1], p0 & _MASK]
        k = [(k[0] + np.uint64(W0)) & _MASK, (k[1] + np.uint64(W1)) & _MASK]
    return np.stack(np.broadcast_arrays(*c)).astype(np.uint32)


def threshold(p):
    """T = floor(p * 65536) for 0 <= p < 1."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError("drop probability {!r} is outside [0, 1)".format(p))
    return int(np.floor(p * 65536.0))


def scale_of(p):
    """fp32(65536 / (65536 - T)): the reciprocal of the keep probability actually realised."""
    return np.float32(65536.0) / np.float32(65536 - threshold(p))


def fields(n, seed, step, lane, first_index=0):
    """The 16-bit field of each of the n elements, as uint32."""
    if first_index < 0 or first_index % 8:
        raise ValueError("first_index must be a non-negative multiple of 8")
    b0 = first_index >> 3
    nb = (first_index + n + 7 >> 3) - b0
    b = np.uint64(b0) + np.arange(nb, dtype=np.uint64)
    w = philox4x32_10((b & _MASK, b >> _S32, step & 0xffffffff, lane), (seed & 0xffffffff, seed >> 32))
    # w[word][block] -> [block][word] -> per block: word 0 low, word 0 high, word 1 low, ...
    w = w.T
    f = np.stack([w & np.uint32(0xffff), w >> np.uint32(16)], axis=-1).reshape(nb * 8)
    return f[:n]


def keep_mask(n, p, seed, step, lane, first_index=0):
    """bool[n]: element k (index first_index + k) is kept."""
    return fields(n, seed, step, lane, first_index) >= np.uint32(threshold(p))


def bf16_round(a):
    """float32 -> the nearest bf16 value (ties to even) as float32; a NaN stays a (quiet) NaN."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7fff) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) << np.uint64(16)
    out = (r & _MASK).astype(np.uint32).view(np.float32)
    return np.where(np.isnan(a), np.float32(np.nan), out).astype(np.float32)


def _apply(x, p, seed, step, lane, first_index, storage):
    """x: float32 values in storage order (any shape; for bf16 storage every value bf16-exact)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    keep = keep_mask(x.size, p, seed, step, lane, first_index).reshape(x.shape)
    with np.errstate(over="ignore", invalid="ignore"):
        prod = x * scale_of(p)  # one fp32 rounding
    if storage == "bf16":
        prod = bf16_round(prod)
    elif storage != "f32":
        raise ValueError(storage)
    return np.where(keep, prod, np.float32(0.0)).astype(np.float32)


def dropout_fwd(x, p, seed, step, lane=0, first_index=0, storage="f32"):
    return _apply(x, p, seed, step, lane, first_index, storage)


def dropout_bwd(dy, p, seed, step, lane=0, first_index=0, storage="f32"):
    return _apply(dy, p, seed, step, lane, first_index, storage)


def storage_mask(shape, p, seed, step, lane=0):
    """The keep mask of a logically NCHW (4-D) or row-major (2-D) array, in its logical shape: a 4-D
    activation is stored NHWC, so the element index runs over [N][H][W][C]."""
    n = int(np.prod(shape))
    keep = keep_mask(n, p, seed, step, lane)
    if len(shape) == 4:
        N, C, H, W = shape
        return np.ascontiguousarray(keep.reshape(N, H, W, C).transpose(0, 3, 1, 2))
    return keep.reshape(shape)


class ODropout(OLayer):
    """The layer on fp64 arrays (NCHW or rows), its mask from keep_mask: `step` counts training
    forwards as DropoutLayer does, the backward uses the step the last training forward recorded.
    The scale is the exact ratio 65536 / (65536 - T)."""

    def __init__(self, name, drop_prob=0.5, seed=0, lane=0, step=0):
        super().__init__(name)
        self.drop_prob, self.seed, self.lane, self.step = float(drop_prob), int(seed), int(lane), int(step)
        self.keep = None

    def forward(self, X, test_mode=False):
        if test_mode:
            return X
        self.keep = storage_mask(X.shape, self.drop_prob, self.seed, self.step, self.lane)
        self.step += 1
        return np.where(self.keep, X * self._scale(X.dtype), np.zeros((), dtype=X.dtype))

    def _scale(self, dtype):
        return np.asarray(65536.0 / (65536 - threshold(self.drop_prob)), dtype=dtype)

    def backward(self, dY):
        return np.where(self.keep, dY * self._scale(dY.dtype), np.zeros((), dtype=dY.dtype))
