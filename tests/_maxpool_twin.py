"""numpy restatement of MaxPoolLayer's rules (TEST INFRASTRUCTURE ONLY).

Reference: layers/pooling.py:45-77, layers/pooling_cy.pyx:8-88 (pool_train / pool_backward), with
what the reference leaves undefined pinned as dorknet_amd pins it:

  * window stride x stride, non-overlapping; OH = H // stride, OW = W // stride; the trailing
    H % stride rows and W % stride columns are not pooled and get a zero gradient;
  * the window is scanned row-major from (0, 0) with a strict >: the first maximum wins;
  * the location is kept as idx = m * stride + n, one uint8 per output element;
  * dX = dY at the recorded location and 0 at every other input position.

Arrays are NCHW.  Max and copy are exact, so the dtype of X / dY is kept and every comparison
against the kernels is bitwise.
"""
from __future__ import annotations

import numpy as np

from oracle.net import OLayer


def windows(X, s):
    """X[N][C][H][W] -> [N][C][OH][OW][s*s], window elements in scan order (k = m * s + n)."""
    N, C, H, W = X.shape
    OH, OW = H // s, W // s
    if OH < 1 or OW < 1:
        raise ValueError("a {}x{} input has no {}x{} window".format(H, W, s, s))
    v = X[:, :, :OH * s, :OW * s].reshape(N, C, OH, s, OW, s)
    return np.ascontiguousarray(v.transpose(0, 1, 2, 4, 3, 5)).reshape(N, C, OH, OW, s * s)


def pool_fwd(X, s):
    """(Y, idx): the scan of pool_train, element by element with a strict >."""
    v = windows(np.asarray(X), s)
    best = v[..., 0].copy()
    idx = np.zeros(best.shape, dtype=np.uint8)
    for k in range(1, s * s):
        better = v[..., k] > best
        best = np.where(better, v[..., k], best)
        idx = np.where(better, np.uint8(k), idx)
    return best, idx.astype(np.uint8)


def take(X, idx, s):
    """The window element at each recorded location."""
    v = windows(np.asarray(X), s)
    return np.take_along_axis(v, idx[..., None].astype(np.int64), axis=-1)[..., 0]


def pool_bwd(idx, dY, s, H, W):
    dY = np.asarray(dY)
    N, C, OH, OW = dY.shape
    dX = np.zeros((N, C, H, W), dtype=dY.dtype)
    for k in range(s * s):
        m, n = divmod(k, s)
        dX[:, :, m:OH * s:s, n:OW * s:s] = np.where(idx == k, dY, np.zeros((), dtype=dY.dtype))
    return dX


class OMaxPool(OLayer):
    """`replay`: a uint8 location array (the GPU layer's max_locs) that the next training forward
    takes instead of its own arg-max, as OReLU.replay does for ReLU decisions: an fp32 tie inside
    a window may resolve to another element than in fp64.  The forward keeps its own arg-max in
    `own_idx` and the input in `X` for the tie analysis."""
    replay = None

    def __init__(self, name, stride=2):
        super().__init__(name)
        self.stride = int(stride)

    def forward(self, X, test_mode=False):
        Y, own = pool_fwd(X, self.stride)
        if test_mode:
            return Y
        idx = own
        if self.replay is not None:
            idx = np.asarray(self.replay, dtype=np.uint8)
            if idx.shape != own.shape:
                raise ValueError("replayed locations shape {} != output {}".format(idx.shape, own.shape))
            self.replay = None
            Y = take(X, idx, self.stride)
        self.X, self.own_idx, self.idx = X, own, idx
        return Y

    def backward(self, dY):
        return pool_bwd(self.idx, dY, self.stride, *self.X.shape[-2:])
