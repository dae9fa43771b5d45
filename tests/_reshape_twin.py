"""numpy restatement of ReshapeLayer's rules (TEST INFRASTRUCTURE ONLY).

Reference: layers/reshape.py:15-21 -- ``X.reshape(output_shape)`` on an NCHW array, so the features of
one image are numbered f = c * H * W + h * W + w.  Arrays are NCHW; a copy is exact, so the dtype is
kept and every comparison against the kernels is bitwise.
"""
from __future__ import annotations

import numpy as np

from oracle.net import OLayer


def flatten(X):
    """X[N][C][H][W] -> [N][C*H*W]."""
    X = np.asarray(X)
    return np.ascontiguousarray(X).reshape(X.shape[0], -1)


def unflatten(Y, shape):
    """Y[N][C*H*W] -> [N][C][H][W], `shape` = (N or -1, C, H, W): the inverse of flatten."""
    Y = np.asarray(Y)
    return np.ascontiguousarray(Y).reshape((Y.shape[0],) + tuple(shape[1:]))


class OReshape(OLayer):
    """ReshapeLayer for oracle.net networks: any pair of shapes with equal feature counts."""

    def __init__(self, name, input_shape, output_shape):
        super().__init__(name)
        self.input_shape, self.output_shape = tuple(input_shape), tuple(output_shape)

    def forward(self, X, test_mode=False):
        self.in_shape = X.shape
        return np.ascontiguousarray(X).reshape((X.shape[0],) + self.output_shape[1:])

    def backward(self, dY):
        return np.ascontiguousarray(dY).reshape(self.in_shape)
