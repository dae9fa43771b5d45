"""DropoutLayer: an extension, the reference has no dropout.

The keep bit of an element is a pure function of (seed, step, lane, element index) -- Philox4x32-10
over blocks of eight elements, DESIGN.md section 20 -- so no mask is stored: the backward regenerates
it (dk_dropout_*, dorknet_amd/csrc/dropout.hip), the layer costs one read and one write per pass, and
a run resumed from a checkpoint (``drop_prob``, ``seed`` and ``step`` are saved) draws the masks the
original run would have drawn.  The element index is the linear index in storage order: NHWC bytes for
a 4-D activation, row-major for 2-D rows.

  * ``step`` counts training forwards; a training forward uses the current step, records it for the
    backward and adds one.  ``lane`` tells data-parallel ranks apart (parallel.DataParallel sets it to
    the rank): one seed, different masks.
  * T = floor(drop_prob * 65536); an element is kept iff its 16-bit field >= T and is then scaled by
    fp32(65536 / (65536 - T)), the reciprocal of the keep probability actually realised.
  * fp32 rows, fp32 or bf16 maps; the output has the input's shape and storage type.  A BatchNorm
    (+ ReLu) in front of the layer is applied on load (dk_dropout_fwd_bnx_*, layers/_bn_input.py),
    bit-identical to dropping the materialised BatchNorm output.
  * a test-mode forward is the identity: no launch, nothing recorded, ``step`` unchanged.
"""
from __future__ import annotations

import math
import numbers

import torch

from .._hip import lib, stream_handle
from .._tensor import BF16, act_dtype, empty_nhwc, rows, to_nhwc
from ._bn_input import BNOut, JoinOut, lattice_tag
from .layer import Layer

# per storage type: the forward (plain, BatchNorm on load) and the backward
_DROPOUT_FWD = {torch.float32: ("dk_dropout_fwd_f32", "dk_dropout_fwd_bnx_f32"),
                BF16: ("dk_dropout_fwd_bf16", "dk_dropout_fwd_bnx_bf16")}
_DROPOUT_BWD = {torch.float32: "dk_dropout_bwd_f32", BF16: "dk_dropout_bwd_bf16"}

MAX_COUNT = 2 ** 63 - 1  # seed and step travel as long long


def checked_prob(layer_name, p):
    """`p` as a float in [0, 1)."""
    if isinstance(p, bool) or not isinstance(p, numbers.Real):
        raise TypeError("DropoutLayer({}): drop_prob must be a number, got {!r}".format(layer_name, p))
    p = float(p)
    if not 0.0 <= p < 1.0:  # (a NaN fails both comparisons)
        raise ValueError("DropoutLayer({}): drop_prob must lie in [0, 1), got {!r}".format(layer_name, p))
    return p


def checked_count(layer_name, which, v):
    """`v` (seed, step) as an int in 0 .. 2**63 - 1."""
    if isinstance(v, bool) or not isinstance(v, numbers.Integral):
        raise TypeError("DropoutLayer({}): {} must be an integer, got {!r}".format(layer_name, which, v))
    v = int(v)
    if not 0 <= v <= MAX_COUNT:
        raise ValueError("DropoutLayer({}): {} must lie in 0 .. 2**63 - 1, got {}".format(layer_name, which, v))
    return v


class DropoutLayer(Layer):
    """
    Zeroes each element with probability `drop_prob` in training and scales the kept ones by the
    reciprocal of the keep probability; the identity in test mode.
    """
    accepts_bn_input = True

    def __init__(self, layer_name, drop_prob=0.5, seed=0):
        super().__init__(layer_name)
        self.drop_prob = checked_prob(layer_name, drop_prob)
        self.seed = checked_count(layer_name, "seed", seed)
        self.step = 0   # training forwards so far
        self.lane = 0   # the data-parallel rank
        self._state = None  # a training forward's record: (threshold, step, lane, shape, storage type)

    def __repr__(self):
        return "DropoutLayer({}, drop_prob={})".format(self.layer_name, self.drop_prob)

    @property
    def threshold(self):
        """T = floor(drop_prob * 65536), in 0..65535."""
        return int(math.floor(self.drop_prob * 65536.0))

    def forward(self, X, test_mode=False):
        if test_mode:
            return X
        self._require_on_gpu()
        if isinstance(X, JoinOut):
            X = X.materialize()
        bn = X if isinstance(X, BNOut) else None
        x = bn.x if bn is not None else X
        dtype = act_dtype(x)
        if len(x.shape) == 4:
            x = to_nhwc(x)
            y = empty_nhwc(*x.shape, dtype=x.dtype)
        elif len(x.shape) == 2:
            if dtype == BF16:
                raise ValueError("DropoutLayer({}): bf16 storage is taken for 4-D maps only".format(self.layer_name))
            x = rows(x)
            y = torch.empty_like(x)
        else:
            raise ValueError("DropoutLayer({}): expected 2-D rows or a 4-D map, got shape {}".format(
                self.layer_name, tuple(x.shape)))
        step = checked_count(self.layer_name, "step", self.step)
        plain, bnx = _DROPOUT_FWD[x.dtype]
        T = self.threshold
        args = (x.data_ptr(), x.numel(), T, self.seed, step, self.lane, 0)
        if bn is not None:
            getattr(lib, bnx)(*args, x.shape[1], *bn.bn_args(), y.data_ptr(), stream_handle())
        else:
            getattr(lib, plain)(*args, y.data_ptr(), stream_handle())
        self._state = (T, step, self.lane, tuple(x.shape), x.dtype)
        self.step = step + 1
        return y

    def backward(self, upstream_dx):
        self._require_on_gpu()
        if self._state is None:
            raise RuntimeError("DropoutLayer({}): backward needs a training-mode forward first (a test-mode "
                               "forward records nothing)".format(self.layer_name))
        T, step, lane, shape, dtype = self._state
        if lattice_tag(upstream_dx):
            raise ValueError("DropoutLayer({}): a lattice-form gradient cannot be masked".format(self.layer_name))
        if act_dtype(upstream_dx) != dtype:
            raise ValueError("DropoutLayer({}) backward of mixed storage types: {} input vs {} gradient".format(
                self.layer_name, dtype, act_dtype(upstream_dx)))
        if tuple(upstream_dx.shape) != shape:
            raise ValueError("DropoutLayer({}) backward shape mismatch: {} vs {}".format(
                self.layer_name, tuple(upstream_dx.shape), shape))
        if len(shape) == 4:
            dy = to_nhwc(upstream_dx)
            dx = empty_nhwc(*shape, dtype=dtype)
        else:
            dy = rows(upstream_dx)
            dx = torch.empty_like(dy)
        getattr(lib, _DROPOUT_BWD[dtype])(dy.data_ptr(), dy.numel(), T, self.seed, step, lane, 0,
                                          dx.data_ptr(), stream_handle())
        return dx

    def save_to_h5(self, open_f, save_grads=True):
        from ..network.checkpoint import save_layer
        save_layer(self, open_f, save_grads)

    def load_from_h5(self, open_f, load_grads=True):
        from ..network.checkpoint import load_layer
        load_layer(self, open_f, load_grads)
