"""ReshapeLayer (reference: layers/reshape.py): flatten a feature map into the dense head, and back.

The reference reshapes an NCHW array, so the features of one image are numbered
``f = c * H * W + h * W + w``.  Activations here are NHWC bytes under that logical NCHW shape, so the
flatten is a batched transpose of [HW][C] into [C][HW] per image and its backward the inverse:
dk_flatten_* (dorknet_amd/csrc/reshape.hip), see DESIGN.md section 18.

  * 4-D -> 2-D (flatten): an fp32 or bf16 input gives fp32 rows, as GlobalAveragePoolingLayer hands the
    fp32 head its input; the backward returns an NHWC gradient of the input's storage type.  A
    BatchNorm (+ ReLu) in front of it is applied on load (dk_flatten_fwd_bnx_*, layers/_bn_input.py),
    bit-identical to flattening the materialised BatchNorm output.
  * 2-D -> 4-D (unflatten), fp32: the flatten's backward kernel as a forward, and the reverse.
  * equal shapes: the identity, no launch.
  * 4-D -> 4-D with different shapes, fp32: a flatten launch followed by an unflatten launch.

The reference's class never runs (its constructor calls ``super.__init__``); that bug is not reproduced.
"""
from __future__ import annotations

import torch

from .._hip import lib, stream_handle
from .._tensor import BF16, act_dtype, empty_nhwc, rows, to_nhwc
from ._bn_input import BNOut, lattice_tag, materialize
from .layer import Layer

# per storage type of the NHWC side: the flatten forward (plain, BatchNorm on load) and its backward
_FLATTEN_FWD = {torch.float32: ("dk_flatten_fwd_f32", "dk_flatten_fwd_bnx_f32"),
                BF16: ("dk_flatten_fwd_bf16", "dk_flatten_fwd_bnx_bf16")}
_FLATTEN_BWD = {torch.float32: "dk_flatten_bwd_f32", BF16: "dk_flatten_bwd_bf16"}


def _checked_shape(layer_name, which, shape):
    """`shape` as a tuple of ints: the batch entry -1 or >= 1, every other entry >= 1."""
    try:
        out = tuple(shape)
        ok = len(out) >= 1 and all(not isinstance(v, bool) and int(v) == v for v in out)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("ReshapeLayer({}): {} must be a tuple of integers, got {!r}".format(layer_name, which, shape))
    out = tuple(int(v) for v in out)
    if out[0] != -1 and out[0] < 1:
        raise ValueError("ReshapeLayer({}): the batch entry of {} must be -1 or positive, got {}".format(
            layer_name, which, out))
    if any(v < 1 for v in out[1:]):
        raise ValueError("ReshapeLayer({}): only the batch entry of {} may be -1, every other entry is a positive "
                         "size, got {}".format(layer_name, which, out))
    return out


def _features(shape):
    n = 1
    for v in shape[1:]:
        n *= v
    return n


class ReshapeLayer(Layer):
    """
    Reshapes between the logical NCHW shapes `input_shape` and `output_shape` (reference:
    layers/reshape.py).  The first entry of a shape is the batch and may be -1 (then, and only then, it
    is taken from the tensor); the products of the remaining entries must agree.
    """

    def __init__(self, layer_name, input_shape=None, output_shape=None):
        super().__init__(layer_name)
        self.input_shape = self.output_shape = None
        self._state = None  # a training forward's record: (input shape, input storage type)
        if input_shape is not None or output_shape is not None:
            self._set_shapes(input_shape, output_shape)

    def _set_shapes(self, input_shape, output_shape):
        if input_shape is None or output_shape is None:
            raise ValueError("ReshapeLayer({}): input_shape and output_shape go together, got {!r} and {!r}".format(
                self.layer_name, input_shape, output_shape))
        i = _checked_shape(self.layer_name, "input_shape", input_shape)
        o = _checked_shape(self.layer_name, "output_shape", output_shape)
        if _features(i) != _features(o):
            raise ValueError("ReshapeLayer({}): input_shape {} holds {} features per image, output_shape {} "
                             "{}".format(self.layer_name, i, _features(i), o, _features(o)))
        if i[0] != -1 and o[0] != -1 and i[0] != o[0]:
            raise ValueError("ReshapeLayer({}): input_shape {} and output_shape {} name different batch "
                             "sizes".format(self.layer_name, i, o))
        self.input_shape, self.output_shape = i, o

    def __repr__(self):
        s = "ReshapeLayer(input_shape={}, output_shape={})".format(self.input_shape,
                                                                   self.output_shape)
        return s

    def _form(self):
        if self.input_shape is None:
            return None
        if self.input_shape[1:] == self.output_shape[1:]:
            return "identity"
        return {(4, 2): "flatten", (2, 4): "unflatten", (4, 4): "remap"}.get(
            (len(self.input_shape), len(self.output_shape)))

    @property
    def accepts_bn_input(self):
        """The flatten applies a preceding BatchNorm (+ ReLu) on load (layers/_chain.plan_group)."""
        return self._form() == "flatten"

    def _refuse(self, what):
        raise NotImplementedError("ReshapeLayer({}): {} (input_shape {}, output_shape {})".format(
            self.layer_name, what, self.input_shape, self.output_shape))

    def _check_batch_and_features(self, shape, side):
        want = self.input_shape if side == "input" else self.output_shape
        if _features(tuple(shape)) != _features(want) or len(shape) != len(want):
            raise ValueError("ReshapeLayer({}): {} of shape {} does not match {}_shape {}".format(
                self.layer_name, "an input" if side == "input" else "a gradient", tuple(shape), side, want))
        for s in (self.input_shape, self.output_shape):
            if s[0] != -1 and s[0] != shape[0]:
                raise ValueError("ReshapeLayer({}): a batch of {} where the layer's shapes name {}".format(
                    self.layer_name, shape[0], s[0]))

    # -- the two launches ----------------------------------------------------------------------

    @staticmethod
    def _flatten(x, bn=None):
        """NHWC fp32 / bf16 (N, C, H, W) -> fp32 rows (N, C*H*W) in the reference's feature order."""
        N, C, H, W = x.shape
        y = torch.empty((N, C * H * W), dtype=torch.float32, device=x.device)
        plain, bnx = _FLATTEN_FWD[x.dtype]
        if bn is not None:
            getattr(lib, bnx)(x.data_ptr(), N, H * W, C, *bn.bn_args(), y.data_ptr(), stream_handle())
        else:
            getattr(lib, plain)(x.data_ptr(), N, H * W, C, y.data_ptr(), stream_handle())
        return y

    @staticmethod
    def _unflatten(y, shape, dtype=torch.float32):
        """fp32 rows (N, C*H*W) -> NHWC (N, C, H, W) of `dtype` (bf16: rounded to nearest even)."""
        N, C, H, W = shape
        x = empty_nhwc(N, C, H, W, dtype)
        getattr(lib, _FLATTEN_BWD[dtype])(y.data_ptr(), N, H * W, C, x.data_ptr(), stream_handle())
        return x

    # -- the Layer protocol --------------------------------------------------------------------

    def forward(self, X, test_mode=False):
        self._require_on_gpu()
        form = self._form()
        if form is None:
            self._refuse("no shapes set" if self.input_shape is None else "only 4-D -> 2-D, 2-D -> 4-D, 4-D -> 4-D "
                         "and equal shapes are supported")
        bn = X if isinstance(X, BNOut) and form == "flatten" else None
        if bn is None:
            X = materialize(X)  # a JoinOut, or a BNOut in front of another form
        dtype = act_dtype(bn if bn is not None else X)
        if dtype == BF16 and form != "flatten":
            self._refuse("a bf16 input is taken by the flatten (4-D -> 2-D) only")
        if form == "identity":
            x = y = X
        elif form == "unflatten":
            x = rows(X)
        else:
            x = to_nhwc(bn.x if bn is not None else X)
        self._check_batch_and_features(x.shape, "input")
        out_shape = (x.shape[0],) + self.output_shape[1:]
        if form == "flatten":
            y = self._flatten(x, bn)
        elif form == "unflatten":
            y = self._unflatten(x, out_shape)
        elif form == "remap":
            y = self._unflatten(self._flatten(x), out_shape)
        self._state = None if test_mode else (tuple(x.shape), dtype)
        return y

    def backward(self, upstream_dx):
        self._require_on_gpu()
        if self._state is None:
            raise RuntimeError("ReshapeLayer({}): backward needs a training-mode forward first (a test-mode "
                               "forward records nothing)".format(self.layer_name))
        in_shape, in_dtype = self._state
        form = self._form()
        if lattice_tag(upstream_dx):
            raise ValueError("ReshapeLayer({}): a lattice-form gradient cannot be reshaped".format(self.layer_name))
        # the output of every form is fp32 (the flatten of a bf16 input included)
        if form != "identity" and act_dtype(upstream_dx) != torch.float32:
            raise ValueError("ReshapeLayer({}) backward of mixed storage types: {} output vs {} gradient".format(
                self.layer_name, torch.float32, act_dtype(upstream_dx)))
        if form == "identity" and act_dtype(upstream_dx) != in_dtype:
            raise ValueError("ReshapeLayer({}) backward of mixed storage types: {} input vs {} gradient".format(
                self.layer_name, in_dtype, act_dtype(upstream_dx)))
        want = (in_shape[0],) + self.output_shape[1:]
        if tuple(upstream_dx.shape) != want:
            raise ValueError("ReshapeLayer({}) backward shape mismatch: {} vs {}".format(
                self.layer_name, tuple(upstream_dx.shape), want))
        if form == "identity":
            return upstream_dx
        if form == "flatten":
            return self._unflatten(rows(upstream_dx), in_shape, in_dtype)
        dy = to_nhwc(upstream_dx)
        if form == "unflatten":
            return self._flatten(dy)
        return self._unflatten(self._flatten(dy), in_shape)

    def save_to_h5(self, open_f, save_grads=True):
        """An extension: the reference defines no checkpoint methods for this layer."""
        from ..network.checkpoint import save_layer
        save_layer(self, open_f, save_grads)

    def load_from_h5(self, open_f, load_grads=True):
        from ..network.checkpoint import load_layer
        load_layer(self, open_f, load_grads)
