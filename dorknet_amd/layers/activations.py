"""ReLU (reference: layers/activations.py), and four activations the reference lacks: LeakyReLu,
ReLu6, HardSwish and SiLu (below ReLu).

``out = max(0, X)``; the backward mask is ``out > 0`` (gradient 0 at 0, :41).  The mask
is kept as uint8 (the reference stores an fp32 copy, :42); ``positive_locs`` still
returns the fp32 mask on request.  When the layer directly follows a BatchNormLayer in a
network or residual chain, the two run fused (BatchNormLayer.forward_bn_relu) and this
layer only records its output.
"""
from __future__ import annotations

import math
import numbers

import torch

from .._hip import lib, stream_handle
from .._tensor import BF16, act_dtype, as_device, empty_nhwc, is_nhwc as is_nhwc_t, rows, to_nhwc
from ._bn_input import BNOut, JoinOut, Partials, lattice_tag
from .layer import Layer


def _same_layout(X):
    X = as_device(X, act_dtype(X))
    return to_nhwc(X) if X.dim() == 4 else rows(X)


def _bf16(*ts):
    """Whether the operands are bf16 storage (the _bf16 entries); mixed storage types are refused."""
    if len({t.dtype for t in ts}) != 1:
        raise ValueError("operands of mixed storage types: {}".format(", ".join(str(t.dtype) for t in ts)))
    return ts[0].dtype == torch.bfloat16


class ReLu(Layer):

    def __init__(self, layer_name):
        super().__init__(layer_name)
        self._mask = None
        self._fused_out = None
        self._join_bn = None
        self._join_done = False
        self._join_y_ptr = None  # data_ptr of the fused join's output (_bn_add)
        self._join_y = None      # that output, when the join left no mask (JoinOut without one)

    def join_backward_done(self):
        """The consumer of this residual join's output applied this ReLU's backward (and stage 1
        of the join BatchNorm's) in its own dgrad epilogue (DepthwiseConvLayer, accepts_join):
        the gradient it returned is already dx, so backward() passes it through."""
        self._join_done = True

    def __repr__(self):
        return "ReLu({})".format(self.layer_name)

    def _empty_like(self, x):
        return empty_nhwc(*x.shape, dtype=x.dtype) if x.dim() == 4 else torch.empty_like(x)

    def forward(self, X, test_mode=False):
        self._require_on_gpu()
        st = stream_handle()
        x = _same_layout(X)
        y = self._empty_like(x)
        mask = None
        if not test_mode:
            mask = torch.empty(x.shape, dtype=torch.uint8, device=x.device,
                               memory_format=torch.channels_last if x.dim() == 4 else torch.contiguous_format)
        fwd = lib.dk_relu_fwd_bf16 if x.dtype == torch.bfloat16 else lib.dk_relu_fwd_f32
        fwd(x.data_ptr(), x.numel(), y.data_ptr(), 0 if mask is None else mask.data_ptr(), st)
        if not test_mode:
            self._mask, self._fused_out, self._join_bn = mask, None, None
            self._join_done = False
            self._join_y = None
        return y

    def forward_add(self, A, B, test_mode=False, defer=False, need_mask=True):
        """ReLU(A + B) in one pass -- the residual join (residual_block.py:75).  A and/or B may
        be a BatchNorm output not yet written (BNOut): the normalisation is applied on load.
        defer: the consumer of the result can form it on load (ResidualBlock.takes_join_input):
        return a JoinOut (layers/_bn_input.py) instead of running the join pass."""
        self._require_on_gpu()
        if act_dtype(A) != act_dtype(B):
            raise ValueError("residual join of mixed storage types: {} vs {}".format(act_dtype(A), act_dtype(B)))
        st = stream_handle()
        if isinstance(A, JoinOut):
            A = A.materialize()
        if isinstance(B, JoinOut):
            B = B.materialize()
        if defer and (isinstance(A, BNOut) or isinstance(B, BNOut)) and self._join_parts_ok(A, B):
            return JoinOut(A, B, self, test_mode, need_mask)
        if isinstance(A, BNOut) or isinstance(B, BNOut):
            y = self._bn_add(A, B, test_mode, st)
            if y is not None:
                return y
        a, b = _same_layout(A), _same_layout(B)
        if a.shape != b.shape:
            raise ValueError("residual join shape mismatch: {} vs {}".format(tuple(a.shape), tuple(b.shape)))
        add = lib.dk_add_bf16 if _bf16(a, b) else lib.dk_add_f32
        y = self._empty_like(a)
        mask = None
        if not test_mode:
            mask = torch.empty(a.shape, dtype=torch.uint8, device=a.device,
                               memory_format=torch.channels_last if a.dim() == 4 else torch.contiguous_format)
        add(a.data_ptr(), b.data_ptr(), a.numel(), 1, y.data_ptr(), 0 if mask is None else mask.data_ptr(), st)
        if not test_mode:
            self._mask, self._fused_out, self._join_bn = mask, None, None
            self._join_y = None
        return y

    @staticmethod
    def _join_parts_ok(A, B):
        if A.dim() != 4 or tuple(A.shape) != tuple(B.shape) or A.shape[1] % 4 or A.dtype != torch.float32:
            return False
        xs = [T.x if isinstance(T, BNOut) else T for T in (A, B)]
        return all(isinstance(x, torch.Tensor) and x.dtype == torch.float32 and is_nhwc_t(x) for x in xs)

    def _join_written(self, jo):
        """The join output of a JoinOut was written (by its consumer, or by its materialize):
        the backward state the join pass leaves (_bn_add)."""
        if not jo.test_mode:
            self._mask, self._fused_out = jo.mask, None
            self._join_bn = jo.A if isinstance(jo.A, BNOut) else None
            self._join_done = False
            self._join_y_ptr = None if jo.y is None else jo.y.data_ptr()  # (None: pooled, mark_pooled)
            self._join_y = jo.y if jo.mask is None else None

    def _bn_add(self, A, B, test_mode, st):
        def parts(T):
            if isinstance(T, BNOut):
                return T.x, T.bn_args()
            return to_nhwc(T), (0, 0, 0, 0, 0)
        if A.dim() != 4 or tuple(A.shape) != tuple(B.shape) or A.shape[1] % 4:
            return None
        (a, pa), (b, pb) = parts(A), parts(B)
        if not (is_nhwc_t(a) and is_nhwc_t(b)):
            return None
        bn_add = lib.dk_bn_add_bf16 if _bf16(a, b) else lib.dk_bn_add_f32
        y = empty_nhwc(*a.shape, dtype=a.dtype)
        mask = None
        if not test_mode:
            mask = torch.empty(a.shape, dtype=torch.uint8, device=a.device, memory_format=torch.channels_last)
        bn_add(a.data_ptr(), *pa, b.data_ptr(), *pb, a.numel(), a.shape[1], 1, y.data_ptr(),
               0 if mask is None else mask.data_ptr(), st)
        if not test_mode:
            self._mask, self._fused_out = mask, None
            self._join_bn = A if isinstance(A, BNOut) else None
            self._join_done = False
            self._join_y_ptr = y.data_ptr()  # a consumer holding y itself may take the mask as y > 0
            self._join_y = None
        return y

    def _attach_fused(self, y, test_mode):
        if not test_mode:
            self._mask, self._fused_out, self._join_bn = None, y, None
            self._join_y = None

    def _mask_from_join(self):
        """The join's ReLU mask from its stored output (y > 0), for a backward that needs the mask
        when the join left none (a JoinOut whose consumer takes it as y > 0)."""
        y = self._join_y
        mask = torch.empty(y.shape, dtype=torch.uint8, device=y.device, memory_format=torch.channels_last)
        fwd = lib.dk_relu_fwd_bf16 if y.dtype == torch.bfloat16 else lib.dk_relu_fwd_f32
        fwd(y.data_ptr(), y.numel(), 0, mask.data_ptr(), stream_handle())  # mask-only pass
        self._mask, self._join_y = mask, None
        return mask

    @property
    def positive_locs(self):
        """fp32 mask (out > 0), as the reference's attribute (activations.py:42)."""
        if self._mask is None and self._join_y is not None:
            self._mask_from_join()
        if self._mask is not None:
            out = torch.empty(self._mask.shape, dtype=torch.float32, device=self._mask.device,
                              memory_format=torch.channels_last if self._mask.dim() == 4 else torch.contiguous_format)
            lib.dk_mask_to_f32(self._mask.data_ptr(), self._mask.numel(), out.data_ptr(), stream_handle())
            return out
        if self._fused_out is not None:
            y = as_device(self._fused_out)  # a BNOut is materialised here
            mask = torch.empty(y.shape, dtype=torch.uint8, device=y.device,
                               memory_format=torch.channels_last if y.dim() == 4 else torch.contiguous_format)
            fwd = lib.dk_relu_fwd_bf16 if y.dtype == torch.bfloat16 else lib.dk_relu_fwd_f32
            fwd(y.data_ptr(), y.numel(), 0, mask.data_ptr(), stream_handle())  # mask-only pass
            out = torch.empty(y.shape, dtype=torch.float32, device=y.device,
                              memory_format=torch.channels_last if y.dim() == 4 else torch.contiguous_format)
            lib.dk_mask_to_f32(mask.data_ptr(), mask.numel(), out.data_ptr(), stream_handle())
            return out
        return None

    def backward(self, upstream_dx):
        self._require_on_gpu()
        if self._join_done:
            self._join_done = False
            return upstream_dx
        if self._mask is None and self._join_y is not None:
            self._mask_from_join()
        if self._mask is None:
            raise RuntimeError("ReLu {}: backward without a training-mode forward (or the layer ran fused with "
                               "the preceding BatchNormLayer; its backward is BatchNormLayer.backward_bn_relu)"
                               .format(self.layer_name))
        dy = _same_layout(upstream_dx)
        dx = self._empty_like(dy)
        bn = getattr(self, "_join_bn", None)
        if bn is not None and tuple(bn.x.shape) == tuple(dy.shape) and is_nhwc_t(dy):
            # the join's BN input: its backward stage 1 rides on this pass (residual_block.py:85-86)
            C = dy.shape[1]
            P = dy.numel() // C
            nb = lib.dk_bn_workspace_bytes(P, C)
            part = Partials(bn, lib.dk_bn_partial_blocks(P, C), C, dy.device)
            bwd = lib.dk_relu_bwd_bn_partial_bf16 if _bf16(dy, bn.x) else lib.dk_relu_bwd_bn_partial_f64
            r = bwd(dy.data_ptr(), self._mask.data_ptr(), bn.x.data_ptr(), P, C, *bn.bn_args(), dx.data_ptr(),
                    part.ptr, nb, stream_handle())
            part.hand(dx, r)
            return dx
        bwd = lib.dk_relu_bwd_bf16 if dy.dtype == torch.bfloat16 else lib.dk_relu_bwd_f32
        bwd(dy.data_ptr(), self._mask.data_ptr(), dy.numel(), dx.data_ptr(), stream_handle())
        return dx

    def save_to_h5(self, open_f, save_grads=True):
        from ..network.checkpoint import save_layer
        save_layer(self, open_f, save_grads)

    def load_from_h5(self, open_f, load_grads=True):
        pass


# ---------------------------------------------------------------------------------------------
# Activations beyond ReLU: extensions, the reference has only ReLu.  dk_act_* (dorknet_amd/csrc/
# act_math.h, activations.hip, batchnorm.hip), DESIGN.md section 23.
# ---------------------------------------------------------------------------------------------

# the `kind` argument of the dk_act_* entries
ACT_LEAKY, ACT_RELU6, ACT_HARDSWISH, ACT_SILU = 0, 1, 2, 3

# per storage type: the forward (plain, BatchNorm on load) and the backward (plain, with stage 1 of the
# BatchNorm's backward)
_ACT_FWD = {torch.float32: ("dk_act_fwd_f32", "dk_act_fwd_bnx_f32"), BF16: ("dk_act_fwd_bf16", "dk_act_fwd_bnx_bf16")}
_ACT_BWD = {torch.float32: ("dk_act_bwd_f32", "dk_act_bwd_bnx_f32"), BF16: ("dk_act_bwd_bf16", "dk_act_bwd_bnx_bf16")}


_F32_MAX = 3.4028234663852886e38  # alpha travels as a C float


def checked_alpha(layer_name, alpha):
    """`alpha` (LeakyReLu's slope for v <= 0) as a finite float."""
    if isinstance(alpha, bool) or not isinstance(alpha, numbers.Real):
        raise TypeError("LeakyReLu({}): alpha must be a number, got {!r}".format(layer_name, alpha))
    alpha = float(alpha)
    if not math.isfinite(alpha) or abs(alpha) > _F32_MAX:  # (a NaN fails isfinite)
        raise ValueError("LeakyReLu({}): alpha must be a finite fp32 value, got {!r}".format(layer_name, alpha))
    return alpha


class _Activation(Layer):
    """An elementwise activation y = act(v) whose backward recomputes act'(v) from the layer's input:
    no mask and no copy are stored, a training forward keeps only a reference to its input -- the
    tensor, or the BNOut of a BatchNormLayer [+ ReLu] in front (applied on load, layers/_bn_input.py).
    After a BNOut forward the backward also writes stage 1 of that BatchNorm's backward (Partials), so
    BatchNorm + activation costs one read and one write forward, two reads and one write backward.
    fp32 rows, fp32 or bf16 maps; the output has the input's shape and storage type."""
    accepts_bn_input = True
    kind = None
    alpha = 0.0

    def __init__(self, layer_name):
        super().__init__(layer_name)
        self._state = None  # a training forward's record: (BNOut or None, input tensor, shape, storage type)

    def __repr__(self):
        return "{}({})".format(type(self).__name__, self.layer_name)

    def _name(self):
        return "{}({})".format(type(self).__name__, self.layer_name)

    def forward(self, X, test_mode=False):
        self._require_on_gpu()
        if isinstance(X, JoinOut):
            X = X.materialize()
        bn = X if isinstance(X, BNOut) else None
        x = bn.x if bn is not None else X
        dtype = act_dtype(x)
        if len(x.shape) == 4:
            x = to_nhwc(as_device(x, dtype))
            y = empty_nhwc(*x.shape, dtype=x.dtype)
        elif len(x.shape) == 2:
            if dtype == BF16:
                raise ValueError("{}: bf16 storage is taken for 4-D maps only".format(self._name()))
            x = rows(as_device(x, dtype))
            y = torch.empty_like(x)
        else:
            raise ValueError("{}: expected 2-D rows or a 4-D map, got shape {}".format(self._name(), tuple(x.shape)))
        plain, bnx = _ACT_FWD[x.dtype]
        if bn is not None:
            getattr(lib, bnx)(x.data_ptr(), x.numel(), x.shape[1], *bn.bn_args(), self.kind, self.alpha, y.data_ptr(),
                              stream_handle())
        else:
            getattr(lib, plain)(x.data_ptr(), x.numel(), self.kind, self.alpha, y.data_ptr(), stream_handle())
        if not test_mode:
            self._state = (bn, x, tuple(x.shape), x.dtype)
        return y

    def backward(self, upstream_dx):
        self._require_on_gpu()
        if self._state is None:
            raise RuntimeError("{}: backward needs a training-mode forward first (a test-mode forward records "
                               "nothing)".format(self._name()))
        bn, x, shape, dtype = self._state
        if lattice_tag(upstream_dx):
            raise ValueError("{}: a lattice-form gradient cannot be taken".format(self._name()))
        if act_dtype(upstream_dx) != dtype:
            raise ValueError("{} backward of mixed storage types: {} input vs {} gradient".format(
                self._name(), dtype, act_dtype(upstream_dx)))
        if tuple(upstream_dx.shape) != shape:
            raise ValueError("{} backward shape mismatch: {} vs {}".format(self._name(), tuple(upstream_dx.shape),
                                                                           shape))
        if len(shape) == 4:
            dy = to_nhwc(as_device(upstream_dx, dtype))
            dx = empty_nhwc(*shape, dtype=dtype)
        else:
            dy = rows(as_device(upstream_dx, dtype))
            dx = torch.empty_like(dy)
        plain, bnx = _ACT_BWD[dtype]
        if bn is not None:
            # the gradient w.r.t. the BNOut, and stage 1 of its owner's backward on the same pass
            C = shape[1]
            P = x.numel() // C
            args = bn.bn_args()  # (raises on a stale BNOut before anything is armed)
            nb = lib.dk_bn_workspace_bytes(P, C)
            part = Partials(bn, lib.dk_bn_partial_blocks(P, C), C, dy.device)
            r = getattr(lib, bnx)(x.data_ptr(), dy.data_ptr(), P, C, *args, self.kind, self.alpha, dx.data_ptr(),
                                  part.ptr, nb, stream_handle())
            part.hand(dx, r)
            return dx
        getattr(lib, plain)(x.data_ptr(), dy.data_ptr(), dy.numel(), self.kind, self.alpha, dx.data_ptr(),
                            stream_handle())
        return dx

    def save_to_h5(self, open_f, save_grads=True):
        from ..network.checkpoint import save_layer
        save_layer(self, open_f, save_grads)

    def load_from_h5(self, open_f, load_grads=True):
        from ..network.checkpoint import load_layer
        load_layer(self, open_f, load_grads)


class LeakyReLu(_Activation):
    """y = v > 0 ? v : alpha * v; the derivative at 0 is alpha (torch.nn.functional.leaky_relu)."""
    kind = ACT_LEAKY

    def __init__(self, layer_name, alpha=0.01):
        super().__init__(layer_name)
        self.alpha = checked_alpha(layer_name, alpha)

    def __repr__(self):
        return "LeakyReLu({}, alpha={})".format(self.layer_name, self.alpha)


class ReLu6(_Activation):
    """y = min(max(v, 0), 6); the derivative is 1 iff 0 < v < 6 (torch.nn.functional.relu6)."""
    kind = ACT_RELU6


class HardSwish(_Activation):
    """y = v * min(max(v + 3, 0), 6) / 6; the derivative is 0 for v <= -3, (2 v + 3) / 6 on (-3, 3), 1 for v >= 3
    (torch.nn.functional.hardswish, whose backward takes the open interval)."""
    kind = ACT_HARDSWISH


class SiLu(_Activation):
    """y = v * s(v), s(v) = 1 / (1 + e^-v); the derivative is s (1 + v (1 - s)) (torch.nn.functional.silu)."""
    kind = ACT_SILU
