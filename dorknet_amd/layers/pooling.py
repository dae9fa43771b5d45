"""Global average pooling (reference: layers/pooling.py:10-43) and max pooling (:45-77).

``forward``: mean over (H, W) -> (N, C); ``backward``: (1/(H*W)) * dy broadcast back.
A bf16 input (bf16 activation storage) is pooled to fp32 means -- the head after it (DenseLayer,
the loss) is fp32 -- and its backward returns a bf16 gradient (dk_gap_fwd_bf16 / dk_gap_bwd_bf16).

MaxPoolLayer is CPU Cython in the reference (layers/pooling_cy.pyx) with an int32 location map the
size of the input; here it is dk_maxpool_* (dorknet_amd/csrc/maxpool.hip): fp32 or bf16 storage,
one uint8 location per output element, and a BatchNorm (+ ReLu) in front of it applied on load
(layers/_bn_input.py), see DESIGN.md.
"""
from __future__ import annotations

import torch

from .._env import getenv
from .._hip import lib, stream_handle
from .._tensor import BF16, act_dtype, empty_nhwc, rows, to_nhwc
from ._bn_input import BNOut, JoinOut, lattice_tag
from .layer import Layer

# per storage type: the pooling backward; the max-pool forward (plain, BatchNorm on load)
_GAP_BWD = {torch.float32: "dk_gap_bwd_f32", BF16: "dk_gap_bwd_bf16"}
_MAXPOOL_FWD = {torch.float32: ("dk_maxpool_fwd_f32", "dk_maxpool_fwd_bnx_f32"),
                BF16: ("dk_maxpool_fwd_bf16", "dk_maxpool_fwd_bnx_bf16")}


class GlobalAveragePoolingLayer(Layer):
    """
    Takes the mean over spatial dimensions, reducing to one feature per channel per image
    """

    def __init__(self, layer_name):
        super().__init__(layer_name)

    def __repr__(self):
        return "GlobalAveragePoolingLayer({})".format(self.layer_name)

    def takes_join_input(self):
        """forward(JoinOut): the last residual block's output is pooled as it is formed
        (dk_gap_join_fwd_f32, bit-identical to the join pass + the pooling) and never stored."""
        from ._chain import fusion_enabled
        return fusion_enabled() and getenv("DORKNET_FUSE_JOIN_FWD") != "0"

    def forward(self, X, test_mode=False):
        self._require_on_gpu()
        if isinstance(X, JoinOut):
            if not X.written and X.dim() == 4 and X.dtype == torch.float32:
                return self._forward_join(X, test_mode)
            X = X.materialize()
        x = to_nhwc(X)
        N, C, H, W = x.shape
        self.spatial_shape = (H, W)
        self._in_dtype = x.dtype
        out = torch.empty((N, C), dtype=torch.float32, device=x.device)
        fwd = lib.dk_gap_fwd_bf16 if x.dtype == BF16 else lib.dk_gap_fwd_f32
        fwd(x.data_ptr(), N, H * W, C, out.data_ptr(), stream_handle())
        return out

    def _forward_join(self, J, test_mode):
        N, C, H, W = J.shape
        self.spatial_shape = (H, W)
        self._in_dtype = torch.float32
        out = torch.empty((N, C), dtype=torch.float32, device=J.device)
        if not test_mode and J.mask is None:
            # the join's ReLU backward takes its mask (y itself is never stored)
            J.mask = torch.empty((N, C, H, W), dtype=torch.uint8, device=J.device, memory_format=torch.channels_last)
        a, b = J.join_args()[:6], J.join_args()[6:12]
        lib.dk_gap_join_fwd_f32(*a, *b, N, H * W, C, 0 if J.mask is None else J.mask.data_ptr(), out.data_ptr(),
                                stream_handle())
        J.mark_pooled()
        return out

    def backward(self, upstream_dx):
        self._require_on_gpu()
        dy = rows(upstream_dx)
        N, C = dy.shape
        H, W = self.spatial_shape
        bf = getattr(self, "_in_dtype", torch.float32) == BF16
        dx = empty_nhwc(N, C, H, W, BF16 if bf else torch.float32)
        getattr(lib, _GAP_BWD[dx.dtype])(dy.data_ptr(), N, H * W, C, dx.data_ptr(), stream_handle())
        return dx

    def save_to_h5(self, open_f, save_grads=True):
        from ..network.checkpoint import save_layer
        save_layer(self, open_f, save_grads)

    def load_from_h5(self, open_f, load_grads=True):
        pass


class MaxPoolLayer(Layer):
    """
    Max over non-overlapping stride x stride windows (reference: layers/pooling.py:45-77,
    layers/pooling_cy.pyx:8-88).

    OH = H // stride, OW = W // stride: trailing rows / columns that fill no window are not pooled
    and get a zero gradient (the reference reads out of bounds there).  The window is scanned
    row-major with a strict >, so the first maximum wins (pool_train).  An fp32 input gives fp32
    y / dx, a bf16 input bf16 (max and copy are exact).  A BNOut input is normalised (+ ReLU) as it
    is loaded (dk_maxpool_fwd_bnx_*), bit-identical to pooling the materialised BatchNorm output.
    """
    accepts_bn_input = True
    MAX_STRIDE = 16  # the recorded location m * stride + n is one byte

    def __init__(self, layer_name, input_shape=None, stride=2):
        # (input_shape: accepted and ignored, the reference never uses it)
        super().__init__(layer_name)
        if isinstance(stride, bool) or int(stride) != stride or not 1 <= int(stride) <= self.MAX_STRIDE:
            raise ValueError("MaxPoolLayer({}): stride must be an integer in 1..{}, got {!r}".format(
                layer_name, self.MAX_STRIDE, stride))
        self.stride = int(stride)
        self.max_locs = None      # uint8 [N][C][OH][OW] (NHWC bytes): m * stride + n of each maximum
        self._in_shape = None
        self._in_dtype = None

    def __repr__(self):
        return "MaxPoolLayer(stride={})".format(self.stride)

    def forward(self, X, test_mode=False):
        self._require_on_gpu()
        if isinstance(X, JoinOut):
            X = X.materialize()
        bn = X if isinstance(X, BNOut) else None
        x = to_nhwc(bn.x if bn is not None else X)
        N, C, H, W = x.shape
        s = self.stride
        OH, OW = H // s, W // s
        if OH < 1 or OW < 1:
            raise ValueError("MaxPoolLayer({}): a {}x{} input has no {}x{} window".format(self.layer_name, H, W, s, s))
        y = empty_nhwc(N, C, OH, OW, x.dtype)
        if test_mode:
            idx = None
            self.max_locs = self._in_shape = self._in_dtype = None
        else:
            idx = torch.empty((N, C, OH, OW), dtype=torch.uint8, device=x.device, memory_format=torch.channels_last)
            self.max_locs, self._in_shape, self._in_dtype = idx, (N, C, H, W), x.dtype
        ip = 0 if idx is None else idx.data_ptr()
        plain, bnx = _MAXPOOL_FWD[x.dtype]
        if bn is not None:
            getattr(lib, bnx)(x.data_ptr(), N, H, W, C, s, *bn.bn_args(), y.data_ptr(), ip, stream_handle())
        else:
            getattr(lib, plain)(x.data_ptr(), N, H, W, C, s, y.data_ptr(), ip, stream_handle())
        return y

    def backward(self, upstream_dx):
        self._require_on_gpu()
        if self.max_locs is None:
            raise RuntimeError("MaxPoolLayer({}): backward needs a training-mode forward first (a test-mode "
                               "forward records no locations)".format(self.layer_name))
        if lattice_tag(upstream_dx):
            raise ValueError("MaxPoolLayer({}): a lattice-form gradient cannot be pooled back".format(self.layer_name))
        if act_dtype(upstream_dx) != self._in_dtype:
            raise ValueError("MaxPoolLayer({}) backward of mixed storage types: {} input vs {} gradient".format(
                self.layer_name, self._in_dtype, act_dtype(upstream_dx)))
        dy = to_nhwc(upstream_dx)
        N, C, H, W = self._in_shape
        s = self.stride
        if tuple(dy.shape) != (N, C, H // s, W // s):
            raise ValueError("MaxPoolLayer({}) backward shape mismatch: {} vs {}".format(
                self.layer_name, tuple(dy.shape), (N, C, H // s, W // s)))
        dx = empty_nhwc(N, C, H, W, self._in_dtype)
        bwd = lib.dk_maxpool_bwd_bf16 if self._in_dtype == BF16 else lib.dk_maxpool_bwd_f32
        bwd(dy.data_ptr(), self.max_locs.data_ptr(), N, H, W, C, s, dx.data_ptr(), stream_handle())
        return dx

    def save_to_h5(self, open_f, save_grads=True):
        """An extension: the reference defines no checkpoint methods for this layer."""
        from ..network.checkpoint import save_layer
        save_layer(self, open_f, save_grads)

    def load_from_h5(self, open_f, load_grads=True):
        from ..network.checkpoint import load_layer
        load_layer(self, open_f, load_grads)
