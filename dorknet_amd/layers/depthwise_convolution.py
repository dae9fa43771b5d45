"""Depthwise (per-channel) convolution (reference: layers/depthwise_convolution.py).

The reference GPU path (forward_cp :85-102, backward_cp :198-221) pads the input into a
copy, runs one thread per output with nine global read-modify-writes, and in backward
funnels N*OH*OW atomicAdds into each weight.  Here: direct NHWC kernels with register
accumulation, bounds checks instead of a padded copy, and a two-stage deterministic
weight-gradient reduction (dk_dwconv_fwd_f32 / _dgrad_f32 / _wgrad_f32).

Public surface identical to the reference: constructor (:11-13), weights (C, R, S),
bias (C,), ``forward`` / ``backward`` / ``__repr__`` (:41-51).
"""
from __future__ import annotations


import torch

from .._env import getenv
from .._hip import HipError, deferred_wgrad_reduce, lib, stream_handle, workspace
from .._tensor import BF16, empty_nhwc, ptr, to_nhwc
from ._bn_input import NO_BN, BNGrad, BNOut, JoinOut, Partials, add_residual, bn_args, fused_residual
from ._common import add_regulariser_grad, grad_buffer, init_weights, l2_strength, weight_grad
from .layer import Layer

# Per storage type, each entry point with the queries that size its launch (names: resolved on
# `lib` at the call).  Forward and stride-1 dgrad: (the _ex entry, its row query).  The bf16 launches
# run whole columns per thread: their own, smaller row counts.
_FWD_EX = {torch.float32: ("dk_dwconv_fwd_ex_f32", "dk_dwconv_fwd_stats_rows"),
           BF16: ("dk_dwconv_fwd_ex_bf16", "dk_dwconv_fwd_bf16_stats_rows")}
_FWD_JOIN = ("dk_dwconv_fwd_join_f32", "dk_dwconv_fwd_stats_rows")
_DGRAD_EX = {torch.float32: ("dk_dwconv_dgrad_ex_f32", "dk_dwconv_dgrad_stats_rows"),
             BF16: ("dk_dwconv_dgrad_ex_bf16", "dk_dwconv_dgrad_bf16_stats_rows")}
# The dgrad with the input's residual join (fp32); a strided _ex dgrad's row count is this query's too
_DGRAD_JOIN = ("dk_dwconv_dgrad_join_f32", "dk_dwconv_dgrad_join_rows")
# The one-pass backward by stride: (entry, row query, workspace query); with the input's residual
# join (fp32 only) the same queries
_BWD_FUSED = {1: {torch.float32: ("dk_dwconv_bwd_bnbwd_f32", "dk_dwconv_bwd_bnbwd_stats_rows",
                                  "dk_dwconv_bwd_bnbwd_workspace_bytes"),
                  BF16: ("dk_dwconv_bwd_bnbwd_bf16", "dk_dwconv_bwd_bnbwd_bf16_stats_rows",
                         "dk_dwconv_bwd_bnbwd_bf16_workspace_bytes")},
              2: {torch.float32: ("dk_dwconv_bwd_s2_bnbwd_f32", "dk_dwconv_bwd_s2_stats_rows",
                                  "dk_dwconv_bwd_s2_workspace_bytes"),
                  BF16: ("dk_dwconv_bwd_s2_bnbwd_bf16", "dk_dwconv_bwd_s2_stats_rows",
                         "dk_dwconv_bwd_s2_workspace_bytes")}}
_BWD_FUSED_JOIN = {1: ("dk_dwconv_bwd_bnbwd_join_f32", "dk_dwconv_bwd_bnbwd_stats_rows",
                       "dk_dwconv_bwd_bnbwd_workspace_bytes"),
                   2: ("dk_dwconv_bwd_s2_bnbwd_join_f32", "dk_dwconv_bwd_s2_stats_rows",
                       "dk_dwconv_bwd_s2_workspace_bytes")}


class DepthwiseConvLayer(Layer):
    def __init__(self, layer_name, filter_block_shape=None,
                 stride=1, padding=1, with_bias=True,
                 weight_regulariser=None, weight_initialiser="normal"):
        """
        filter_block_shape = (num_incoming_channels, num_filter_rows, num_filter_cols)
        """
        super().__init__(layer_name)
        self.stride = stride
        self.padding = padding
        self.with_bias = with_bias
        self.weight_regulariser = weight_regulariser
        self.weight_initialiser = weight_initialiser
        if filter_block_shape is not None:
            self.num_filters, self.f_rows, self.f_cols = filter_block_shape
            weights = init_weights(tuple(filter_block_shape), weight_initialiser, 2 * self.num_filters)
            self.learned_params = {"weights": weights}
            self.grads = {"weights": weights * 0}
            if with_bias:
                bias = (weights[:, 0, 0] * 0).copy()
                self.learned_params["bias"] = bias
                self.grads["bias"] = bias * 0
        else:
            self.num_filters = None
            self.learned_params = {}
            self.grads = {}

    def __repr__(self):
        out = "DepthwiseConvLayer({}, ".format(self.layer_name)
        if self.num_filters is not None:
            out += "filter_block_shape=({}, {}, {}), ".format(self.num_filters, self.f_rows, self.f_cols)
        out += "stride={}, padding={}, with_bias={}, weight_regulariser={})".format(
            self.stride, self.padding, self.with_bias, repr(self.weight_regulariser))
        return out

    def _w_rsc(self, st):
        w = self.learned_params["weights"]
        C, R, S = w.shape
        w_rsc = torch.empty((R, S, C), dtype=torch.float32, device=w.device)
        lib.dk_dw_weight_rsc_f32(w.data_ptr(), C, R, S, w_rsc.data_ptr(), st)
        return w_rsc

    accepts_bn_input = True   # forward(BNOut): the preceding BatchNorm is applied on load
    produces_bn_stats = True  # forward(..., bn_stats=StatsRequest): emits the next BN's statistics

    def join_geometry_ok(self):
        """forward(JoinOut) can form the residual join on load (dk_dwconv_fwd_join_f32): 3 x 3, pad
        1, stride 1 or 2, no bias (the shapes and dtype are checked at the call)."""
        return (self.num_filters is not None and self.f_rows == 3 and self.f_cols == 3 and self.padding == 1
                and self.stride in (1, 2) and not self.with_bias)

    def _takes_join(self, X):
        return (self.join_geometry_ok() and X.dim() == 4 and X.dtype == torch.float32
                and X.shape[1] == self.num_filters and X.shape[1] % 4 == 0 and X.shape[1] <= 512)

    def forward(self, X, test_mode=False, bn_stats=None):
        self._require_on_gpu()
        st = stream_handle()
        if isinstance(X, JoinOut):
            if not X.written and self._takes_join(X):
                return self._forward_join(X, test_mode, bn_stats, st)
            X = X.materialize()
        bn = X if isinstance(X, BNOut) and X.dim() == 4 and X.shape[1] % 4 == 0 else None
        x = bn.x if bn is not None else to_nhwc(X)
        N, C, H, W = x.shape
        R, S = self.f_rows, self.f_cols
        # float-then-int output size (depthwise_convolution.py:89-90)
        self.num_row_patches = ((H + 2 * self.padding - R) / self.stride) + 1
        self.num_col_patches = ((W + 2 * self.padding - S) / self.stride) + 1
        OH, OW = int(self.num_row_patches), int(self.num_col_patches)
        entry, rows_query = _FWD_EX[x.dtype]  # (bf16 storage, BASELINE config 5: the _bf16 entry points)
        y = empty_nhwc(N, C, OH, OW, x.dtype)
        bias = self.learned_params["bias"] if self.with_bias else None
        rows = 0
        if bn_stats is not None and not test_mode and self.stride in (1, 2):
            rows = getattr(lib, rows_query)(N, OH, OW, C, self.stride)
        w = self.learned_params["weights"]  # W[C][R][S], read in place by the _ex entry
        stats = bn_stats.arm_buffer(rows, C, x.device, N * OH * OW) if rows else None
        r = getattr(lib, entry)(x.data_ptr(), N, H, W, C, w.data_ptr(), R, S, self.stride, self.padding, ptr(bias),
                                y.data_ptr(), OH, OW, *bn_args(bn), ptr(stats), st)
        if stats is not None:
            bn_stats.launched(stats, r)
        if not test_mode:
            # the reference keeps the *padded* input (:87-88); padding is implicit here, and
            # a BNOut input is kept as the BatchNorm's raw input + parameters
            self.X = x
            self._bn_in = bn
        return y

    def _forward_join(self, J, test_mode, bn_stats, st):
        """forward on a residual block's output not yet written (JoinOut): the join is formed as the
        input window is loaded and stored once (dk_dwconv_fwd_join_f32); the layer then holds y as
        its input, exactly as after the join pass."""
        N, C, H, W = J.shape
        R, S = self.f_rows, self.f_cols
        self.num_row_patches = ((H + 2 * self.padding - R) / self.stride) + 1
        self.num_col_patches = ((W + 2 * self.padding - S) / self.stride) + 1
        OH, OW = int(self.num_row_patches), int(self.num_col_patches)
        y = empty_nhwc(N, C, OH, OW)
        entry, rows_query = _FWD_JOIN
        rows = getattr(lib, rows_query)(N, OH, OW, C, self.stride) if bn_stats is not None and not test_mode else 0
        stats = bn_stats.arm_buffer(rows, C, J.device, N * OH * OW) if rows else None
        r = getattr(lib, entry)(*J.join_args(), N, H, W, C, self.learned_params["weights"].data_ptr(), self.stride,
                                0, y.data_ptr(), OH, OW, ptr(stats), st)
        if stats is not None:
            bn_stats.launched(stats, r)
        J.mark_written()
        if not test_mode:
            self.X = J.y
            self._bn_in = None
        return y

    accepts_residual = True  # backward(dy, residual=R) returns dx + R (the residual join, fused)

    skips_input_grad = True  # backward(dy, need_dx=False): parameter gradients only (chain_backward)

    def accepts_bn_grad(self, bn_layer):
        """backward(BNGrad): the following BatchNorm's apply, this layer's dgrad and its weight
        gradient run as one pass -- 3x3, padding 1, no bias, C % 4 == 0: stride 1
        (dk_dwconv_bwd_bnbwd_f32 / _bf16) and stride 2 (dk_dwconv_bwd_s2_bnbwd_f32 / _bf16, C / 4
        dividing 256; DORKNET_DW_S2_FUSED=0 turns it off)."""
        bx = getattr(bn_layer, "X", None)
        return getattr(self, "X", None) is not None and bx is not None and self._takes_bn_grad(bx)

    def _takes_bn_grad(self, bx):
        x = self.X
        if x.dim() != 4 or bx.dim() != 4 or x.dtype not in (torch.float32, BF16) or bx.dtype != x.dtype:
            return False
        N, C, H, W = x.shape
        if not (self.f_rows == 3 and self.f_cols == 3 and self.padding == 1 and not self.with_bias and C % 4 == 0):
            return False
        if self.stride == 2:
            return (getenv("DORKNET_DW_S2_FUSED", "1") != "0" and 256 % (C // 4) == 0
                    and tuple(bx.shape) == (N, C, (H + 1) // 2, (W + 1) // 2))
        return self.stride == 1 and tuple(bx.shape) == tuple(x.shape)

    accepts_join = True  # backward(BNGrad, residual=R, join=relu): the input's residual join rides on dx

    def _join_ok(self, join, need_dx):
        """`join`: the ReLu that closed the residual block whose output is this layer's input
        (residual_block.py:75).  The fused backward takes over its backward and stage 1 of its
        BatchNorm's (dk_dwconv_bwd_bnbwd_join_f32) when this layer has no input BatchNorm."""
        x = self.X
        jb = getattr(join, "_join_bn", None)
        mask = getattr(join, "_mask", None)
        if not (need_dx and self._bn_in is None and jb is not None and tuple(jb.x.shape) == tuple(x.shape)
                and jb.x.dtype == torch.float32 and jb.x.is_contiguous(memory_format=torch.channels_last)):
            return False
        if mask is None:
            # a join that left no mask (JoinOut): the fused backwards take it as x > 0 (x is the
            # join's output); the plain join dgrad rebuilds it (ReLu._mask_from_join)
            return (getattr(join, "_join_y", None) is not None
                    and getattr(join, "_join_y_ptr", None) == x.data_ptr())
        return tuple(mask.shape) == tuple(x.shape) and mask.is_contiguous(memory_format=torch.channels_last)

    def takes_lattice_residual(self, join, s):
        """backward(dy, residual=R, join=relu) adds R given as the compact stride-s lattice (a
        strided pointwise skip projection's un-widened input gradient) in the fused join dgrad
        (dk_dwconv_dgrad_join_f32, residual_lattice = s): fp32, this layer's stride is s, and the
        join fuses.  Any other path widens such a residual first (dense_residual)."""
        x = getattr(self, "X", None)
        if (x is None or x.dim() != 4 or x.dtype != torch.float32 or self.stride != s or s < 2 or join is None
                or self.with_bias or not self._join_ok(join, True)):
            return False
        N, C, H, W = x.shape
        return getattr(lib, _DGRAD_JOIN[1])(N, H, W, C, self.f_rows, self.f_cols, s, self.padding) > 0

    def _backward_bn_grad(self, G, residual, need_dx, join=None):
        """One-pass backward from the following BatchNorm's deferred gradient (see
        accepts_bn_grad), stride 1 or 2: dx (+ the residual addend, + the input BatchNorm's backward
        partial sums) and the weight gradient; dy itself is never written.  With the input's residual
        join (fp32, _join_ok) the _join entries: dx masked by y > 0 (y = this layer's input, the
        join's output) or by the stored mask, stage 1 of the join's BatchNorm on the store, and at
        stride 2 a strided skip's compact lattice residual added as such."""
        st = stream_handle()
        x = self.X
        N, C, H, W = x.shape
        R, S = self.f_rows, self.f_cols
        s2 = self.stride == 2
        w = self.learned_params["weights"]
        gw = grad_buffer(self, "weights", (C, R, S))
        s = l2_strength(self.weight_regulariser)
        bn = self._bn_in
        dx = empty_nhwc(N, C, H, W, x.dtype) if need_dx else None
        joined = join is not None and not (s2 and x.dtype == BF16) and self._join_ok(join, need_dx)
        residual, res, lat = fused_residual(residual, dx, 2 if joined and s2 else 0) if need_dx else (None, None, 0)
        if s2 and not joined and residual is not None and res is None:
            raise NotImplementedError("{}: the fused stride-2 backward needs an NHWC residual".format(self.layer_name))
        entry, rows_query, ws_query = _BWD_FUSED_JOIN[self.stride] if joined else _BWD_FUSED[self.stride][x.dtype]
        # the BatchNorm whose stage 1 rides on the dx store: the join's, or this layer's input's
        pbn = join._join_bn if joined else bn if need_dx else None
        rows = getattr(lib, rows_query)(N, H, W, C) if pbn is not None else 0
        g = to_nhwc(G.g)
        if s2:
            geometry, filt = (N, H, W, C, (H + 1) // 2, (W + 1) // 2), ()
            nb = getattr(lib, ws_query)(N, H, W, C)
        else:
            geometry, filt = (N, H, W, C), (R, S, self.padding)
            nb = getattr(lib, ws_query)(N, H, W, C, R, S)
        if not joined:
            on_load = bn_args(bn)
        else:
            if s2:
                mask = lat  # (the mask is y > 0; this operand says how the residual is laid out)
            else:
                # x IS the join's output: the kernel takes the mask as x > 0 instead of reading it
                # (DORKNET_JOIN_MASK=1 reads the stored mask)
                from_y = getattr(join, "_join_y_ptr", None) == x.data_ptr() and getenv("DORKNET_JOIN_MASK") != "1"
                if not from_y and join._mask is None:
                    join._mask_from_join()
                mask = 0 if from_y else join._mask.data_ptr()
            on_load = (mask, pbn.x.data_ptr(), pbn.mean.data_ptr(), pbn.invstd.data_ptr())
        part = Partials(pbn, rows, C, x.device)
        # the weight-gradient reduce on the side stream (not with a non-l2 regulariser, whose term
        # is added to gw on this stream right after)
        red = deferred_wgrad_reduce(self, nb, s is not None)
        with red:
            r = getattr(lib, entry)(g.data_ptr(), G.x.data_ptr(), *geometry, *G.bnbwd_args(), x.data_ptr(),
                                    w.data_ptr(), *filt, s or 0.0, gw.data_ptr(), ptr(dx), ptr(res), *on_load,
                                    part.ptr, red.ws, nb, st)
        red.flush()
        if s is None:
            add_regulariser_grad(gw, w, self.weight_regulariser)
        if not need_dx:
            return None
        part.hand(dx, r)
        if joined:
            join.join_backward_done()
            if not s2 and residual is not None and res is None:
                raise RuntimeError("{}: the fused join needs the residual in the dgrad epilogue".format(
                    self.layer_name))
        elif residual is not None and res is None:
            dx = add_residual(dx, residual)  # (a new tensor: the BN then recomputes its sums)
        return dx

    def backward(self, upstream_dx, residual=None, need_dx=True, join=None):
        self._require_on_gpu()
        if isinstance(upstream_dx, BNGrad):
            if self._takes_bn_grad(upstream_dx.x):
                return self._backward_bn_grad(upstream_dx, residual, need_dx, join)
            upstream_dx = upstream_dx.materialize()
        st = stream_handle()
        dy = to_nhwc(upstream_dx)
        x = self.X
        N, C, H, W = x.shape
        R, S = self.f_rows, self.f_cols
        OH, OW = int(self.num_row_patches), int(self.num_col_patches)
        w = self.learned_params["weights"]
        bf = x.dtype == BF16
        if bf and (dy.dtype != BF16 or self.with_bias):
            raise NotImplementedError("{}: bf16 storage needs a bf16 gradient and no bias".format(self.layer_name))
        bn = self._bn_in
        wnb = lib.dk_dwconv_wgrad_workspace_bytes(N, OH, OW, C, R, S)

        def launch(wl2, s, gw, sst):
            args = (dy.data_ptr(), x.data_ptr(), N, H, W, C, R, S, self.stride, self.padding, OH, OW, wl2, s, gw,
                    workspace.get(wnb), wnb)
            if bf:
                lib.dk_dwconv_wgrad_bnx_bf16(*args, *bn_args(bn), sst)
            elif bn is not None:
                lib.dk_dwconv_wgrad_bnx_f32(*args, *bn.bn_args(), sst)
            else:
                lib.dk_dwconv_wgrad_f32(*args, sst)
        weight_grad(self, dy, x, N * OH * OW, C, (C, R, S), launch)
        if not need_dx:
            return None
        dx = empty_nhwc(N, C, H, W, x.dtype)
        nb = lib.dk_dwconv_dgrad_workspace_bytes(C, R, S)
        entry, rows_query = _DGRAD_EX[x.dtype]
        join_entry, join_rows_query = _DGRAD_JOIN
        geometry = (dy.data_ptr(), N, OH, OW, C, w.data_ptr(), R, S, self.stride, self.padding, dx.data_ptr(), H, W)
        jrows = (getattr(lib, join_rows_query)(N, H, W, C, R, S, self.stride, self.padding)
                 if join is not None and not bf and self._join_ok(join, True) else 0)
        # a residual handed over as its compact lattice is added as such by the join dgrad only
        residual, res, lat = fused_residual(residual, dx, self.stride if jrows else 0, retry=False)
        if residual is not None and res is None:
            jrows = 0
        # the input BatchNorm's stage-1 partials ride on the dgrad store: stride 1 in the dgrad's
        # epilogue, stride > 1 on the sub-pixel dgrad's store (same row count as its join form)
        rows = 0
        if bn is not None and R == S:
            if self.stride == 1:
                rows = getattr(lib, rows_query)(N, H, W, C, 1)
            else:
                rows = getattr(lib, join_rows_query)(N, H, W, C, R, S, self.stride, self.padding)
        if rows and self.padding <= R - 1 and (residual is None or res is not None):
            # + stage 1 of the input BatchNorm's backward, in the dgrad epilogue (+ the residual)
            part = Partials(bn, rows, C, dx.device)
            r = getattr(lib, entry)(*geometry, workspace.get(nb), nb, ptr(res), bn.x.data_ptr(), *bn.bn_args(),
                                    part.ptr, st)
            part.hand(dx, r)
            return dx
        if jrows:
            # the input's residual join: its ReLU backward and its BatchNorm's stage 1 on the store
            jb = join._join_bn
            if join._mask is None:
                join._mask_from_join()
            part = Partials(jb, jrows, C, dx.device)
            r = getattr(lib, join_entry)(*geometry, workspace.get(nb), nb, ptr(res), lat, join._mask.data_ptr(),
                                         jb.x.data_ptr(), jb.mean.data_ptr(), jb.invstd.data_ptr(), part.ptr, st)
            part.hand(dx, r)
            join.join_backward_done()
            return dx
        if bf:
            if residual is not None and res is None:
                raise NotImplementedError("{}: bf16 residual must be a bf16 NHWC tensor".format(self.layer_name))
            getattr(lib, entry)(*geometry, workspace.get(nb), nb, ptr(res), 0, *NO_BN, 0, st)
            return dx
        if res is not None:
            try:
                getattr(lib, entry)(*geometry, workspace.get(nb), nb, res.data_ptr(), 0, *NO_BN, 0, st)
                return dx
            except HipError:  # geometry without a fused residual (generic gather dgrad)
                pass
        lib.dk_dwconv_dgrad_f32(*geometry, workspace.get(nb), nb, st)
        return add_residual(dx, residual) if residual is not None else dx

    def save_to_h5(self, open_f, save_grads=True):
        from ..network.checkpoint import save_layer
        save_layer(self, open_f, save_grads)

    def load_from_h5(self, open_f, load_grads=True):
        from ..network.checkpoint import load_layer
        load_layer(self, open_f, load_grads)
