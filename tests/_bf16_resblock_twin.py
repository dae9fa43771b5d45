"""Bf16Twin (tests/test_gpu_bf16_fullsize.py) extended to residual blocks.  TEST INFRASTRUCTURE.

The torch fp64 twin with the bf16 path's roundings emulated; besides the leaf-layer rules of Bf16Twin
(a stored layer output and its gradient are bf16; a pointwise layer's weights and a BatchNorm output it
consumes on load are rounded as bf16 MFMA operands; a BatchNorm applied on load by a depthwise layer
stays fp32) it rounds where a residual block stores bf16:

  * the skip projection's output (and the gradient w.r.t. the skip projection's input);
  * the join output y = ReLU(bn(chain) + skip), rounded once from the fp32 sum -- the chain's last
    BatchNorm is applied on load by the join in fp32 and is not rounded (fuse=True); with
    DORKNET_FUSE=0 that BatchNorm writes its bf16 output first and the join adds two stored tensors;
  * the gradient after the join's ReLU backward;
  * the block's input gradient, chain + skip: rounded once when the chain's first dgrad adds the skip
    gradient in its epilogue (fuse=True); with DORKNET_FUSE=0 the chain's gradient is stored first and a
    separate add rounds the sum again.

With DORKNET_FUSE=0 every layer runs on its own and stores its output, so every BatchNorm / ReLU output
is rounded, also in front of a depthwise layer.
"""
import numpy as np
import torch

from tests.test_gpu_bf16_fullsize import Bf16Twin, _q


class ResBf16Twin(Bf16Twin):

    def __init__(self, layers, emulate=True, fuse=True):
        super().__init__(layers, emulate)
        self.fuse = fuse

    def _leaf(self, l, h):
        from dorknet_amd.layers.pointwise_convolution import PointwiseConvLayer
        if self.emulate and isinstance(l, PointwiseConvLayer):
            w = self._p(l, "weights")
            self.params[(l.layer_name, "weights")] = _q(w, True, False)  # bf16 MFMA operand
            try:
                return self._layer(l, h)
            finally:
                self.params[(l.layer_name, "weights")] = w
        return self._layer(l, h)

    def _chain(self, L, h, last_bn_on_load=False):
        """The leaf rules of Bf16Twin.run over the list L; last_bn_on_load: the list's closing
        BatchNorm is applied on load by a residual join in fp32 (not rounded)."""
        from dorknet_amd.layers.activations import ReLu
        from dorknet_amd.layers.batch_norm import BatchNormLayer
        from dorknet_amd.layers.depthwise_convolution import DepthwiseConvLayer
        from dorknet_amd.layers.residual_block import ResidualBlock
        for i, l in enumerate(L):
            if isinstance(l, ResidualBlock):
                h = self._block(l, h)
                continue
            h = self._leaf(l, h)
            if not self.emulate:
                continue
            nxt = L[i + 1] if i + 1 < len(L) else None
            if isinstance(l, (BatchNormLayer, ReLu)):
                if isinstance(l, BatchNormLayer) and isinstance(nxt, ReLu) and self.fuse:
                    continue  # one apply with the ReLU
                if nxt is None and last_bn_on_load and self.fuse:
                    fwd = False
                else:
                    fwd = not (self.fuse and isinstance(nxt, DepthwiseConvLayer))
                h = _q(h, fwd=fwd, bwd=True)
            else:
                h = _q(h)  # a stored bf16 layer output; its gradient is stored bf16 too
        return h

    def _block(self, blk, x):
        if not self.emulate:
            return self._layer(blk, x)
        x = _q(x, fwd=False, bwd=True)  # chain + skip gradient: one rounding of the sum
        # DORKNET_FUSE=0: the chain's input gradient is stored (rounded) before the separate add
        xc = x if self.fuse else _q(x, fwd=False, bwd=True)
        h = self._chain(blk.layer_list, xc, last_bn_on_load=True)
        if blk.skip_projection is not None:
            xs = _q(x, fwd=False, bwd=True)  # the skip projection's input gradient, stored bf16
            s = _q(self._leaf(blk.skip_projection, xs))  # its output, stored bf16
        else:
            s = x
        v = _q(h + s, fwd=False, bwd=True)  # the gradient after the join's ReLU backward
        return _q(torch.relu(v))  # the join output, rounded once from the fp32 sum

    def run(self, X, dY, input_grad=False):
        x = torch.tensor(np.asarray(X, np.float64), requires_grad=input_grad)
        h = self._chain(self.layers, x)
        h.backward(torch.as_tensor(np.asarray(dY, np.float64)))
        grads = {}
        for (name, k), p in self.params.items():
            g = p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)
            if k == "weights" and name in self.l2:
                g = g + self.l2[name] * p.detach()
            grads[(name, k)] = g.numpy()
        return h.detach().numpy(), (x.grad.numpy() if input_grad else None), grads
