"""SGD with momentum (reference: optimisers/SGDMomentum.py).

Parameter discovery is the reference's (:7-14): every top-level layer with
``learned_params`` plus one level of ``layer_list`` -- so ResidualBlock skip
projections are *not* updated (a reference quirk, kept as the default).
``update_skip_projections=True`` (an extension, not in the reference) also updates each
ResidualBlock's ``skip_projection``; pass the same flag to ``parallel.DataParallel`` so
their gradients are all-reduced.  ``update_weights`` computes,
per parameter tensor, ``d = -lr * g + momentum * v;  W += d;  v = d`` (:31-39) -- as one
multi-tensor HIP launch over all tensors instead of ~4 CuPy kernels per tensor.
``save_state_to_h5`` / ``load_state_from_h5`` (an extension) keep the velocities and the
hyper-parameters in a file of their own (optimisers/_multi.py).
"""
from __future__ import annotations

from .._hip import lib
from ._multi import MultiTensorOptimiser


class SGDMomentum(MultiTensorOptimiser):
    _HYPER = ("momentum",)
    _STATE_WORDS = ("parameters, grads and velocities", "grad / velocity")

    def __init__(self, network, learning_rate, momentum, update_skip_projections=False):
        super().__init__(network, learning_rate, update_skip_projections)
        self.momentum = momentum

    def _launch(self, table, ntens, total_blocks, stream):
        lib.dk_sgd_momentum_multi_f32(table, ntens, total_blocks, float(self.learning_rate), float(self.momentum),
                                      1.0, stream)
