"""Plain SGD (reference: optimisers/SGD.py).

``update_weights`` computes, per parameter tensor, ``d = -lr * g;  W += d`` (:20-24) as one
multi-tensor HIP launch (dk_sgd_multi_f32), each operation rounded once to fp32.

Deviation from the reference: its discovery loop (:8-11) tests and appends ``layer`` (the
ResidualBlock, whose own ``learned_params`` is None) where SGDMomentum.py:10-12 uses ``l``, so it
never updates anything inside a residual block -- a typo, not a semantic.  Discovery here is
SGDMomentum's: top-level layers plus one level of ``layer_list``, and skip projections only with
``update_skip_projections=True`` (an extension; pass the same flag to ``parallel.DataParallel``).
``save_state_to_h5`` / ``load_state_from_h5`` (an extension) keep the hyper-parameters in a file
of their own; plain SGD has no state tensors (optimisers/_multi.py).
"""
from __future__ import annotations

from .._hip import lib
from ._multi import MultiTensorOptimiser


class SGD(MultiTensorOptimiser):
    _HAS_STATE = False
    _STATE_WORDS = ("parameters and grads", "grad")

    def __init__(self, network, learning_rate, update_skip_projections=False):
        super().__init__(network, learning_rate, update_skip_projections)

    def _launch(self, table, ntens, total_blocks, stream):
        lib.dk_sgd_multi_f32(table, ntens, total_blocks, float(self.learning_rate), stream)
