"""RMSProp (reference: optimisers/RMSProp.py, which is NumPy only and never ran on a GPU).

``update_weights`` computes, per parameter tensor (:28-36),
``c = decay * c + (1 - decay) * g**2;  d = -lr * g / sqrt(c + 1e-5);  W += d`` as one multi-tensor
HIP launch (dk_rmsprop_multi_f32): the reference's expression in IEEE fp32, one rounding per
operation, in the order written.  ``1 - decay_rate`` is formed in double here and rounded to fp32
once, as the reference's Python scalar is when it meets the array.  ``grad_cache`` holds ``c``:
``{layer: {param: tensor}}``, zeros shaped like the grads.

Deviation from the reference: its discovery loop (:12-15) tests and appends ``layer`` (the
ResidualBlock, whose own ``learned_params`` is None) where SGDMomentum.py:10-12 uses ``l``, so it
never updates anything inside a residual block -- a typo, not a semantic.  Discovery here is
SGDMomentum's: top-level layers plus one level of ``layer_list``, and skip projections only with
``update_skip_projections=True`` (an extension; pass the same flag to ``parallel.DataParallel``).
``save_state_to_h5`` / ``load_state_from_h5`` (an extension) keep the cache and the
hyper-parameters in a file of their own (optimisers/_multi.py).
"""
from __future__ import annotations

from .._hip import lib
from ._multi import MultiTensorOptimiser

EPS = 1e-5  # RMSProp.py:35


class RMSProp(MultiTensorOptimiser):
    _HYPER = ("decay_rate",)
    _STATE_WORDS = ("parameters, grads and caches", "grad / cache")

    def __init__(self, network, learning_rate, decay_rate, update_skip_projections=False):
        super().__init__(network, learning_rate, update_skip_projections)
        self.decay_rate = decay_rate

    def _launch(self, table, ntens, total_blocks, stream):
        decay = float(self.decay_rate)
        lib.dk_rmsprop_multi_f32(table, ntens, total_blocks, float(self.learning_rate), decay, 1.0 - decay, EPS,
                                 stream)
