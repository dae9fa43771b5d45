"""Adam and AdamW (an extension: the reference has neither).

The update is ``torch.optim.Adam`` / ``torch.optim.AdamW`` (non-amsgrad; the weight decay is
decoupled in both classes here) written as single fp32 operations.  The host scalars are formed in
Python double and rounded to fp32 once, where they meet the data (the rule RMSProp.py follows).
With ``t`` the 1-based step number::

    omb1 = 1 - beta1            omb2 = 1 - beta2
    neg_step = -(lr / (1 - beta1**t))
    sbc2 = sqrt(1 - beta2**t)
    keep = 1 - lr * weight_decay

    g' = s * g                     only with max_grad_norm (s: the clip scale); otherwise g' = g
    w  = keep * w                  only for tensors named in decay_params and weight_decay != 0
    m  = beta1 * m + omb1 * g'
    v  = beta2 * v + omb2 * (g' * g')
    den = sqrt(v) / sbc2 + eps
    w  = w + neg_step * (m / den)

``update_weights`` is one multi-tensor HIP launch (dk_adam_multi_f32): each operation one correctly
rounded fp32 operation in the order written, denormals kept.  With ``max_grad_norm`` set it is three
launches and still no host synchronisation: the two stages of the global gradient norm
(optimisers/clip.py), then the update reading the clip scale from device memory; the gradients
themselves are left as they were.  ``last_grad_norm`` is then the 0-d device view of the norm.

State: ``m[layer][param]`` and ``v[layer][param]``, zeros shaped like the grads, and ``step_count``
(0 at construction; ``update_weights`` increments it and uses it as ``t``).  Decay applies to the
tensors whose key is in ``decay_params``: by default conv and dense ``weights``, not ``gamma``,
``beta`` or ``bias``.  ``AdamW`` is Adam with ``weight_decay`` required (default 0.01 in torch; here
it has to be given); the state file's ``type`` tells the two apart.

State file (optimisers/_multi.py): the attributes ``type``, ``learning_rate``, ``beta1``, ``beta2``,
``eps``, ``weight_decay``, ``step_count``, ``update_skip_projections`` and the datasets
``optimiser/<layer_name>/<param>/m`` and ``.../v``.  ``max_grad_norm`` and ``decay_params`` are
constructor choices and are not stored.
"""
from __future__ import annotations

import math

from .._hip import lib, stream_handle
from ._multi import MultiTensorOptimiser
from .clip import measure_grad_norm


def adam_scalars(learning_rate, beta1, beta2, weight_decay, t):
    """(omb1, omb2, neg_step, sbc2, keep) in Python double for the 1-based step number t."""
    lr, b1, b2 = float(learning_rate), float(beta1), float(beta2)
    return (1 - b1, 1 - b2, -(lr / (1 - b1 ** t)), math.sqrt(1 - b2 ** t), 1 - lr * float(weight_decay))


class Adam(MultiTensorOptimiser):
    _HYPER = ("beta1", "beta2", "eps", "weight_decay")
    _COUNTERS = ("step_count",)
    _POINTERS = 4  # w, g, m, v
    _STATE_WORDS = ("parameters, grads and moments", "grad / moment")

    def __init__(self, network, learning_rate, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0,
                 decay_params=("weights",), max_grad_norm=None, update_skip_projections=False):
        super().__init__(network, learning_rate, update_skip_projections)
        self.beta1 = beta1
        self.beta2 = beta2
        self.eps = eps
        self.weight_decay = weight_decay
        self.decay_params = tuple(decay_params)
        self.max_grad_norm = max_grad_norm
        self.step_count = 0
        self.last_grad_norm = None

    def _init_state(self):
        self.m = self._zero_state()
        self.v = self._zero_state()

    # -- the device table: {w, g, m, v, n, first_block, flags}, 56 bytes per row ----------------

    def _entries(self):
        out = []
        for layer in self.learnable_layers:
            for param in layer.learned_params.keys():
                out.append((layer.learned_params[param], layer.grads[param], self.m[layer][param],
                            self.v[layer][param], 1 if param in self.decay_params else 0))
        return out

    def _launch(self, table, ntens, total_blocks, stream, grad_scale=None):
        """The update for step number ``step_count`` (at least 1)."""
        omb1, omb2, neg_step, sbc2, keep = adam_scalars(self.learning_rate, self.beta1, self.beta2,
                                                        self.weight_decay, max(int(self.step_count), 1))
        lib.dk_adam_multi_f32(table, ntens, total_blocks, float(self.beta1), omb1, float(self.beta2), omb2,
                              neg_step, sbc2, float(self.eps), keep, grad_scale, stream)

    def update_weights(self):
        t = self._dev
        t.ensure(self._entries())
        grad_scale = None
        if self.max_grad_norm is not None:
            # the table's signature holds every gradient's pointer and size: while it is the one the
            # norm's table was last checked under, that table needs no second walk over the tensors
            st = getattr(self, "_clip_state", None)
            out = measure_grad_norm(self, self.max_grad_norm,
                                    unchanged=st is not None and st.checked_under is t.sig)
            self._clip_state.checked_under = t.sig
            self.last_grad_norm = out[0]
            grad_scale = out.data_ptr() + 4
        self.step_count += 1
        self._launch(t.ptr, t.ntens, t.blocks, stream_handle(), grad_scale)

    # -- the state file -----------------------------------------------------------------------

    def _state_items(self):
        self._check_layer_names()
        return [("optimiser/{}/{}/{}".format(layer.layer_name, k, which), state[layer][k])
                for layer in self.learnable_layers for k in self.m[layer]
                for which, state in (("m", self.m), ("v", self.v))]


class AdamW(Adam):
    """Adam with the weight decay required."""

    def __init__(self, network, learning_rate, weight_decay, beta1=0.9, beta2=0.999, eps=1e-8,
                 decay_params=("weights",), max_grad_norm=None, update_skip_projections=False):
        super().__init__(network, learning_rate, beta1, beta2, eps, weight_decay, decay_params, max_grad_norm,
                         update_skip_projections)
