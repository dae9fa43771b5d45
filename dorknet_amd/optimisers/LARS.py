"""LARS: layer-wise adaptive rate scaling (You, Gitman, Ginsburg 2017; an extension: the reference has
no such optimiser).  Momentum SGD in the reference's form (optimisers/SGDMomentum.py:33-39, the
learning rate inside the velocity, which is also the paper's form) whose step for each tensor is
scaled by a trust ratio, so that a learning rate scaled up with the batch does not blow up the
layers whose ``||w|| / ||g||`` is small.

For tensor ``t``, with ``adapt`` = (its key is in ``adapt_params``: by default conv and dense
``weights``, not ``gamma``, ``beta`` or ``bias``)::

    wn = (float) sqrt(sum_i (double) w_i^2)          gn = (float) sqrt(sum_i (double) g_i^2)
    ratio = 1
    if adapt and wn > 0 and gn > 0:
        ratio = (trust * wn) / ((gn + wd * wn) + eps)
    per element:
        g' = g + wd * w             only if adapt and wd != 0
        step = (-lr) * ratio        (exactly -lr when ratio == 1)
        d = step * g' + mom * v;    w = w + d;    v = d

``trust`` (``trust_coefficient``), ``wd`` (``weight_decay``), ``eps``, ``lr`` and ``mom`` are formed
in Python double and rounded to fp32 once, where they meet the data.  Every operation is one correctly
rounded fp32 operation in the order written, denormals kept; the sums are fp64 in a fixed order.  A
tensor that is not adapted gets SGDMomentum's update bit for bit.  A non-finite norm is not
special-cased: it propagates, so a poisoned step stays visible.

``update_weights`` is three multi-tensor HIP launches over one table (rows
``{w, g, v, n, first_block, flags}``, 2048 elements per block, bit 0 of ``flags`` = adapt) with no
allocation and no host synchronisation: ``dk_lars_norms_multi_f32`` (two fp64 partial sums per
block, then one block per tensor) and ``dk_lars_multi_f32`` (the update, each block reading its own
tensor's ratio).  Afterwards ``last_stats`` is the device tensor ``[ntens, 4]`` of
``{wn, gn, ratio, 0}`` rows (the norms are those before the step) and ``stat_names`` lists
``(layer_name, param)`` in row order.  ``measure_tensor_norms()`` runs the norm launches alone and
returns ``last_stats``: a per-tensor monitoring readout that changes no parameter.  The stats tensor
and the workspace are allocated when the table is rebuilt (a pointer or a size changed), not per
step.

Layers with an ``l2`` regulariser already add ``strength * W`` to their gradient, so ``gn`` includes
that term and ``weight_decay`` defaults to 0.  Under ``parallel.DataParallel`` call
``update_weights()`` after ``finish()``: the norms are fixed-order sums, so every rank forms the same
ratios from the same averaged gradients.  ``clip_grad_norm(opt, c)`` (optimisers/clip.py) works
unchanged: it scales the gradients before the norms are taken.

State: ``grad_cache`` (the velocities), as in SGDMomentum.  State file (optimisers/_multi.py): the
attributes ``type`` (``LARS``), ``learning_rate``, ``momentum``, ``trust_coefficient``,
``weight_decay``, ``eps``, ``update_skip_projections`` and the datasets SGDMomentum writes.
``adapt_params`` is a constructor choice and is not stored.
"""
from __future__ import annotations

import torch

from .._hip import lib, stream_handle
from ._multi import MultiTensorOptimiser


class LARS(MultiTensorOptimiser):
    _HYPER = ("momentum", "trust_coefficient", "weight_decay", "eps")
    _PER_BLOCK = 2048  # kChunk (csrc/multi_tensor.hip)
    _STATE_WORDS = ("parameters, grads and velocities", "grad / velocity")

    def __init__(self, network, learning_rate, momentum=0.9, trust_coefficient=0.001, weight_decay=0.0, eps=1e-8,
                 adapt_params=("weights",), update_skip_projections=False):
        super().__init__(network, learning_rate, update_skip_projections)
        self.momentum = momentum
        self.trust_coefficient = trust_coefficient
        self.weight_decay = weight_decay
        self.eps = eps
        self.adapt_params = tuple(adapt_params)
        self.last_stats = None
        self._stats = self._ws = None

    # -- the device table: {w, g, v, n, first_block, flags}, 48 bytes per row -------------------

    def _entries(self):
        out = []
        for layer in self.learnable_layers:
            for param in layer.learned_params.keys():
                out.append((layer.learned_params[param], layer.grads[param], self.grad_cache[layer][param],
                            1 if param in self.adapt_params else 0))
        return out

    @property
    def stat_names(self):
        """(layer_name, param) of each row of ``last_stats``."""
        return [(layer.layer_name, param) for layer in self.learnable_layers for param in layer.learned_params.keys()]

    def _ensure(self):
        t = self._dev
        if t.ensure(self._entries()) or self._stats is None:
            self._stats = torch.zeros((t.ntens, 4), dtype=torch.float32, device="cuda")
            self._ws = torch.empty(max(int(lib.dk_lars_workspace_bytes(t.blocks)), 16), dtype=torch.uint8,
                                   device="cuda")
        return t

    def _norms(self, t, stream):
        if t.ntens:  # (an empty stats tensor has no address to hand over)
            lib.dk_lars_norms_multi_f32(t.ptr, t.ntens, t.blocks, float(self.trust_coefficient),
                                        float(self.weight_decay), float(self.eps), self._stats.data_ptr(),
                                        self._ws.data_ptr(), self._ws.numel(), stream)
        self.last_stats = self._stats

    def measure_tensor_norms(self):
        """The two norm launches alone: ``last_stats`` for the parameters and gradients as they are
        now.  Nothing is updated and nothing waits for the device."""
        self._norms(self._ensure(), stream_handle())
        return self.last_stats

    def update_weights(self):
        t = self._ensure()
        stream = stream_handle()
        self._norms(t, stream)
        if t.ntens:
            lib.dk_lars_multi_f32(t.ptr, t.ntens, t.blocks, float(self.learning_rate), float(self.momentum),
                                  float(self.weight_decay), self._stats.data_ptr(), stream)
