"""Clipping by the global gradient norm (an extension; no counterpart in the reference).

``clip_grad_norm(optimiser, max_norm)`` is torch's ``clip_grad_norm_`` over the gradients the
optimiser applies (``optimiser.learnable_layers``), as three launches and no host synchronisation:

* ``dk_grad_norm_multi_f32``: stage 1 writes one fp64 sum of squares per 2048-element chunk, stage 2
  (one block) adds them in a fixed order and writes ``out[0] = (float)sqrt(total)`` and
  ``out[1] = min(1, max_norm / (out[0] + 1e-6))``, one fp32 rounding per operation;
* ``dk_grad_scale_multi_f32``: ``g = out[1] * g`` in place, one rounding; a scale of 1 writes nothing.

The norm is bit-identical from run to run, and across ranks that hold the same gradients.  The
table (one 24-byte row ``{g, n, first_block}`` per gradient tensor), the workspace and the two
output words are cached on the optimiser (``_clip_state``); the table (dorknet_amd/_table.py) and the
workspace are rebuilt only when a pointer or a size changes.
``Adam(max_grad_norm=c)`` uses the norm launches alone and reads ``out[1]`` in its update.
"""
from __future__ import annotations

import math

import torch

from .._hip import lib, stream_handle
from .._table import DeviceTable

CHUNK = 2048  # elements per block of the norm and scale kernels (kChunk, csrc/multi_tensor.hip)


class _ClipState:
    """The table, the workspace sized for it and the two output words."""

    def __init__(self):
        self.table = DeviceTable(CHUNK, "clip_grad_norm", ("grads", "grad"), 1, hint="call it after network.to_gpu()")
        self.ws = self.out = None
        self.checked_under = None  # Adam: the signature of its own table this one was last checked under


def _state(optimiser):
    st = getattr(optimiser, "_clip_state", None)
    if st is None:
        st = optimiser._clip_state = _ClipState()
    t = st.table
    if t.ensure([(layer.grads[k],) for layer in optimiser.learnable_layers for k in layer.learned_params.keys()]):
        st.checked_under = None
        st.ws = torch.empty(max(int(lib.dk_grad_norm_workspace_bytes(t.blocks)), 8), dtype=torch.uint8,
                            device="cuda")
        if st.out is None:
            st.out = torch.zeros(2, dtype=torch.float32, device="cuda")
    return st


def measure_grad_norm(optimiser, max_norm=None, unchanged=False):
    """The two norm launches.  Returns the device tensor ``out``: ``out[0]`` the norm, ``out[1]`` the
    clip scale for ``max_norm`` (1 with ``max_norm`` None, <= 0 or infinite: measure only).
    ``unchanged``: the caller has just checked that no gradient tensor moved since this table was
    last checked (Adam's own table signature holds the same pointers): it is used without a walk."""
    st = getattr(optimiser, "_clip_state", None) if unchanged else None
    if st is None:
        st = _state(optimiser)
    c = 0.0 if max_norm is None or not math.isfinite(max_norm) else float(max_norm)
    t = st.table
    lib.dk_grad_norm_multi_f32(t.ptr, t.ntens, t.blocks, c, st.out.data_ptr(), st.ws.data_ptr(), st.ws.numel(),
                               stream_handle())
    return st.out


def clip_grad_norm(optimiser, max_norm):
    """Scale the gradients of ``optimiser.learnable_layers`` in place so that their global l2 norm is
    at most ``max_norm``; returns the norm before scaling as a 0-d device tensor (no host
    synchronisation: read it with ``float()`` only where a wait is acceptable).  Works for SGD,
    SGDMomentum, RMSProp, Adam and LARS.

    Under ``parallel.DataParallel`` call it after ``finish()``: the norm is then of the averaged
    gradients and bit-identical on every rank, so every rank applies the same scale."""
    out = measure_grad_norm(optimiser, max_norm)
    t = optimiser._clip_state.table
    lib.dk_grad_scale_multi_f32(t.ptr, t.ntens, t.blocks, out.data_ptr() + 4, stream_handle())
    return out[0]
