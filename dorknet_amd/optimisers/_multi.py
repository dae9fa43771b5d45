"""What the optimisers share: parameter discovery, the DataParallel flag handshake, the device
table of the multi-tensor kernels (dorknet_amd/csrc/multi_tensor.hip) and the state file.

Parameter discovery is the reference's SGDMomentum.py:7-14: every top-level layer with
``learned_params`` plus one level of ``layer_list``, skip projections only with
``update_skip_projections=True`` (an extension).  The reference's SGD.py:8-11 and
RMSProp.py:12-15 loop over ``layer_list`` too but test and append ``layer`` (the block, whose own
``learned_params`` is None) where SGDMomentum.py uses ``l``: a typo under which nothing inside a
ResidualBlock is ever updated.  All three optimisers here use SGDMomentum's discovery.

The table has one 40-byte row ``{w, g, state, n, first_block}`` per parameter tensor (``state``:
the velocity or the squared-gradient cache, 0 for plain SGD), 256 elements per block.  It is
built (dorknet_amd/_table.py) at the first ``update_weights`` and again only when a pointer or a
size changes; the scalars travel as kernel arguments.  After that an update is one launch: no
allocation, no host synchronisation.

State file (``save_state_to_h5`` / ``load_state_from_h5``; its own file, not the weights file):
a group ``optimiser`` with the attributes ``type`` (the class name), ``learning_rate``,
``momentum`` or ``decay_rate`` where the class has one, ``update_skip_projections``, and one fp32
dataset ``optimiser/<layer_name>/<param>`` per state tensor, in the parameter's shape.

Adam (optimisers/Adam.py) is built on the same base with a wider row and state of its own: it
overrides ``_init_state``, ``_entries`` and ``_state_items`` and names its integer attribute
(``step_count``) in ``_COUNTERS``.  LARS (optimisers/LARS.py) keeps SGDMomentum's state and adds a
flags word to the row; its kernels take 2048 elements per block (``_PER_BLOCK``) and its update is
three launches, so it overrides ``_entries`` and ``update_weights``.
"""
from __future__ import annotations

import numpy as np
import torch

from .._hip import stream_handle
from .._table import DeviceTable


def discover_learnable_layers(network, update_skip_projections=False):
    out = []
    for layer in network.layers:
        if layer.learned_params is not None:
            out.append(layer)
        if hasattr(layer, "layer_list"):  # For composite layers like ResidualBlock
            for l in layer.layer_list:
                if l.learned_params is not None:
                    out.append(l)
            skip = getattr(layer, "skip_projection", None)
            if update_skip_projections and skip is not None and skip.learned_params:
                out.append(skip)
    return out


class MultiTensorOptimiser:
    """Base of SGD, SGDMomentum, RMSProp and Adam.  A subclass names its extra hyper-parameter in
    ``_HYPER`` (also the state file's attribute), says in ``_HAS_STATE`` whether it keeps a state
    tensor per parameter (``grad_cache``), and launches its kernel in ``_launch``.  ``_entries``
    lists the table's rows: ``_POINTERS`` tensors each, then integer words (dorknet_amd/_table.py)."""

    _HYPER = ()
    _COUNTERS = ()  # integer attributes of the state file (Adam's step_count)
    _HAS_STATE = True
    _POINTERS = 3  # w, g, state
    _PER_BLOCK = 256  # elements per block of the class's kernels (LARS: 2048)
    _STATE_WORDS = ("parameters, grads and state", "grad / state")

    def __init__(self, network, learning_rate, update_skip_projections=False):
        name = type(self).__name__
        self.network = network
        self.update_skip_projections = update_skip_projections
        # a data-parallel wrapper must all-reduce exactly the gradients this optimiser applies
        # (parallel.DataParallel checks the same pair from its side)
        dp_flag = getattr(network, "_dp_update_skip_projections", None)
        if dp_flag is not None and dp_flag != update_skip_projections:
            raise ValueError("{}(update_skip_projections={}) disagrees with DataParallel's "
                             "update_skip_projections={}: skip-projection gradients would be applied "
                             "un-averaged".format(name, update_skip_projections, dp_flag))
        try:
            network._opt_update_skip_projections = update_skip_projections
        except AttributeError:
            pass
        self.learnable_layers = discover_learnable_layers(network, update_skip_projections)
        self.learning_rate = learning_rate
        self._init_state()
        self._dev = DeviceTable(self._PER_BLOCK, name, self._STATE_WORDS, self._POINTERS)

    def _zero_state(self):
        """{layer: {param: zeros shaped like the gradient}}"""
        out = {}
        for layer in self.learnable_layers:
            layer_d = {}
            for k, v in layer.grads.items():
                layer_d[k] = torch.zeros_like(v) if isinstance(v, torch.Tensor) else np.zeros_like(v)
            out[layer] = layer_d
        return out

    def _init_state(self):
        if self._HAS_STATE:
            self.grad_cache = self._zero_state()

    def set_learning_rate(self, new_lr):
        self.learning_rate = new_lr

    def multiply_learning_rate(self, multiplier):
        self.learning_rate *= multiplier

    # -- the device table ---------------------------------------------------------------------

    def _entries(self):
        out = []
        for layer in self.learnable_layers:
            for param in layer.learned_params.keys():
                w = layer.learned_params[param]
                g = layer.grads[param]
                v = self.grad_cache[layer][param] if self._HAS_STATE else None
                out.append((w, g, v))
        return out

    def _launch(self, table, ntens, total_blocks, stream):
        raise NotImplementedError

    @property
    def _table(self):
        """The table on the device (None before the first update)."""
        return self._dev.rows

    def update_weights(self):
        t = self._dev
        t.ensure(self._entries())
        self._launch(t.ptr, t.ntens, t.blocks, stream_handle())

    # -- the state file -----------------------------------------------------------------------

    def _check_layer_names(self):
        seen = set()
        for layer in self.learnable_layers:
            if layer.layer_name in seen:
                raise ValueError("{}: two learnable layers are named {!r}; the state file keys its "
                                 "datasets by layer name".format(type(self).__name__, layer.layer_name))
            seen.add(layer.layer_name)

    def _state_items(self):
        """[(dataset path, state tensor or array)], refusing layer names that would collide."""
        self._check_layer_names()
        if not self._HAS_STATE:
            return []
        return [("optimiser/{}/{}".format(layer.layer_name, k), v)
                for layer in self.learnable_layers for k, v in self.grad_cache[layer].items()]

    def save_state_to_h5(self, fname):
        from ..network.checkpoint import _write, open_h5
        items = self._state_items()
        with open_h5(fname, "w") as f:
            g = f.create_group("optimiser")
            g.attrs["type"] = type(self).__name__
            g.attrs["learning_rate"] = np.float64(self.learning_rate)
            for h in self._HYPER:
                g.attrs[h] = np.float64(getattr(self, h))
            for h in self._COUNTERS:
                g.attrs[h] = np.int64(getattr(self, h))
            g.attrs["update_skip_projections"] = bool(self.update_skip_projections)
            for path, v in items:
                _write(f, path, v)

    def load_state_from_h5(self, fname):
        """Restore the hyper-parameters and copy the stored state into the existing state tensors
        in place (the device table stays valid).  Everything is read and checked first: a
        ValueError leaves the optimiser as it was."""
        from ..network.checkpoint import _as_str, open_h5
        name = type(self).__name__
        items = self._state_items()
        with open_h5(fname, "r") as f:
            if "optimiser" not in f:
                raise ValueError("{}: {} holds no optimiser state".format(name, fname))
            attrs = f["optimiser"].attrs
            stored = _as_str(attrs["type"]) if "type" in attrs else None
            if stored != name:
                raise ValueError("{}: {} holds the state of a {}".format(name, fname, stored))
            for h in ("learning_rate", *self._HYPER, *self._COUNTERS, "update_skip_projections"):
                if h not in attrs:
                    raise ValueError("{}: {} has no attribute {!r}".format(name, fname, h))
            if bool(attrs["update_skip_projections"]) != bool(self.update_skip_projections):
                raise ValueError("{}: {} was saved with update_skip_projections={}".format(
                    name, fname, bool(attrs["update_skip_projections"])))
            scalars = {h: float(attrs[h]) for h in ("learning_rate", *self._HYPER)}
            scalars.update({h: int(attrs[h]) for h in self._COUNTERS})
            values = []
            for path, v in items:
                if path not in f:
                    raise ValueError("{}: {} has no dataset {}".format(name, fname, path))
                d = f[path]
                if d.shape is None or tuple(d.shape) != tuple(v.shape):
                    raise ValueError("{}: dataset {} has shape {}, the state tensor {}".format(
                        name, path, d.shape, tuple(v.shape)))
                values.append(np.ascontiguousarray(d[:], dtype=np.float32))
        for (_, v), a in zip(items, values):
            if isinstance(v, torch.Tensor):
                v.copy_(torch.from_numpy(a))
            else:
                v[...] = a
        for h, x in scalars.items():
            setattr(self, h, x)
