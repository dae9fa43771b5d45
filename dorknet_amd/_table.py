"""The device table of the multi-tensor kernels (dorknet_amd/csrc/multi_tensor.hip): one int64 row
``{pointers..., n, first_block, extra words...}`` per tensor, ``first_block`` the running sum of
``ceil(n / per_block)``.  The five layouts of include/dorknet_hip.h are this one shape:

    SGD, SGDMomentum, RMSProp   {w, g, state, n, first_block}              256 elements per block
    Adam                        {w, g, m, v, n, first_block, flags}        256
    LARS                        {w, g, v, n, first_block, flags}           2048 (flags bit 0: adapt)
    the gradient norm / scale   {g, n, first_block}                        2048
    the l2 term                 {w, n, first_block, strength as fp32}      2048

An entry is a tuple: ``pointers`` tensors, then the integer extra words; the first tensor defines
``n``.  A pointer column may be None throughout (plain SGD's state): 0 pointers.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

_PTR, _NUMEL = torch.Tensor.data_ptr, torch.Tensor.numel


def table_columns(entries, pointers):
    """The integer columns ``[pointer columns..., n, extra columns...]`` of ``entries``: what a table is
    built from, and its signature.  This is the walk every call pays, so it goes column by column at
    C speed.  Anything but a tensor among the pointers raises TypeError."""
    if not entries:
        return []
    cols = list(zip(*entries))
    out = [[0] * len(c) if c[0] is None and c.count(None) == len(c) else list(map(_PTR, c))
           for c in cols[:pointers]]
    out.append(list(map(_NUMEL, cols[0])))
    out += cols[pointers:]
    return out


def table_rows(columns, pointers, per_block):
    """(int64 rows [ntens][pointers + 2 + extras], total blocks) for the columns of ``table_columns``."""
    if not columns:
        return np.zeros((0, pointers + 2), dtype=np.int64), 0
    blocks = [-(-n // per_block) for n in columns[pointers]]
    first = np.cumsum([0] + blocks[:-1])
    cols = [*columns[:pointers + 1], first, *columns[pointers + 1:]]
    return np.ascontiguousarray(np.array(cols, dtype=np.int64).T), sum(blocks)


@functools.lru_cache(maxsize=None)
def f32_word(x):
    """The table word {fp32(x), 0.0f}."""
    return int(np.array([x, 0.0], dtype=np.float32).view(np.int64)[0])


class DeviceTable:
    """``ensure(entries)`` builds the table at the first call and again only when a pointer, a size
    or an extra word changed.  Then ``ptr`` (the device address), ``ntens`` and ``blocks`` are the
    first three arguments of the C entry, ``rows`` is the device tensor and ``sig`` the columns it
    was built from: the same object until the next rebuild.

    ``who`` and ``words`` = (what the tensors are, what to call a size mismatch) word the errors."""

    def __init__(self, per_block, who, words, pointers, hint="build the optimiser after network.to_gpu()"):
        self.per_block, self.who, self.words, self.pointers, self.hint = per_block, who, words, pointers, hint
        self.sig = self.rows = self.ptr = None
        self.ntens = self.blocks = 0

    def _check(self, entries):
        k = self.pointers
        empty = [j for j in range(1, k) if all(e[j] is None for e in entries)]
        for e in entries:
            tensors = [t for j, t in enumerate(e[:k]) if j not in empty]
            for t in tensors:
                if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32
                        and t.is_contiguous()):
                    raise RuntimeError("{}: {} must be contiguous fp32 device tensors ({})".format(
                        self.who, self.words[0], self.hint))
            if any(t.numel() != tensors[0].numel() for t in tensors):
                raise ValueError("{}: {} size mismatch".format(self.who, self.words[1]))

    def ensure(self, entries):
        """True if the table was (re)built."""
        try:
            sig = table_columns(entries, self.pointers)
        except (AttributeError, TypeError):  # host arrays: the check says what is wrong
            self._check(entries)
            raise
        if sig == self.sig:
            return False
        self._check(entries)
        rows, self.blocks = table_rows(sig, self.pointers, self.per_block)
        self.rows = torch.as_tensor(rows, device="cuda")
        self.ptr, self.ntens, self.sig = self.rows.data_ptr(), len(rows), sig
        return True
