"""The device-table builder (dorknet_amd/_table.py) without a GPU: the rows of all four layouts of
include/dorknet_hip.h against rows written out by hand, the columns (the signature) of CPU tensors, and
the refusals of host tensors, word for word.  (What needs device tensors -- the size mismatch and the
rebuild rule -- is in tests/test_gpu_optimisers.py.)"""
import struct

import numpy as np
import pytest
import torch

from dorknet_amd._table import DeviceTable, f32_word, table_columns, table_rows
from tests import _head_ref as R

W, G, M, V = (0x7f0000001000, 0x7f0000002000), (0x7f0000003000, 0x7f0000004000), (0x10, 0x20), (0x30, 0x40)


def test_rows_of_the_four_layouts():
    # SGD / SGDMomentum / RMSProp: {w, g, state, n, first_block}, 256 elements per block
    rows, blocks = table_rows([list(W), list(G), list(M), [257, 5]], 3, 256)
    assert rows.dtype == np.int64 and rows.flags.c_contiguous and blocks == 3
    assert rows.tobytes() == struct.pack("<5q", W[0], G[0], M[0], 257, 0) + struct.pack("<5q", W[1], G[1], M[1], 5, 2)
    # plain SGD: the state pointers are 0
    rows, _ = table_rows([list(W), list(G), [0, 0], [257, 5]], 3, 256)
    assert rows.tolist() == [[W[0], G[0], 0, 257, 0], [W[1], G[1], 0, 5, 2]]
    # Adam: {w, g, m, v, n, first_block, flags}
    rows, blocks = table_rows([list(W), list(G), list(M), list(V), [256, 1], (1, 0)], 4, 256)
    assert blocks == 2 and rows.tobytes() == (struct.pack("<7q", W[0], G[0], M[0], V[0], 256, 0, 1)
                                              + struct.pack("<7q", W[1], G[1], M[1], V[1], 1, 1, 0))
    # the gradient norm and scale: {g, n, first_block}, 2048 elements per block
    rows, blocks = table_rows([list(G), [2049, 2048]], 1, 2048)
    assert blocks == 3 and rows.tobytes() == struct.pack("<3q", G[0], 2049, 0) + struct.pack("<3q", G[1], 2048, 2)
    # the l2 term: {w, n, first_block, fp32 strength, fp32 pad}, as tests/_head_ref.py states it
    rows, blocks = table_rows([list(W), [5, 3000], (f32_word(0.5), f32_word(1e-3))], 1, 2048)
    assert blocks == 3 and rows.tobytes() == R.l2_table_bytes(W, [5, 3000], [0.5, 1e-3])
    # no tensors: no rows, of the layout's width without extras
    rows, blocks = table_rows([], 3, 256)
    assert rows.shape == (0, 5) and rows.dtype == np.int64 and blocks == 0


@pytest.mark.parametrize("per_block", [256, 2048])
def test_first_block_is_the_running_sum_of_blocks(per_block):
    sizes = [1, per_block - 1, per_block, per_block + 1, 3 * per_block + 5, 2]
    rows, blocks = table_rows([list(range(8, 14)), sizes], 1, per_block)
    assert rows[:, 1].tolist() == sizes and rows[:, 2].tolist() == [0, 1, 2, 3, 5, 9] and blocks == 10


def test_columns_of_tensors():
    w = [torch.zeros(7), torch.zeros(3, 4)]
    g = [torch.zeros(7), torch.zeros(3, 4)]
    m = [torch.zeros(7), torch.zeros(12)]
    cols = table_columns([(w[0], g[0], None), (w[1], g[1], None)], 3)  # plain SGD: no state
    assert cols == [[t.data_ptr() for t in w], [t.data_ptr() for t in g], [0, 0], [7, 12]]
    cols = table_columns([(w[0], g[0], m[0], 1), (w[1], g[1], m[1], 0)], 3)  # an extra word per row
    assert [list(c) for c in cols] == [[t.data_ptr() for t in w], [t.data_ptr() for t in g],
                                       [t.data_ptr() for t in m], [7, 12], [1, 0]]
    assert cols == table_columns([(w[0], g[0], m[0], 1), (w[1], g[1], m[1], 0)], 3)   # it is the signature:
    assert cols != table_columns([(w[0], g[0], m[0], 1), (w[1], g[1], m[1], 1)], 3)   # an extra word,
    assert cols != table_columns([(w[0], g[0], m[0], 1), (w[1], g[1], m[0], 0)], 3)   # a pointer
    assert cols != table_columns([(w[0], g[0], m[0], 1), (torch.zeros(11), g[1], m[1], 0)], 3)  # or a size changes it
    assert table_columns([], 3) == []
    with pytest.raises(TypeError):
        table_columns([(np.zeros(3, np.float32), g[0], None)], 3)
    with pytest.raises(TypeError):  # a state column is None throughout or not at all
        table_columns([(w[0], g[0], None), (w[1], g[1], m[1])], 3)
    assert f32_word(0.5) == 0x3f000000 and f32_word(-2.0) == 0xc0000000 and f32_word(0.0) == 0


def test_host_tensors_are_refused_word_for_word():
    host = np.zeros(3, np.float32)
    cpu = torch.zeros(3)
    opt = DeviceTable(256, "RMSProp", ("parameters, grads and caches", "grad / cache"), 3)
    for entry in [(host, host, host), (cpu, cpu, cpu), (cpu, cpu, None), (cpu, None, cpu)]:
        with pytest.raises(RuntimeError) as e:
            opt.ensure([entry])
        assert str(e.value) == ("RMSProp: parameters, grads and caches must be contiguous fp32 device tensors "
                                "(build the optimiser after network.to_gpu())")
    clip = DeviceTable(2048, "clip_grad_norm", ("grads", "grad"), 1, hint="call it after network.to_gpu()")
    for entry in [(host,), (cpu,), (None,)]:
        with pytest.raises(RuntimeError) as e:
            clip.ensure([entry])
        assert str(e.value) == ("clip_grad_norm: grads must be contiguous fp32 device tensors (call it after "
                                "network.to_gpu())")
    assert opt.rows is None and opt.sig is None and opt.ntens == 0 and opt.blocks == 0
