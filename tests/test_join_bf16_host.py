"""Host-side checks of the bf16 residual join and the strided bf16 pointwise backward (no GPU): the type
guards run before any device work, the new entries are declared next to their fp32 twins with the same
arguments and have perfmodel entries, and the new row query answers on the host."""
import numpy as np
import pytest
import torch

from dorknet_amd import perfmodel
from dorknet_amd._hip import lib, parse_header

BF16 = torch.bfloat16


def test_mixed_storage_types_raise():
    from dorknet_amd.layers._bn_input import add_residual
    from dorknet_amd.layers.activations import ReLu
    from dorknet_amd.layers.residual_block import _add
    a = torch.zeros((1, 4, 2, 2), dtype=BF16)
    b = torch.zeros((1, 4, 2, 2), dtype=torch.float32)
    relu = ReLu("join")
    relu.is_on_gpu = True  # the guard is host logic: it runs before anything touches the device
    for A, B in ((a, b), (b, a)):
        with pytest.raises(ValueError, match="mixed storage types"):
            relu.forward_add(A, B)
        with pytest.raises(ValueError, match="mixed storage types"):
            _add(A, B)
        with pytest.raises(ValueError, match="mixed storage types"):
            add_residual(A, B)


def test_bf16_pointwise_backward_with_bias_still_refused():
    from dorknet_amd.layers.pointwise_convolution import PointwiseConvLayer
    np.random.seed(0)
    for stride in (1, 2):
        layer = PointwiseConvLayer("pw", stride=stride, filter_block_shape=(8, 4), with_bias=True)
        layer.is_on_gpu = True
        layer.X = torch.zeros((1, 4, 4, 4), dtype=BF16)
        layer._bn_in = None
        layer.out_hw = (4 // stride, 4 // stride)
        with pytest.raises(NotImplementedError, match="bias"):
            layer.backward(torch.zeros((1, 8, 4 // stride, 4 // stride), dtype=BF16))


def test_strided_dgrad_row_query():
    # the shapes of tests/test_gpu_join_bf16.py: positive, and monotone in the batch
    for K, C, OH, OW in ((128, 64, 7, 7), (64, 64, 12, 12)):
        rows = [lib.dk_pwconv_dgrad_bf16_stats_rows(N, OH, OW, K, C, 2) for N in (1, 2, 3, 8, 64)]
        assert rows[0] > 0 and all(a <= b for a, b in zip(rows, rows[1:])) and rows[-1] > rows[0], rows
        # the GEMM runs over the N x OH x OW lattice at every stride
        assert lib.dk_pwconv_dgrad_bf16_stats_rows(2, OH, OW, K, C, 1) == lib.dk_pwconv_dgrad_bf16_stats_rows(
            2, OH, OW, K, C, 2)


def test_new_entries_declared_like_their_fp32_twins():
    decls = parse_header()
    twins = {"dk_add_bf16": "dk_add_f32", "dk_bn_add_bf16": "dk_bn_add_f32",
             "dk_relu_bwd_bn_partial_bf16": "dk_relu_bwd_bn_partial_f64"}
    half = {"a", "b", "y", "dy", "x", "dx"}
    for h, f in twins.items():
        (rh, ph), (rf, pf) = decls[h], decls[f]
        assert rh == rf and [n for _, n in ph] == [n for _, n in pf], (h, f)
        for (th, n), (tf, _) in zip(ph, pf):
            assert th == (tf.replace("float", "uint16_t") if n in half and "*" in tf else tf), (h, n, th, tf)
    assert [n for _, n in decls["dk_pwconv_dgrad_bf16_stats_rows"][1]] == ["N", "OH", "OW", "K", "C", "stride"]


def test_new_entries_have_perfmodel_work():
    n, C = 256 * 56 * 56 * 64, 64
    args = (1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, n, C, 1, 1, 1, 0)
    f32, b16 = perfmodel.work("dk_bn_add_f32", args), perfmodel.work("dk_bn_add_bf16", args)
    # with a mask: 13 bytes per element in fp32, 7 in bf16; the same flops
    assert f32 == (9 * n, 13 * n) and b16 == (9 * n, 7 * n)
    assert perfmodel.work("dk_add_bf16", (1, 1, n, 1, 1, 0, 0)) == (n, 6 * n)
    assert perfmodel.work("dk_relu_bwd_bn_partial_bf16", (1, 1, 1, n // C, C, 0))[1] == 7 * n
    assert perfmodel.work("dk_pwconv_dgrad_bf16_stats_rows", (2, 7, 7, 128, 64, 2)) == (0, 0)
    for name in ("dk_add_bf16", "dk_bn_add_bf16", "dk_relu_bwd_bn_partial_bf16"):
        assert perfmodel.peak_tflops(name) == perfmodel.PEAK_F32_TFLOPS
