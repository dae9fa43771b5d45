"""Whole steps through the layer API with every torch.empty allocation filled with NaN.

The layers size the BatchNorm partial-row buffers with torch.empty from a dk_*_rows() query and
hand them to a launch that computes its own row count; a fold then reduces every allocated row.
Where the two counts differ, rows the launch never wrote go into dgamma, dbeta, k12, mean and std
-- silently, since fresh device memory is usually zero or stale-but-finite.  With the poison below
any such read (and any other read of an output region a kernel does not write) turns the step's
results into NaN.  This catches every Python-side pairing of query and launch, not only the ones
tests/test_gpu_partial_rows.py lists."""
import numpy as np
import pytest
import torch

import tests.test_gpu_bf16 as bf16_tests
import tests.test_gpu_fold as fold_tests
from tests._convert import layer_to_oracle, rel_err

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


@pytest.fixture
def poisoned_empty(monkeypatch):
    """torch.empty / torch.empty_like return NaN-filled tensors (floating-point types) for the
    duration of the test."""
    counts = [0]
    empty, empty_like = torch.empty, torch.empty_like

    def poison(t):
        if t.is_floating_point():
            t.fill_(float("nan"))
            counts[0] += 1
        return t

    monkeypatch.setattr(torch, "empty", lambda *a, **k: poison(empty(*a, **k)))
    monkeypatch.setattr(torch, "empty_like", lambda *a, **k: poison(empty_like(*a, **k)))
    yield counts
    assert counts[0] > 0, "the step allocated nothing through torch.empty"


def host(t):
    return t.detach().float().cpu().numpy()


def test_bf16_bn_relu_depthwise_dgrad_partials(poisoned_empty, monkeypatch):
    """bf16 BatchNorm -> ReLU -> depthwise 3 x 3 (stride 1), fused: the depthwise dgrad
    (dk_dwconv_dgrad_ex_bf16) writes stage 1 of the BatchNorm's backward into part rows.  At
    H = W = 30 the bf16 launch writes 1 row where the fp32 query counts 3: sized by the fp32 query
    the buffer kept two unwritten rows, the armed fold was refused and the BatchNorm folded them
    into dgamma, dbeta and its dx."""
    from dorknet_amd import _hip
    from dorknet_amd.layers.activations import ReLu
    from dorknet_amd.layers.batch_norm import BatchNormLayer
    from dorknet_amd.layers.depthwise_convolution import DepthwiseConvLayer
    from dorknet_amd.network.feed_forward_network import FeedForwardNetwork
    monkeypatch.setenv("DORKNET_FUSE", "1")
    N, C, H = 2, 64, 30
    np.random.seed(3)
    torch.manual_seed(3)
    net = FeedForwardNetwork("advice")
    for l in (BatchNormLayer("bn", input_dimension=4, incoming_chans=C), ReLu("relu"),
              DepthwiseConvLayer("dw", filter_block_shape=(C, 3, 3), stride=1, padding=1, with_bias=False)):
        net.add_layer(l)
    net.to_gpu()
    bn = net.layers[0]
    bn.learned_params["gamma"].copy_(1.0 + 0.2 * torch.randn_like(bn.learned_params["gamma"]))
    bn.learned_params["beta"].copy_(0.1 * torch.randn_like(bn.learned_params["beta"]))
    olayers = [layer_to_oracle(l) for l in net.layers]
    parts = []
    orig = _hip.lib.dk_dwconv_dgrad_ex_bf16
    monkeypatch.setattr(_hip.lib, "dk_dwconv_dgrad_ex_bf16", lambda *a: parts.append(a[22]) or orig(*a))
    rng = np.random.RandomState(5)
    cl = torch.channels_last
    X = torch.as_tensor(rng.randn(N, C, H, H).astype(np.float32), device="cuda").to(BF16).contiguous(memory_format=cl)
    _, Y = net.forward(X, None)
    dY = torch.as_tensor(rng.randn(*Y.shape).astype(np.float32), device="cuda").to(BF16).contiguous(memory_format=cl)
    dX = net.backward(dY, input_grad=True)
    torch.cuda.synchronize()
    assert parts and all(parts), "the depthwise dgrad did not take the BatchNorm's partial rows"
    a = host(X).astype(np.float64)
    for o in olayers:
        a = o.forward(a)
    d = host(dY).astype(np.float64)
    for o in reversed(olayers):
        d = o.backward(d)
    got = {"dgamma": host(bn.grads["gamma"]), "dbeta": host(bn.grads["beta"]), "dX": host(dX), "Y": host(Y),
           "dw": host(net.layers[2].grads["weights"])}
    want = {"Y": a, "dX": d, "dgamma": olayers[0].grads["gamma"], "dbeta": olayers[0].grads["beta"],
            "dw": olayers[2].grads["weights"]}
    for k in got:
        assert np.isfinite(got[k]).all(), k
        e = rel_err(got[k].reshape(np.shape(want[k])), want[k])
        assert e <= 1e-2, (k, e)


def test_bf16_mobilenet_stack_step(poisoned_empty, monkeypatch):
    """The first two blocks of the MobileNet stack, 4 x 64 x 32 x 32 in bf16, fused: forward +
    backward within the bounds of test_mobilenet_stack_bf16_vs_oracle (a NaN fails every one)."""
    bf16_tests.test_mobilenet_stack_bf16_vs_oracle(monkeypatch, "1")


def test_f32_resnet_stem_res1_step(poisoned_empty, monkeypatch):
    """ResNet-18-depsep stem + res1 (4 x 3 x 65 x 65), in-launch folds on and off: outputs,
    gradients and running statistics agree as test_layer_path_folds_match_separate_launches
    requires (its comparison fails on any NaN)."""
    fold_tests.test_layer_path_folds_match_separate_launches(monkeypatch)
