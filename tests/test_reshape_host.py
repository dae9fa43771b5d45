"""ReshapeLayer without a GPU: the rules (tests/_reshape_twin.py) against explicit index loops, the
layer's constructor validation / repr / alias import, the h5 + json round trip of a network holding a
ReshapeLayer, the chain executor's plan for a BatchNorm + ReLu in front of a flatten, and the entry
points' argument errors."""
import json
import os

import numpy as np
import pytest
import torch

from dorknet_amd import _hip
from dorknet_amd.layers.reshape import ReshapeLayer
from tests._reshape_twin import OReshape, flatten, unflatten


def test_twin_matches_index_loops():
    N, C, H, W = 2, 3, 2, 2
    X = np.arange(N * C * H * W, dtype=np.float32).reshape(N, C, H, W) * 0.5 - 3
    Y = flatten(X)
    assert Y.shape == (N, C * H * W) and Y.dtype == X.dtype
    for n in range(N):
        for c in range(C):
            for h in range(H):
                for w in range(W):
                    assert Y[n, c * H * W + h * W + w] == X[n, c, h, w]
    # a channels-last view of the same values flattens in the same (c, h, w) order, not in memory order
    Xcl = np.ascontiguousarray(X.transpose(0, 2, 3, 1)).transpose(0, 3, 1, 2)
    assert not Xcl.flags["C_CONTIGUOUS"] and np.array_equal(flatten(Xcl), Y)
    Z = unflatten(Y, (-1, C, H, W))
    assert Z.shape == X.shape and np.array_equal(Z, X)
    assert np.array_equal(unflatten(Y, (N, C, H, W)), X)
    o = OReshape("r", (-1, C, H, W), (-1, C * H * W))
    assert np.array_equal(o.forward(X.astype(np.float64)), Y.astype(np.float64))
    assert np.array_equal(o.backward(Y.astype(np.float64)), X.astype(np.float64))
    o = OReshape("r", (-1, 3, 2, 2), (-1, 2, 3, 2))
    assert np.array_equal(o.forward(X), X.reshape(N, 2, 3, 2)) and o.backward(X.reshape(N, 2, 3, 2)).shape == X.shape


def test_constructor_and_repr():
    l = ReshapeLayer("flat", (-1, 16, 7, 7), (-1, 16 * 49))
    assert l.layer_name == "flat" and l.is_on_gpu is False  # Layer.__init__ ran (the reference's never does)
    assert l.learned_params is None and l.grads is None
    assert l.input_shape == (-1, 16, 7, 7) and l.output_shape == (-1, 784)
    assert repr(l) == "ReshapeLayer(input_shape=(-1, 16, 7, 7), output_shape=(-1, 784))"
    assert l.accepts_bn_input is True
    assert ReshapeLayer("u", (-1, 784), (-1, 16, 7, 7)).accepts_bn_input is False   # unflatten
    assert ReshapeLayer("i", (-1, 4, 3, 3), (-1, 4, 3, 3)).accepts_bn_input is False  # identity
    assert ReshapeLayer("m", (-1, 4, 3, 3), (-1, 9, 2, 2)).accepts_bn_input is False  # 4-D -> 4-D
    assert ReshapeLayer("b", [8, 4, 3, 3], (-1, 36)).input_shape == (8, 4, 3, 3)      # a fixed batch, a list
    with pytest.raises(RuntimeError):
        l.forward(torch.zeros(1, 16, 7, 7))  # not on the GPU: there is no CPU path
    with pytest.raises(RuntimeError):
        l.backward(torch.zeros(1, 784))


@pytest.mark.parametrize("i,o", [
    ((-1, 16, 7, 7), (-1, 16 * 48)),     # mismatched products
    ((-1, 784), (-1, 16, 7, 6)),
    ((-1, 16, 7, 7), (-1, 16, -1)),      # -1 outside the batch slot
    ((-1, -1, 7, 7), (-1, 784)),
    ((4, 16, -1, 7), (4, 784)),
    ((-1, 16, 7, 7), (-1, 0)),           # a size below 1
    ((0, 16, 7, 7), (0, 784)),
    ((4, 16, 7, 7), (8, 784)),           # two different batch sizes
    ((-1, 16, 7.5, 7), (-1, 840)),       # not integers
    ((-1, 16, 7, 7), None),              # one shape without the other
    (784, (-1, 784)),
])
def test_constructor_validation(i, o):
    with pytest.raises(ValueError):
        ReshapeLayer("r", i, o)


def test_reference_alias_import():
    import dorknet_amd
    dorknet_amd.install_reference_aliases()
    from layers.reshape import ReshapeLayer as Aliased
    assert Aliased is ReshapeLayer


def test_plan_group_defers_bn_relu_into_a_flatten():
    from dorknet_amd.layers._chain import plan_group
    from dorknet_amd.layers.activations import ReLu
    from dorknet_amd.layers.batch_norm import BatchNormLayer
    bn, relu = BatchNormLayer("bn", incoming_chans=8), ReLu("relu")
    flat = ReshapeLayer("flat", (-1, 8, 3, 3), (-1, 72))
    group, mode = plan_group([bn, relu, flat], 0, True)
    assert mode == "defer" and group == (bn, relu)
    group, mode = plan_group([bn, flat], 0, True)
    assert mode == "defer" and group == (bn,)
    assert plan_group([bn, relu, flat], 0, False) == ((bn,), "single")  # DORKNET_FUSE=0
    # the other forms take no BNOut: the pair runs as one apply pass and the layer gets a tensor
    for other in (ReshapeLayer("i", (-1, 8, 3, 3), (-1, 8, 3, 3)), ReshapeLayer("m", (-1, 8, 3, 3), (-1, 2, 6, 6))):
        assert plan_group([bn, relu, other], 0, True)[1] == "pair"


def _h5_available():
    from dorknet_amd.network import checkpoint
    try:
        checkpoint._backend().File  # noqa: B018
        from dorknet_amd.network import _h5lite
        if checkpoint._backend() is _h5lite:
            _h5lite._load()
        return True
    except ImportError:
        return False


@pytest.mark.skipif(not _h5_available(), reason="neither h5py nor the HDF5 C library is available")
def test_network_with_a_reshape_round_trips(tmp_path):
    from dorknet_amd.network.feed_forward_network import FeedForwardNetwork
    from examples.mnist_lenet import MNISTLeNet
    np.random.seed(5)
    net = MNISTLeNet("lenet")
    net.layers.insert(0, ReshapeLayer("fixed", (32, 784), (32, 1, 28, 28)))  # a fixed batch: kept, like the -1
    rng = np.random.RandomState(6)
    for l in net.layers:
        if type(l).__name__ == "BatchNormLayer":
            shp = l._param_shape(l.incoming_chans)
            l.non_learned_params["running_mean"] = rng.standard_normal(shp).astype(np.float32)
            l.non_learned_params["running_std"] = rng.rand(*shp).astype(np.float32) + 0.5
    h5f, js = str(tmp_path / "w.h5"), str(tmp_path / "s.json")
    net.save_weights_to_h5(h5f)
    net.save_layer_structure_to_json(js)
    with open(js) as f:
        assert json.load(f)["flatten"] == "ReshapeLayer(input_shape=(-1, 64, 7, 7), output_shape=(-1, 3136))"
    fresh = FeedForwardNetwork("x")
    fresh.load_network_from_json_and_h5(js, h5f)
    assert [(type(l).__name__, l.layer_name) for l in fresh.layers] == [(type(l).__name__, l.layer_name)
                                                                        for l in net.layers]
    got = {l.layer_name: l for l in fresh.layers if isinstance(l, ReshapeLayer)}
    assert got["flatten"].input_shape == (-1, 64, 7, 7) and got["flatten"].output_shape == (-1, 3136)
    assert got["fixed"].input_shape == (32, 784) and got["fixed"].output_shape == (32, 1, 28, 28)
    assert all(type(v) is int for l in got.values() for v in l.input_shape + l.output_shape)
    assert got["flatten"].accepts_bn_input is True
    w0 = np.asarray(net.layers[-1].learned_params["weights"])
    assert np.array_equal(np.asarray(fresh.layers[-1].learned_params["weights"]), w0)
    with pytest.raises(ValueError):
        from dorknet_amd.network.checkpoint import open_h5
        with open_h5(str(tmp_path / "e.h5"), "w") as f:
            ReshapeLayer("unset").save_to_h5(f)


@pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="run __graft_entry__.build() first")
def test_argument_errors_without_a_device():
    import ctypes
    lib = _hip.lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)  # non-NULL, so that it is the sizes that are refused (before any launch)
    bn = (p, p, p, p, 1)
    for N, HW, C in [(0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (1, -3, 4), (1, 4, -4)]:
        for f in (lib.dk_flatten_fwd_f32, lib.dk_flatten_fwd_bf16, lib.dk_flatten_bwd_f32, lib.dk_flatten_bwd_bf16):
            with pytest.raises(_hip.HipError, match="bad arguments"):
                f(p, N, HW, C, p, None)
        for f in (lib.dk_flatten_fwd_bnx_f32, lib.dk_flatten_fwd_bnx_bf16):
            with pytest.raises(_hip.HipError, match="bad arguments"):
                f(p, N, HW, C, *bn, p, None)
    for f in (lib.dk_flatten_fwd_f32, lib.dk_flatten_bwd_bf16):  # a NULL tensor
        with pytest.raises(_hip.HipError, match="bad arguments"):
            f(None, 1, 4, 4, p, None)
        with pytest.raises(_hip.HipError, match="bad arguments"):
            f(p, 1, 4, 4, None, None)
    with pytest.raises(_hip.HipError, match="bad arguments"):
        lib.dk_flatten_fwd_bnx_f32(p, 1, 4, 4, p, None, p, p, 1, p, None)  # a NULL BN parameter
