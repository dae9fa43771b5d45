"""MaxPoolLayer without a GPU: the rules (tests/_maxpool_twin.py) against torch's CPU max_pool2d and
its autograd, a case spelled out by hand, the layer's constructor / repr / alias import, the h5 +
json round trip of a network holding a pool, and the entry points' argument errors."""
import json
import os

import numpy as np
import pytest
import torch

from dorknet_amd import _hip
from dorknet_amd.layers.pooling import MaxPoolLayer
from tests._maxpool_twin import OMaxPool, pool_bwd, pool_fwd

# (N, C, H, W, stride): scalar channels with a remainder row and column; stride 3; one window per
# quadrant; the stride-1 identity; C = 68
TIED_CASES = [(2, 3, 7, 9, 2), (2, 5, 10, 11, 3), (1, 4, 8, 8, 4), (2, 8, 6, 6, 1), (2, 68, 14, 14, 2)]


@pytest.mark.parametrize("case", TIED_CASES)
def test_twin_matches_torch_cpu_bitwise(case):
    N, C, H, W, s = case
    rng = np.random.RandomState(sum(case))
    X = rng.randint(-1, 3, size=(N, C, H, W)).astype(np.float32)  # {-1, 0, 1, 2}: ties dominate
    Y, idx = pool_fwd(X, s)
    dY = rng.randn(*Y.shape).astype(np.float32)
    dX = pool_bwd(idx, dY, s, H, W)
    xt = torch.tensor(X, requires_grad=True)
    yt = torch.nn.functional.max_pool2d(xt, s, s)
    yt.backward(torch.tensor(dY))
    assert Y.dtype == np.float32 and idx.dtype == np.uint8 and dX.dtype == np.float32
    assert np.array_equal(Y.view(np.int32), yt.detach().numpy().view(np.int32))
    assert np.array_equal(dX.view(np.int32), xt.grad.numpy().view(np.int32))
    if s > 1:
        from tests._maxpool_twin import windows
        v = windows(X, s)
        tied = ((v == Y[..., None]).sum(-1) > 1).mean()
        assert tied > 0.3, tied  # the case really exercises the tie rule


def test_hand_written_case():
    X = np.array([[[[1, 3, 2, 2, 9],
                    [0, 3, 2, 2, 9],
                    [5, 4, 0, 1, 9],
                    [4, 6, -1, 7, 9]]]], dtype=np.float32)
    Y, idx = pool_fwd(X, 2)
    # window (0, 0) = [1, 3, 0, 3]: the maximum 3 sits at k = 1 and k = 3, the first wins;
    # window (0, 1) is all 2: k = 0; the column of 9s fills no window
    assert Y.tolist() == [[[[3, 2], [6, 7]]]]
    assert idx.tolist() == [[[[1, 0], [3, 3]]]]
    dY = np.array([[[[10, 20], [30, 40]]]], dtype=np.float32)
    dX = pool_bwd(idx, dY, 2, 4, 5)
    assert dX.tolist() == [[[[0, 10, 20, 0, 0],
                             [0, 0, 0, 0, 0],
                             [0, 0, 0, 0, 0],
                             [0, 30, 0, 40, 0]]]]


def test_twin_layer_replay():
    X = np.array([[[[1, 3], [0, 3]]]], dtype=np.float64)
    o = OMaxPool("p", 2)
    assert o.forward(X).tolist() == [[[[3]]]] and o.idx.tolist() == [[[[1]]]]
    o.replay = np.array([[[[3]]]], dtype=np.uint8)
    assert o.forward(X).tolist() == [[[[3]]]]
    assert o.idx.tolist() == [[[[3]]]] and o.own_idx.tolist() == [[[[1]]]] and o.replay is None
    assert o.backward(np.array([[[[5.0]]]])).tolist() == [[[[0, 0], [0, 5]]]]
    with pytest.raises(ValueError):
        pool_fwd(np.zeros((1, 1, 3, 1)), 2)  # OW == 0


def test_constructor_repr_and_stride_validation():
    l = MaxPoolLayer("pool")
    assert l.layer_name == "pool" and l.stride == 2 and l.is_on_gpu is False  # Layer.__init__ ran
    assert l.learned_params is None and l.grads is None
    assert repr(l) == "MaxPoolLayer(stride=2)"
    assert repr(MaxPoolLayer("p", input_shape=(1, 2, 3, 4), stride=3)) == "MaxPoolLayer(stride=3)"
    assert MaxPoolLayer("p", None, 16).stride == 16 and MaxPoolLayer("p", stride=1).stride == 1
    assert MaxPoolLayer.accepts_bn_input is True
    for bad in (0, 17, -2, 2.5, None, "2"):
        with pytest.raises((ValueError, TypeError)):
            MaxPoolLayer("p", stride=bad)
    with pytest.raises(RuntimeError):
        l.forward(torch.zeros(1, 1, 2, 2))  # not on the GPU: there is no CPU path


def test_reference_alias_import():
    import dorknet_amd
    dorknet_amd.install_reference_aliases()
    from layers.pooling import MaxPoolLayer as Aliased
    assert Aliased is MaxPoolLayer


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
def test_network_with_pools_round_trips(tmp_path):
    from dorknet_amd.network.feed_forward_network import FeedForwardNetwork
    from examples.mnist_maxpool import MNISTMaxPoolNet
    np.random.seed(5)
    net = MNISTMaxPoolNet("pooled")
    net.layers[[l.layer_name for l in net.layers].index("pool_2")].stride = 3
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
        assert json.load(f)["pool_1"] == "MaxPoolLayer(stride=2)"
    fresh = FeedForwardNetwork("x")
    fresh.load_network_from_json_and_h5(js, h5f)
    assert [(type(l).__name__, l.layer_name) for l in fresh.layers] == [(type(l).__name__, l.layer_name)
                                                                        for l in net.layers]
    pools = [l for l in fresh.layers if isinstance(l, MaxPoolLayer)]
    assert [(p.layer_name, p.stride) for p in pools] == [("pool_1", 2), ("pool_2", 3)]
    assert all(type(p.stride) is int for p in pools)
    w0 = np.asarray(net.layers[0].learned_params["weights"])
    assert np.array_equal(np.asarray(fresh.layers[0].learned_params["weights"]), w0)


@pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="run __graft_entry__.build() first")
def test_argument_errors_without_a_device():
    import ctypes
    lib = _hip.lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)  # non-NULL, so that it is the sizes that are refused (before any launch)
    bn = (p, p, p, p, 1)
    # (N, H, W, C, stride): stride outside 1..16, a size below 1, OH == 0, OW == 0
    for N, H, W, C, s in [(1, 4, 4, 4, 0), (1, 4, 4, 4, 17), (1, 4, 4, 4, -1), (0, 4, 4, 4, 2), (1, 0, 4, 4, 2),
                          (1, 4, 0, 4, 2), (1, 4, 4, 0, 2), (1, 1, 4, 4, 2), (1, 33, 5, 12, 16)]:
        for fwd in (lib.dk_maxpool_fwd_f32, lib.dk_maxpool_fwd_bf16):
            with pytest.raises(_hip.HipError, match="bad arguments"):
                fwd(p, N, H, W, C, s, p, p, None)
        for fwd in (lib.dk_maxpool_fwd_bnx_f32, lib.dk_maxpool_fwd_bnx_bf16):
            with pytest.raises(_hip.HipError, match="bad arguments"):
                fwd(p, N, H, W, C, s, *bn, p, p, None)
        for bwd in (lib.dk_maxpool_bwd_f32, lib.dk_maxpool_bwd_bf16):
            with pytest.raises(_hip.HipError, match="bad arguments"):
                bwd(p, p, N, H, W, C, s, p, None)
