"""DropoutLayer without a GPU: the mask rule (tests/_dropout_twin.py) against the pinned vectors, its
statistics, the layer's constructor / repr / validation / alias import, the h5 + json round trip of a
network holding the layer (alone and inside a ResidualBlock), the entry points' argument errors, and
DataParallel's lane assignment over a two-process gloo group."""
import json
import os
import socket

import numpy as np
import pytest
import torch

from dorknet_amd import _hip
from dorknet_amd.layers.dropout import DropoutLayer
from tests._dropout_twin import (ODropout, bf16_round, dropout_bwd, dropout_fwd, keep_mask, philox4x32_10, scale_of,
                                 storage_mask, threshold)


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


def test_philox_known_answers():
    assert _hex(philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    f = 0xffffffff
    assert _hex(philox4x32_10((f, f, f, f), (f, f))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344),
                              (0xa4093822, 0x299f31d0))) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    # arrays of counters give the same words as one call each
    c0 = np.arange(5, dtype=np.uint64)
    many = philox4x32_10((c0, 0, 7, 1), (3, 0))
    for i in range(5):
        assert np.array_equal(many[:, i], philox4x32_10((i, 0, 7, 1), (3, 0)))


def test_pinned_keep_bits_and_counts():
    """Seed 1, step 0, lane 0, p 0.5.  Of the first 4096 elements the rule keeps 2061, a share of
    0.50317 -- the share the rule's statement gives; the count of 2062 quoted beside it there is 0.50342
    and does not follow from the rule (a plain-integer restatement of the generator counts 2061 too)."""
    assert keep_mask(16, 0.5, 1, 0, 0).astype(int).tolist() == [0, 1, 0, 1, 0, 1, 1, 1, 0, 1, 1, 1, 0, 0, 0, 1]
    kept = int(keep_mask(4096, 0.5, 1, 0, 0).sum())
    assert kept == 2061 and round(kept / 4096, 5) == 0.50317
    # a buffer that crosses the 32-bit boundary of the block index: the upper counter word is used
    far = keep_mask(64, 0.5, 1, 0, 0, first_index=2 ** 35 - 32)
    assert int(far.sum()) == 37
    assert not np.array_equal(far[32:], keep_mask(32, 0.5, 1, 0, 0))  # block 2^32 is not block 0
    # a mask is a window of the one stream of its (seed, step, lane)
    assert np.array_equal(keep_mask(4096, 0.5, 1, 0, 0)[64:200], keep_mask(136, 0.5, 1, 0, 0, first_index=64))
    for bad in (-8, 4, 9):
        with pytest.raises(ValueError):
            keep_mask(8, 0.5, 1, 0, 0, first_index=bad)


@pytest.mark.parametrize("p", [0.25, 0.5, 0.9])
def test_kept_share(p):
    """n = 4096, seeds 1..8, steps 0..3: the kept share lies within 4 standard deviations of a
    binomial share, 4 * sqrt(p (1 - p) / n), of the probability realised, 1 - T / 65536."""
    n, T = 4096, threshold(p)
    bound = 4.0 * np.sqrt(p * (1.0 - p) / n)
    worst = 0.0
    for seed in range(1, 9):
        for step in range(4):
            worst = max(worst, abs(float(keep_mask(n, p, seed, step, 0).mean()) - (1.0 - T / 65536.0)))
    print("p {}: worst deviation {:.4f}, bound {:.4f}".format(p, worst, bound))
    assert worst <= bound


def test_masks_depend_on_every_argument():
    base = keep_mask(4096, 0.5, 3, 5, 0)
    assert np.array_equal(base, keep_mask(4096, 0.5, 3, 5, 0))
    for other in (keep_mask(4096, 0.5, 4, 5, 0), keep_mask(4096, 0.5, 3, 6, 0), keep_mask(4096, 0.5, 3, 5, 1),
                  keep_mask(4096, 0.5, 3 + 2 ** 32, 5, 0)):  # (the seed's upper word is the second key word)
        assert 0.4 < float((other != base).mean()) < 0.6  # independent masks disagree on about half
    # only the lower 32 bits of the step enter the counter
    assert np.array_equal(base, keep_mask(4096, 0.5, 3, 5 + 2 ** 32, 0))
    # a larger p drops a superset
    assert not (keep_mask(4096, 0.9, 3, 5, 0) & ~base).any()


def test_threshold_and_scale():
    assert threshold(0) == 0 and threshold(0.5) == 32768 and threshold(0.9) == 58982 and threshold(0.99999) == 65535
    assert threshold(1e-6) == 0
    assert scale_of(0) == np.float32(1.0) and scale_of(0.5) == np.float32(2.0)
    assert scale_of(0.9) == np.float32(65536.0 / (65536 - 58982))
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            threshold(bad)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_forward_backward_arithmetic():
    rng = np.random.RandomState(0)
    x = rng.randn(300).astype(np.float32)
    x[:4] = [np.inf, -np.inf, -0.0, 1e-42]
    # p = 0 keeps everything and returns the input bits
    assert np.array_equal(_bits(dropout_fwd(x, 0.0, 9, 2)), _bits(x))
    xb = bf16_round(x)
    assert np.array_equal(_bits(dropout_fwd(xb, 0.0, 9, 2, storage="bf16")), _bits(xb))
    keep = keep_mask(300, 0.9, 9, 2, 0)
    y = dropout_fwd(x, 0.9, 9, 2)
    assert np.array_equal(_bits(y[keep]), _bits(x[keep] * scale_of(0.9)))
    assert not _bits(y[~keep]).any()  # +0.0, not -0.0
    assert np.array_equal(_bits(dropout_bwd(x, 0.9, 9, 2)), _bits(y))  # the same rule over dy
    # dropped NaNs and infinities become +0.0, kept ones stay
    bad = np.full(300, np.nan, dtype=np.float32)
    bad[1::2] = -np.inf
    yb = dropout_fwd(bad, 0.5, 9, 2)
    k5 = keep_mask(300, 0.5, 9, 2, 0)
    assert not _bits(yb[~k5]).any() and 100 < int((~k5).sum()) < 200
    assert (np.isnan(yb[k5]) | np.isinf(yb[k5])).all()
    # bf16: the fp32 product is rounded once, to nearest even
    yb16 = dropout_fwd(xb, 0.9, 9, 2, storage="bf16")
    want = torch.as_tensor(xb[keep] * scale_of(0.9)).to(torch.bfloat16).float().numpy()
    assert np.array_equal(_bits(yb16[keep]), _bits(want)) and not _bits(yb16[~keep]).any()
    assert np.array_equal(_bits(bf16_round(np.float32([1.00390625, 1.01171875]))), _bits(np.float32([1.0, 1.015625])))


def test_twin_layer_steps_and_storage_order():
    X = np.random.RandomState(1).randn(2, 6, 5, 5)
    o = ODropout("d", 0.5, seed=11)
    Y0 = o.forward(X)
    assert o.step == 1 and Y0.dtype == np.float64
    keep0 = storage_mask(X.shape, 0.5, 11, 0)
    # NHWC storage order: element (n, c, h, w) has index ((n * H + h) * W + w) * C + c
    flat = keep_mask(X.size, 0.5, 11, 0, 0)
    assert keep0[1, 4, 2, 3] == flat[((1 * 5 + 2) * 5 + 3) * 6 + 4]
    assert np.array_equal(Y0, np.where(keep0, X * 2.0, 0.0))
    dY = np.ones_like(X)
    assert np.array_equal(o.backward(dY), np.where(keep0, 2.0, 0.0))
    assert np.array_equal(o.backward(dY), np.where(keep0, 2.0, 0.0))  # the recorded step, twice
    Y1 = o.forward(X)
    assert o.step == 2 and not np.array_equal(Y1 != 0, Y0 != 0)
    assert o.forward(X, test_mode=True) is X and o.step == 2
    R = np.random.RandomState(2).randn(4, 24)
    assert np.array_equal(ODropout("r", 0.25, 3).forward(R) != 0, keep_mask(96, 0.25, 3, 0, 0).reshape(4, 24))


def test_constructor_repr_and_validation():
    l = DropoutLayer("drop")
    assert l.layer_name == "drop" and l.drop_prob == 0.5 and l.seed == 0 and l.step == 0 and l.lane == 0
    assert l.is_on_gpu is False and l.learned_params is None and l.grads is None
    assert repr(l) == "DropoutLayer(drop, drop_prob=0.5)"
    assert repr(DropoutLayer("d", 0.25, seed=7)) == "DropoutLayer(d, drop_prob=0.25)"
    assert DropoutLayer.accepts_bn_input is True
    assert DropoutLayer("d", 0).threshold == 0 and DropoutLayer("d", 0.9).threshold == threshold(0.9)
    assert DropoutLayer("d", np.float32(0.5), seed=np.int64(2 ** 63 - 1)).seed == 2 ** 63 - 1
    for bad in (-0.01, 1.0, 2, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            DropoutLayer("d", bad)
    for bad in ("0.5", None, [0.5], True):
        with pytest.raises((TypeError, ValueError)):
            DropoutLayer("d", bad)
    for bad in (-1, 2 ** 63, 1.5, "3", None, True):
        with pytest.raises((TypeError, ValueError)):
            DropoutLayer("d", 0.5, seed=bad)
    x = torch.zeros(2, 3)
    assert l.forward(x, test_mode=True) is x and l.step == 0  # the identity, on any device
    with pytest.raises(RuntimeError):
        l.forward(x)  # not on the GPU: there is no CPU path
    with pytest.raises(RuntimeError):
        l.backward(x)


def test_reference_alias_import():
    import dorknet_amd
    dorknet_amd.install_reference_aliases()
    from layers.dropout import DropoutLayer as Aliased
    assert Aliased is DropoutLayer


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
def test_network_with_dropout_round_trips(tmp_path):
    """A dense head with a dropout, and a ResidualBlock whose layer_list holds one: drop_prob, seed and
    step come back, so the reloaded network draws the mask of step k next."""
    from dorknet_amd.layers.activations import ReLu
    from dorknet_amd.layers.dense_layer import DenseLayer
    from dorknet_amd.layers.losses import SoftmaxWithCrossEntropy
    from dorknet_amd.layers.pointwise_convolution import PointwiseConvLayer
    from dorknet_amd.layers.residual_block import ResidualBlock
    from dorknet_amd.network.feed_forward_network import FeedForwardNetwork
    np.random.seed(5)
    net = FeedForwardNetwork("dropped")
    inner = DropoutLayer("block_drop", 0.25, seed=2 ** 40 + 3)
    inner.step = 2 ** 33 + 1
    net.add_layer(ResidualBlock("block", [PointwiseConvLayer("pw", filter_block_shape=(8, 8), with_bias=False),
                                          inner], post_skip_activation=ReLu("block_relu")))
    net.add_layer(DenseLayer("dense_1", incoming_chans=24, output_dim=16))
    net.add_layer(ReLu("relu"))
    head = DropoutLayer("drop", 0.9, seed=77)
    head.step = 12
    net.add_layer(head)
    net.add_layer(DenseLayer("dense_2", incoming_chans=16, output_dim=5))
    net.set_loss_layer(SoftmaxWithCrossEntropy("softmax"))
    h5f, js = str(tmp_path / "w.h5"), str(tmp_path / "s.json")
    net.save_weights_to_h5(h5f)
    net.save_layer_structure_to_json(js)
    with open(js) as f:
        assert json.load(f)["drop"] == "DropoutLayer(drop, drop_prob=0.9)"
    fresh = FeedForwardNetwork("x")
    fresh.load_network_from_json_and_h5(js, h5f)
    assert [(type(l).__name__, l.layer_name) for l in fresh.layers] == [(type(l).__name__, l.layer_name)
                                                                        for l in net.layers]
    got = fresh.layers[3]
    assert isinstance(got, DropoutLayer) and (got.drop_prob, got.seed, got.step, got.lane) == (0.9, 77, 12, 0)
    assert type(got.seed) is int and type(got.step) is int and type(got.drop_prob) is float
    sub = fresh.layers[0].layer_list[1]
    assert isinstance(sub, DropoutLayer) and sub.layer_name == "block_drop"
    assert (sub.drop_prob, sub.seed, sub.step) == (0.25, 2 ** 40 + 3, 2 ** 33 + 1)
    assert np.array_equal(np.asarray(fresh.layers[1].learned_params["weights"]),
                          np.asarray(net.layers[1].learned_params["weights"]))
    # loading validates as the constructor does
    from dorknet_amd.network.checkpoint import open_h5
    with open_h5(h5f, "r+") as f:
        f["drop/layer_info"].attrs["drop_prob"] = 1.5
    with pytest.raises(ValueError):
        FeedForwardNetwork("y").load_network_from_json_and_h5(js, h5f)
    with open_h5(h5f, "r+") as f:
        f["drop/layer_info"].attrs["drop_prob"] = 0.5
        f["drop/layer_info"].attrs["step"] = np.int64(-1)
    with pytest.raises(ValueError):
        FeedForwardNetwork("z").load_network_from_json_and_h5(js, h5f)


@pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="run __graft_entry__.build() first")
def test_argument_errors_without_a_device():
    import ctypes
    lib = _hip.lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)  # non-NULL, so that it is the scalars that are refused (before any launch)
    bn = (p, p, p, p, 1)
    plain = [lib.dk_dropout_fwd_f32, lib.dk_dropout_fwd_bf16, lib.dk_dropout_bwd_f32, lib.dk_dropout_bwd_bf16]
    bnx = [lib.dk_dropout_fwd_bnx_f32, lib.dk_dropout_fwd_bnx_bf16]
    # (n, threshold, seed, step, lane, first_index)
    bad = [(0, 100, 1, 0, 0, 0), (-8, 100, 1, 0, 0, 0), (8, -1, 1, 0, 0, 0), (8, 65536, 1, 0, 0, 0),
           (8, 100, -1, 0, 0, 0), (8, 100, 1, -1, 0, 0), (8, 100, 1, 0, -1, 0), (8, 100, 1, 0, 0, -8),
           (8, 100, 1, 0, 0, 4), (8, 100, 1, 0, 0, 2 ** 63 - 8)]
    for n, T, seed, step, lane, first in bad:
        for f in plain:
            with pytest.raises(_hip.HipError, match="bad arguments"):
                f(p, n, T, seed, step, lane, first, p, None)
        for f in bnx:
            with pytest.raises(_hip.HipError, match="bad arguments"):
                f(p, n, T, seed, step, lane, first, 4, *bn, p, None)
    ok = (8, 100, 1, 0, 0, 0)
    for f in plain:  # a NULL tensor
        for x, y in ((None, p), (p, None)):
            with pytest.raises(_hip.HipError, match="bad arguments"):
                f(x, *ok, y, None)
    for f in bnx:
        for C in (0, -4):
            with pytest.raises(_hip.HipError, match="bad arguments"):
                f(p, *ok, C, *bn, p, None)
        for i in range(4):  # a NULL parameter
            holed = tuple(None if j == i else v for j, v in enumerate(bn))
            with pytest.raises(_hip.HipError, match="bad arguments"):
                f(p, *ok, 4, *holed, p, None)
        for x, y in ((None, p), (p, None)):
            with pytest.raises(_hip.HipError, match="bad arguments"):
                f(x, *ok, 4, *bn, y, None)


# ---- DataParallel sets the lane to the rank ------------------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


class _Net:
    """A network with no GPU work: one dense layer's worth of parameters on the host, a dropout at the
    top level and one inside a residual block."""

    def __init__(self):
        from dorknet_amd.layers.residual_block import ResidualBlock
        self.top = DropoutLayer("top", 0.5, seed=5)
        self.inner = DropoutLayer("inner", 0.25, seed=5)
        self.layers = [self.top, ResidualBlock("block", [self.inner])]
        self.loss_layer = None


def _lane_worker(rank, world, port, q):
    try:
        import torch.distributed as dist
        from dorknet_amd.parallel import DataParallel
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        net = _Net()
        assert net.top.lane == 0 and net.inner.lane == 0
        DataParallel(net, device=torch.device("cpu"))
        assert net.top.lane == rank and net.inner.lane == rank, (rank, net.top.lane, net.inner.lane)
        assert net.top.step == 0 and net.top.seed == 5
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception:  # pragma: no cover - reported to the parent
        import traceback
        q.put((rank, traceback.format_exc()))
        raise


def test_data_parallel_sets_lane_to_rank_gloo_world2():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_lane_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert results == {0: "ok", 1: "ok"}, results
    # and the ranks' masks differ while each stays reproducible
    assert not np.array_equal(keep_mask(4096, 0.5, 5, 0, 0), keep_mask(4096, 0.5, 5, 0, 1))
