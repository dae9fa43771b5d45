"""SGD and RMSProp (reference: optimisers/SGD.py, optimisers/RMSProp.py) and the optimiser state
file, without a GPU: parameter discovery, the reference's import lines, signatures, the
DataParallel flag handshake, the numpy twins against their fp64 versions, the C entries' argument
checks and the state file's refusals."""
import os

import numpy as np
import pytest

import dorknet_amd
from dorknet_amd import _hip
from dorknet_amd.network import checkpoint
from dorknet_amd.optimisers.RMSProp import RMSProp
from dorknet_amd.optimisers.SGD import SGD
from dorknet_amd.optimisers.SGDMomentum import SGDMomentum
from examples.resnet18_depsep import ResNet18
from tests import _optim_twin as twin

try:
    checkpoint._backend().File  # noqa: B018
    from dorknet_amd.network import _h5lite
    if checkpoint._backend() is _h5lite:
        _h5lite._load()
    HAVE_H5 = True
except ImportError:  # pragma: no cover - environment dependent
    HAVE_H5 = False

needs_h5 = pytest.mark.skipif(not HAVE_H5, reason="neither h5py nor the HDF5 C library is available")

NEW = [(SGD, (0.05,)), (RMSProp, (0.05, 0.9))]
IDS = ["SGD", "RMSProp"]


def _counts(opt):
    ntens = sum(len(l.learned_params) for l in opt.learnable_layers)
    nparam = sum(v.size for l in opt.learnable_layers for v in l.learned_params.values())
    return ntens, nparam


@pytest.mark.parametrize("cls,args", NEW, ids=IDS)
def test_discovery_is_sgd_momentum_s(cls, args):
    np.random.seed(0)
    net = ResNet18("r18")
    ref = SGDMomentum(net, 0.05, 0.9)
    opt = cls(net, *args)
    assert [id(l) for l in opt.learnable_layers] == [id(l) for l in ref.learnable_layers]
    assert not any(l.layer_name.endswith("_pw_skip") for l in opt.learnable_layers)
    assert _counts(opt) == (104, 1336312)
    ref = SGDMomentum(net, 0.05, 0.9, update_skip_projections=True)
    opt = cls(net, *args, update_skip_projections=True)
    assert [id(l) for l in opt.learnable_layers] == [id(l) for l in ref.learnable_layers]
    assert sum(l.layer_name.endswith("_pw_skip") for l in opt.learnable_layers) == 3
    assert _counts(opt) == (107, 1336312 + 172032)


@pytest.mark.parametrize("cls,args", NEW, ids=IDS)
def test_layers_inside_residual_blocks_are_updated(cls, args):
    """The reference's SGD.py:8-11 / RMSProp.py:12-15 append `layer` (the block, learned_params None)
    where SGDMomentum.py uses `l`: nothing inside a block would ever move.  Here every learnable
    layer of every block's layer_list is listed, once, and no block itself is."""
    np.random.seed(0)
    net = ResNet18("r18")
    opt = cls(net, *args)
    listed = [id(l) for l in opt.learnable_layers]
    blocks = [l for l in net.layers if hasattr(l, "layer_list")]
    assert len(blocks) == 8
    inner = [l for b in blocks for l in b.layer_list if l.learned_params is not None]
    assert len(inner) == 8 * 8  # per block: 2 x (depthwise, BN, pointwise, BN)
    assert all(listed.count(id(l)) == 1 for l in inner)
    assert not any(id(b) in listed for b in blocks)


def test_reference_import_lines():
    dorknet_amd.install_reference_aliases()
    from optimisers.RMSProp import RMSProp as R2
    from optimisers.SGD import SGD as S2
    assert S2 is SGD and R2 is RMSProp


def test_signatures_and_learning_rate():
    np.random.seed(0)
    net = ResNet18("r18")
    sgd = SGD(net, 0.1)
    rms = RMSProp(net, 0.1, 0.95)
    kw = RMSProp(network=net, learning_rate=0.2, decay_rate=0.5)
    assert SGD(network=net, learning_rate=0.3).learning_rate == 0.3
    assert (kw.learning_rate, kw.decay_rate) == (0.2, 0.5)
    assert sgd.network is net and rms.network is net
    assert (sgd.learning_rate, rms.learning_rate, rms.decay_rate) == (0.1, 0.1, 0.95)
    for opt in (sgd, rms):
        opt.set_learning_rate(0.5)
        assert opt.learning_rate == 0.5
        opt.multiply_learning_rate(0.1)
        assert opt.learning_rate == 0.5 * 0.1
    assert set(rms.grad_cache) == set(rms.learnable_layers)
    for layer in rms.learnable_layers:
        assert rms.grad_cache[layer].keys() == layer.grads.keys()
        for k, g in layer.grads.items():
            c = np.asarray(rms.grad_cache[layer][k])
            assert c.shape == np.shape(g) and c.dtype == np.asarray(g).dtype and not c.any()
    assert not hasattr(sgd, "grad_cache")  # as in the reference


@pytest.mark.parametrize("cls,args", NEW, ids=IDS)
def test_data_parallel_handshake(cls, args):
    np.random.seed(0)
    net = ResNet18("r18")
    net._dp_update_skip_projections = True
    with pytest.raises(ValueError, match="update_skip_projections"):
        cls(net, *args)
    with pytest.raises(ValueError, match="update_skip_projections"):
        cls(net, *args, update_skip_projections=False)
    opt = cls(net, *args, update_skip_projections=True)
    assert net._opt_update_skip_projections is True and opt.update_skip_projections is True
    net._dp_update_skip_projections = False
    with pytest.raises(ValueError, match="update_skip_projections"):
        cls(net, *args, update_skip_projections=True)
    cls(net, *args)
    assert net._opt_update_skip_projections is False


@pytest.mark.parametrize("cls,args", NEW, ids=IDS)
def test_host_parameters_are_refused(cls, args):
    """The RuntimeError SGDMomentum raises: the table takes contiguous fp32 device tensors only."""
    np.random.seed(0)
    net = ResNet18("r18")
    with pytest.raises(RuntimeError, match="to_gpu"):
        cls(net, *args).update_weights()
    with pytest.raises(RuntimeError, match="to_gpu"):
        SGDMomentum(net, 0.1, 0.9).update_weights()


def _ulps(got32, want64, at):
    """|got - want| in fp32 ulps at the magnitude `at`."""
    return np.abs(got32.astype(np.float64) - want64) / np.spacing(np.abs(at).astype(np.float32)).astype(np.float64)


def test_twins_agree_with_their_fp64_versions():
    """Each fp32 result is a chain of at most six correctly rounded operations, so it lies within
    4 fp32 ulp of the fp64 evaluation.  c: at most four roundings on any path to the sum (the
    scalar, its product, [the square,] the sum), each at most one ulp of c.  W: |W| in [1, 2) and
    |d| <= lr / sqrt(1 - decay) < 1/16, so the roundings inside d weigh under 1/16 ulp of W each and
    the final sum adds half an ulp."""
    rng = np.random.default_rng(7)
    n = 20000
    W = (rng.uniform(1, 2, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    g = rng.standard_normal(n).astype(np.float32)
    lr, decay = 0.01, 0.9
    W32 = twin.sgd_update(W, g, lr)
    assert W32.dtype == np.float32
    assert _ulps(W32, twin.sgd_update_f64(W, g, lr), W32).max() <= 4
    for c in (np.zeros(n, np.float32), (rng.standard_normal(n) ** 2).astype(np.float32)):
        W32, c32 = twin.rmsprop_update(W, g, c, lr, decay)
        W64, c64 = twin.rmsprop_update_f64(W, g, c, lr, decay)
        assert W32.dtype == np.float32 and c32.dtype == np.float32
        assert _ulps(c32, c64, c32).max() <= 4
        assert _ulps(W32, W64, W32).max() <= 4
    # the written order and the scalars' single rounding, on values where they show
    W1, c1 = twin.rmsprop_update(np.float32([1.0]), np.float32([3.0]), np.float32([0.5]), 0.1, 0.9)
    f = np.float32
    c_want = f(0.9) * f(0.5) + f(1 - 0.9) * (f(3.0) * f(3.0))
    assert c1[0] == c_want and f(1 - 0.9) != f(1) - f(0.9)
    assert W1[0] == f(1.0) + (f(-0.1) * f(3.0)) / np.sqrt(c_want + f(1e-5))


def test_twin_keeps_denormals_after_a_fast_math_library_is_loaded():
    """The oracle's C library is linked with -ffast-math (the reference's flags) and switches the thread
    that loads it to flush-to-zero; the fp32 twins evaluate under the default environment regardless
    and put the previous one back."""
    import ctypes
    lib = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "lib",
                       "libdorknet_oracle.so")
    if os.path.exists(lib):
        ctypes.CDLL(lib)
    mode = twin.host_keeps_denormals()
    W, g = np.float32([1.0, 2.0]), np.float32([1e-20, -1e-20])
    W2, c2 = twin.rmsprop_update(W, g, np.zeros(2, np.float32), 0.01, 0.9)
    # fp32(0.1) * fp32(1e-20)^2 = 1.0e-41 = 7136 * 2^-149
    assert c2.view(np.uint32).tolist() == [7136, 7136] and W2.tolist() == [1.0, 2.0]
    assert twin.host_keeps_denormals() == mode


@pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="run __graft_entry__.build() first")
def test_argument_errors_without_a_device():
    import ctypes
    lib = _hip.lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    for table, ntens, blocks in [(None, 1, 1), (p, -1, 1), (p, 1, -1)]:
        with pytest.raises(_hip.HipError, match="bad arguments"):
            lib.dk_sgd_multi_f32(table, ntens, blocks, 0.1, None)
        with pytest.raises(_hip.HipError, match="bad arguments"):
            lib.dk_rmsprop_multi_f32(table, ntens, blocks, 0.1, 0.9, 0.1, 1e-5, None)
    assert lib.dk_sgd_multi_f32(None, 0, 0, 0.1, None) == 0  # nothing to do
    assert lib.dk_rmsprop_multi_f32(None, 0, 0, 0.1, 0.9, 0.1, 1e-5, None) == 0
    assert lib.dk_abi_version() == 1


@pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="run __graft_entry__.build() first")
def test_momentum_argument_errors_without_a_device():
    """dk_sgd_momentum_multi_f32 refuses what its siblings refuse, before any launch."""
    import ctypes
    lib = _hip.lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    for table, ntens, blocks in [(None, 1, 1), (p, -1, 1), (p, 1, -1), (p, 1, 1 << 31)]:
        with pytest.raises(_hip.HipError, match="bad arguments"):
            lib.dk_sgd_momentum_multi_f32(table, ntens, blocks, 0.1, 0.9, 1.0, None)
    assert lib.dk_sgd_momentum_multi_f32(None, 0, 0, 0.1, 0.9, 1.0, None) == 0  # nothing to do
    assert lib.dk_sgd_momentum_multi_f32(p, 0, 5, 0.1, 0.9, 1.0, None) == 0


# ---- the state file ------------------------------------------------------------------------------

def _small_net():
    from dorknet_amd.layers.batch_norm import BatchNormLayer
    from dorknet_amd.layers.convolution import ConvLayer
    from dorknet_amd.layers.dense_layer import DenseLayer
    from dorknet_amd.network.feed_forward_network import FeedForwardNetwork
    np.random.seed(5)
    net = FeedForwardNetwork("small")
    net.add_layer(ConvLayer("conv", filter_block_shape=(8, 4, 3, 3), with_bias=False))
    net.add_layer(BatchNormLayer("bn", input_dimension=4, incoming_chans=8))
    net.add_layer(DenseLayer("dense", incoming_chans=8, output_dim=5))
    return net


def _filled(opt, seed):
    rng = np.random.default_rng(seed)
    for d in opt.grad_cache.values():
        for k in d:
            d[k][...] = rng.standard_normal(d[k].shape).astype(np.float32)
    return opt


def _snapshot(opt):
    hyper = {h: getattr(opt, h) for h in ("learning_rate", *opt._HYPER)}
    return hyper, {(l.layer_name, k): np.array(v) for l, d in getattr(opt, "grad_cache", {}).items()
                   for k, v in d.items()}


def _same(a, b):
    return a[0] == b[0] and a[1].keys() == b[1].keys() and all(np.array_equal(a[1][k], b[1][k]) for k in a[1])


@needs_h5
def test_state_file_layout_and_host_round_trip(tmp_path):
    net = _small_net()
    for cls, args, hyper in [(SGDMomentum, (0.25, 0.75), "momentum"), (RMSProp, (0.25, 0.75), "decay_rate"),
                             (SGD, (0.25,), None)]:
        fname = str(tmp_path / (cls.__name__ + ".h5"))
        opt = cls(net, *args)
        if hyper:
            _filled(opt, 1)
        opt.save_state_to_h5(fname)
        with checkpoint.open_h5(fname, "r") as f:
            assert list(f.keys()) == ["optimiser"]
            a = f["optimiser"].attrs
            want = {"type", "learning_rate", "update_skip_projections"} | ({hyper} if hyper else set())
            assert set(a.keys()) == want
            assert checkpoint._as_str(a["type"]) == cls.__name__ and float(a["learning_rate"]) == 0.25
            assert bool(a["update_skip_projections"]) is False
            if hyper:
                assert float(a[hyper]) == 0.75
                assert sorted(f["optimiser"].keys()) == ["bn", "conv", "dense"]
                for layer in opt.learnable_layers:
                    for k, v in opt.grad_cache[layer].items():
                        d = f["optimiser/{}/{}".format(layer.layer_name, k)]
                        assert tuple(d.shape) == v.shape and d.dtype == np.float32 and np.array_equal(d[:], v)
            else:
                assert list(f["optimiser"].keys()) == []
        fresh = cls(net, *((0.5, 0.5) if hyper else (0.5,)))
        tensors = {(l.layer_name, k): id(v) for l, d in getattr(fresh, "grad_cache", {}).items()
                   for k, v in d.items()}
        fresh.load_state_from_h5(fname)
        assert _same(_snapshot(fresh), _snapshot(opt))
        if hyper:
            assert all(id(fresh.grad_cache[l][k]) == tensors[(l.layer_name, k)]  # loaded in place
                       for l in fresh.learnable_layers for k in fresh.grad_cache[l])


@needs_h5
def test_state_file_refusals(tmp_path):
    net = _small_net()
    saved = _filled(RMSProp(net, 0.25, 0.75), 1)
    good = str(tmp_path / "rms.h5")
    saved.save_state_to_h5(good)

    def refused(opt, fname):
        before = _snapshot(opt)
        with pytest.raises(ValueError):
            opt.load_state_from_h5(fname)
        assert _same(_snapshot(opt), before)

    # the stored type differs from the optimiser's class
    refused(_filled(SGDMomentum(net, 0.5, 0.5), 2), good)
    refused(SGD(net, 0.5), good)
    sgd_file = str(tmp_path / "sgd.h5")
    SGD(net, 0.125).save_state_to_h5(sgd_file)
    refused(_filled(RMSProp(net, 0.5, 0.5), 2), sgd_file)

    def rewrite(fname, skip=None, reshape=None):
        with checkpoint.open_h5(good, "r") as src, checkpoint.open_h5(fname, "w") as dst:
            g = dst.create_group("optimiser")
            for k in src["optimiser"].attrs.keys():
                g.attrs[k] = src["optimiser"].attrs[k]
            for layer in saved.learnable_layers:
                for k in saved.grad_cache[layer]:
                    path = "optimiser/{}/{}".format(layer.layer_name, k)
                    if path == skip:
                        continue
                    a = src[path][:]
                    if path == reshape:
                        a = a.reshape(-1)
                    dst.create_dataset(path, a.shape, dtype=np.float32)[:] = a

    # a dataset is missing (the last one: everything before it has been read by then)
    fname = str(tmp_path / "missing.h5")
    rewrite(fname, skip="optimiser/dense/bias")
    refused(_filled(RMSProp(net, 0.5, 0.5), 2), fname)
    # a dataset's shape differs (same element count)
    fname = str(tmp_path / "shape.h5")
    rewrite(fname, reshape="optimiser/dense/weights")
    refused(_filled(RMSProp(net, 0.5, 0.5), 2), fname)
    # the rewritten file is otherwise loadable: the refusals above are about what was changed
    fname = str(tmp_path / "copy.h5")
    rewrite(fname)
    ok = _filled(RMSProp(net, 0.5, 0.5), 2)
    ok.load_state_from_h5(fname)
    assert _same(_snapshot(ok), _snapshot(saved))

    # two learnable layers share a layer_name
    dup = _small_net()
    dup.layers[2].layer_name = "conv"
    refused(_filled(RMSProp(dup, 0.5, 0.5), 2), good)
    with pytest.raises(ValueError):
        RMSProp(dup, 0.5, 0.5).save_state_to_h5(str(tmp_path / "dup.h5"))
