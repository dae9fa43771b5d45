"""LARS without a GPU: the definition (tests/_lars_twin.py) against torch.optim.SGD on the CPU in fp64, the
written order and the single rounding of each scalar, parameter discovery, the DataParallel handshake,
the refusal of host tensors, the adapt flags, the reference alias, the C entries' argument checks and
the state file."""
import ctypes
import os

import numpy as np
import pytest
import torch

import dorknet_amd
from dorknet_amd import _hip
from dorknet_amd.network import checkpoint
from dorknet_amd.optimisers import clip
from dorknet_amd.optimisers.LARS import LARS
from dorknet_amd.optimisers.RMSProp import RMSProp
from dorknet_amd.optimisers.SGDMomentum import SGDMomentum
from examples.resnet18_depsep import ResNet18
from tests import _lars_twin as twin
from tests import _optim_twin

try:
    checkpoint._backend().File  # noqa: B018
    from dorknet_amd.network import _h5lite
    if checkpoint._backend() is _h5lite:
        _h5lite._load()
    HAVE_H5 = True
except ImportError:  # pragma: no cover - environment dependent
    HAVE_H5 = False

needs_h5 = pytest.mark.skipif(not HAVE_H5, reason="neither h5py nor the HDF5 C library is available")

CLASSES = [(LARS, (0.05,))]
IDS = ["LARS"]


# ---- the rule ------------------------------------------------------------------------------------

def test_written_order_and_single_scalar_rounding():
    """On values where they show: every scalar is formed in double and rounded to fp32 once, and the
    operations run in the order written."""
    f = np.float32
    lr, mom, trust, wd, eps = 0.1, 0.9, 0.001, 0.3, 1e-8
    wn, gn = f(3.3), f(2.9)
    r = twin.trust_ratio(wn, gn, trust, wd, eps)
    r_want = (f(trust) * wn) / ((gn + f(wd) * wn) + f(eps))
    assert isinstance(r, np.float32) and r == r_want
    # the order shows: the same expression associated another way is another number
    assert r != f(trust) * (wn / ((gn + f(wd) * wn) + f(eps)))
    # eps is added last, to the rounded sum: with a norm pair whose sum's spacing is above eps it vanishes,
    assert twin.trust_ratio(wn, gn, trust, wd, eps) == twin.trust_ratio(wn, gn, trust, wd, 0.0)
    # ... and with tiny norms it decides
    tiny = twin.trust_ratio(f(1e-8), f(1e-8), trust, 0.0, eps)
    assert tiny == (f(trust) * f(1e-8)) / (f(1e-8) + f(eps)) != twin.trust_ratio(f(1e-8), f(1e-8), trust, 0.0, 0.0)
    # ratio exactly 1: not adapted, or either norm zero; a non-finite norm is not special-cased
    assert twin.trust_ratio(wn, gn, trust, wd, eps, adapt=False) == 1
    assert twin.trust_ratio(f(0), gn, trust, wd, eps) == 1 and twin.trust_ratio(wn, f(0), trust, wd, eps) == 1
    assert np.isnan(twin.trust_ratio(f(np.inf), f(np.inf), trust, wd, eps))
    assert twin.trust_ratio(wn, f(np.inf), trust, wd, eps) == 0
    # (a NaN norm fails the rule's "> 0" as written: ratio 1, and the NaN is in the tensor itself)
    assert twin.trust_ratio(f(np.nan), gn, trust, wd, eps) == 1

    W, g, v = f([1.5]), f([3.0]), f([0.5])
    r = twin.trust_ratio(f(1.7), f(0.9), trust, wd, eps)
    W1, v1 = twin.lars_update(W, g, v, lr, mom, wd, r)
    g_want = f(3.0) + f(wd) * f(1.5)
    step = f(-lr) * r
    d_want = step * g_want + f(mom) * f(0.5)
    assert all(isinstance(x, np.float32) for x in (g_want, step, d_want))
    assert v1[0] == d_want and W1[0] == f(1.5) + d_want
    # the step is one number formed first: scaling the gradient by the ratio and then by -lr differs
    assert twin.lars_update(W, g, f([0.0]), lr, mom, wd, r)[1][0] == step * g_want != f(-lr) * (r * g_want)
    # the scalars are rounded once from double: built from fp32 pieces they are other numbers
    lr2 = 0.3 * 3
    assert f(lr2) != f(0.3) * f(3) and twin.lars_update(W, g, v, lr2, mom, 0.0, 1.0)[1][0] == \
        f(-lr2) * f(3.0) + f(mom) * f(0.5)
    # no decay for a tensor that is not adapted or a zero weight_decay; with ratio 1 the step is -lr
    # exactly and the update is SGD momentum's
    W2, v2 = twin.lars_update(W, g, v, lr, mom, wd, 1.0, adapt=False)
    W3, v3 = twin.lars_update(W, g, v, lr, mom, 0.0, 1.0)
    Ws, vs = _optim_twin.sgd_momentum_update(W, g, v, lr, mom)
    assert W2[0] == W3[0] == Ws[0] and v2[0] == v3[0] == vs[0] == f(-lr) * f(3.0) + f(mom) * f(0.5)
    # the fp64 twin is the same expression in double
    W4, v4 = twin.lars_update_f64(W, g, v, lr, mom, wd, 0.25)
    d64 = (-lr * 0.25) * (3.0 + wd * 1.5) + mom * 0.5
    assert v4[0] == d64 and W4[0] == 1.5 + d64
    assert twin.trust_ratio_f64(1.7, 2.9, trust, wd, eps) == (trust * 1.7) / ((2.9 + wd * 1.7) + eps)


def test_twin_matches_sgd_momentum_twin_when_not_adapted():
    rng = np.random.default_rng(1)
    n = 5000
    W, g, v = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    a = twin.lars_update(W, g, v, 0.03, 0.9, 0.01, twin.trust_ratio(3.0, 4.0, 0.001, 0.01, 1e-8, adapt=False),
                         adapt=False)
    b = _optim_twin.sgd_momentum_update(W, g, v, 0.03, 0.9)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


STEPS, PER_STEP = 5, 1.2
D_MAX = 2.0 ** -6


def _fp64_inputs(seed, n=20000):
    rng = np.random.default_rng(seed)
    W = rng.uniform(1.25, 1.75, n) * rng.choice([-1.0, 1.0], n)
    return rng, W


def _ulps_of_w(got, want):
    return float((np.abs(got - want) / np.spacing(np.abs(want))).max())


def test_fp64_twin_against_torch_not_adapted():
    """adapt_params = (): the fp64 twin against torch.optim.SGD(momentum=0.9) in fp64 over 5 steps at a
    constant lr, where torch's buffer is buf = mom * buf + g and v = -lr * buf.

    The bound, counted: |w| stays in [1, 2) (asserted), so an ulp of w is 2^-52 = 2u with u = 2^-53.
    Per step each side rounds its final w + d once: 0.5 ulp each, 1 ulp of new difference.  The two d
    differ by their own roundings: the twin's d = v carries 3 per step (two products, one sum) on terms
    of at most D = max(|lr g|, |d|) <= 2^-6 (asserted), carried on by the momentum, at most
    3 u D (1 - 0.9^5) / 0.1 = 12.3 u D; torch's buffer carries 2 per step on terms of at most D / lr, which
    after the factor lr is 8.2 u D, and lr * buf rounds once more (fused or not): u D.  Together
    21.5 u D <= 21.5 / 64 u < 0.17 ulp.  So 1.2 ulp per step covers it: 6 ulp over the 5 steps.  The
    same count bounds |v + lr * buf| by 21.5 u D (the product's rounding is then this test's own)."""
    lr, mom = 1e-3, 0.9
    rng, W = _fp64_inputs(3)
    n = W.size
    p = torch.nn.Parameter(torch.from_numpy(W.copy()))
    opt = torch.optim.SGD([p], lr=lr, momentum=mom)
    v = np.zeros(n)
    worst = worst_v = 0.0
    for _ in range(STEPS):
        g = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-4, 0, n)
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        W, v, ratio = twin.lars_step_f64(W, g, v, lr, mom, 0.001, 0.0, 1e-8, adapt=False)
        assert ratio == 1.0
        assert np.abs(v).max() <= D_MAX and np.abs(lr * g).max() <= D_MAX and 1 <= np.abs(W).min() \
            and np.abs(W).max() < 2
        buf = opt.state[p]["momentum_buffer"].numpy()
        worst_v = max(worst_v, float(np.abs(v + lr * buf).max() / (2.0 ** -53 * D_MAX)))
        worst = max(worst, _ulps_of_w(p.detach().numpy(), W))
    print("not adapted: worst |w - torch| = {:.2f} fp64 ulp (bound {}), worst |v + lr buf| = {:.2f} u D "
          "(bound 21.5)".format(worst, STEPS * PER_STEP, worst_v))
    assert worst <= STEPS * PER_STEP and worst_v <= 21.5


def test_fp64_twin_against_torch_adapted():
    """Momentum 0 with weight_decay: the fp64 twin against torch.optim.SGD(weight_decay=wd) in fp64 over 5
    steps, the group's lr set to lr * ratio before each step, the ratio formed from numpy's fp64 norms
    of the twin's w and of g (the same double for both sides, and -(lr * ratio) is the twin's step
    exactly).

    The bound, counted as in the test above: 1 ulp of new difference per step from the two final
    sums.  d = step * (g + wd * w) + 0 * v carries at most 3 roundings on either side (wd * w, the sum,
    the product; torch may fuse and round less), each at most u D with D = |step| (|g| + wd |w|) <= 2^-6
    (asserted): 6 u D < 0.05 ulp; the earlier difference in w comes back through wd * step * w, a factor
    below 2^-6 of it.  1.2 ulp per step covers it: 6 ulp over the 5 steps."""
    lr, trust, wd, eps = 1.0, 0.001, 0.01, 1e-8
    rng, W = _fp64_inputs(4)
    n = W.size
    p = torch.nn.Parameter(torch.from_numpy(W.copy()))
    opt = torch.optim.SGD([p], lr=lr, momentum=0.0, weight_decay=wd)
    v = np.zeros(n)
    worst, ratios = 0.0, []
    for _ in range(STEPS):
        g = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-4, 0, n)
        ratio = twin.trust_ratio_f64(twin.norm_f64(W), twin.norm_f64(g), trust, wd, eps)
        ratios.append(ratio)
        assert (lr * ratio * (np.abs(g) + wd * np.abs(W))).max() <= D_MAX
        opt.param_groups[0]["lr"] = lr * ratio
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        W, v, r2 = twin.lars_step_f64(W, g, v, lr, 0.0, trust, wd, eps)
        assert r2 == ratio and 1 <= np.abs(W).min() and np.abs(W).max() < 2
        worst = max(worst, _ulps_of_w(p.detach().numpy(), W))
    print("adapted: worst |w - torch| = {:.2f} fp64 ulp (bound {}); ratios {}".format(
        worst, STEPS * PER_STEP, ["{:.3e}".format(r) for r in ratios]))
    assert worst <= STEPS * PER_STEP
    assert all(0 < r < 1 and r != ratios[0] for r in ratios[1:])  # the ratio is at work and moves


# ---- the optimiser -------------------------------------------------------------------------------

def _counts(opt):
    ntens = sum(len(l.learned_params) for l in opt.learnable_layers)
    nparam = sum(v.size for l in opt.learnable_layers for v in l.learned_params.values())
    return ntens, nparam


@pytest.mark.parametrize("cls,args", CLASSES, ids=IDS)
def test_discovery_is_sgd_momentum_s(cls, args):
    np.random.seed(0)
    net = ResNet18("r18")
    ref = SGDMomentum(net, 0.05, 0.9)
    opt = cls(net, *args)
    assert [id(l) for l in opt.learnable_layers] == [id(l) for l in ref.learnable_layers]
    assert _counts(opt) == (104, 1336312) and len(opt.stat_names) == 104
    ref = SGDMomentum(net, 0.05, 0.9, update_skip_projections=True)
    opt = cls(net, *args, update_skip_projections=True)
    assert [id(l) for l in opt.learnable_layers] == [id(l) for l in ref.learnable_layers]
    assert sum(l.layer_name.endswith("_pw_skip") for l in opt.learnable_layers) == 3
    assert _counts(opt) == (107, 1336312 + 172032) and len(opt.stat_names) == 107


@pytest.mark.parametrize("cls,args", CLASSES, ids=IDS)
def test_data_parallel_handshake(cls, args):
    np.random.seed(0)
    net = ResNet18("r18")
    net._dp_update_skip_projections = True
    with pytest.raises(ValueError, match="update_skip_projections"):
        cls(net, *args)
    opt = cls(net, *args, update_skip_projections=True)
    assert net._opt_update_skip_projections is True and opt.update_skip_projections is True
    net._dp_update_skip_projections = False
    with pytest.raises(ValueError, match="update_skip_projections"):
        cls(net, *args, update_skip_projections=True)
    cls(net, *args)
    assert net._opt_update_skip_projections is False


@pytest.mark.parametrize("cls,args", CLASSES, ids=IDS)
def test_host_parameters_are_refused(cls, args):
    np.random.seed(0)
    net = ResNet18("r18")
    opt = cls(net, *args)
    with pytest.raises(RuntimeError, match="to_gpu"):
        opt.update_weights()
    with pytest.raises(RuntimeError, match="to_gpu"):
        opt.measure_tensor_norms()
    assert opt.last_stats is None  # a refused step leaves nothing behind
    with pytest.raises(RuntimeError, match="to_gpu"):
        clip.clip_grad_norm(opt, 1.0)


def test_signature_state_flags_and_aliases():
    np.random.seed(0)
    net = ResNet18("r18")
    opt = LARS(net, 0.1)
    assert (opt.learning_rate, opt.momentum, opt.trust_coefficient, opt.weight_decay, opt.eps) == \
        (0.1, 0.9, 0.001, 0.0, 1e-8)
    assert opt.adapt_params == ("weights",) and opt.last_stats is None and opt.update_skip_projections is False
    assert LARS._HYPER == ("momentum", "trust_coefficient", "weight_decay", "eps")
    assert LARS._PER_BLOCK == 2048 and SGDMomentum._PER_BLOCK == 256 and RMSProp._PER_BLOCK == 256
    assert opt._dev.per_block == 2048 and SGDMomentum(net, 0.1, 0.9)._dev.per_block == 256
    kw = LARS(network=net, learning_rate=0.2, momentum=0.8, trust_coefficient=0.02, weight_decay=1e-4, eps=1e-6,
              adapt_params=("weights", "gamma"), update_skip_projections=True)
    assert (kw.momentum, kw.trust_coefficient, kw.weight_decay, kw.eps) == (0.8, 0.02, 1e-4, 1e-6)
    assert kw.adapt_params == ("weights", "gamma") and kw.update_skip_projections is True
    opt.set_learning_rate(0.5)
    opt.multiply_learning_rate(0.1)
    assert opt.learning_rate == 0.5 * 0.1
    # the state is SGDMomentum's: one zero velocity per gradient
    assert set(opt.grad_cache) == set(opt.learnable_layers)
    for layer in opt.learnable_layers:
        assert opt.grad_cache[layer].keys() == layer.grads.keys()
        for k, g in layer.grads.items():
            s = np.asarray(opt.grad_cache[layer][k])
            assert s.shape == np.shape(g) and s.dtype == np.float32 and not s.any()
    # bit 0 of a row's flags: exactly the weights by default, and as adapt_params says
    pairs = [(l, k) for l in opt.learnable_layers for k in l.learned_params]
    keys = [k for _, k in pairs]
    assert opt.stat_names == [(l.layer_name, k) for l, k in pairs]
    flags = [e[3] for e in opt._entries()]
    assert len(flags) == 104 and set(keys) == {"weights", "bias", "gamma", "beta"}
    assert flags == [1 if k == "weights" else 0 for k in keys] and 0 < sum(flags) < 104
    for (w, g, v, _), (l, k) in zip(opt._entries(), pairs):
        assert w is l.learned_params[k] and g is l.grads[k] and v is opt.grad_cache[l][k]
    assert [e[3] for e in kw._entries()][:104] != flags
    assert [e[3] for e in LARS(net, 0.1, adapt_params=("gamma", "bias"))._entries()] == \
        [1 if k in ("gamma", "bias") else 0 for k in keys]
    assert not any(e[3] for e in LARS(net, 0.1, adapt_params=())._entries())
    dorknet_amd.install_reference_aliases()
    from optimisers.LARS import LARS as L2
    assert L2 is LARS


@pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="run __graft_entry__.build() first")
def test_argument_errors_without_a_device():
    lib = _hip.lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    for table, ntens, blocks in [(None, 1, 1), (p, -1, 1), (p, 1, -1), (p, 1, 1 << 31)]:
        with pytest.raises(_hip.HipError, match="bad arguments"):
            lib.dk_lars_norms_multi_f32(table, ntens, blocks, 0.001, 0.0, 1e-8, p, p, 64, None)
        with pytest.raises(_hip.HipError, match="bad arguments"):
            lib.dk_lars_multi_f32(table, ntens, blocks, 0.1, 0.9, 0.0, p, None)
    with pytest.raises(_hip.HipError, match="bad arguments"):
        lib.dk_lars_norms_multi_f32(p, 1, 1, 0.001, 0.0, 1e-8, None, p, 64, None)  # no stats
    with pytest.raises(_hip.HipError, match="bad arguments"):
        lib.dk_lars_multi_f32(p, 1, 1, 0.1, 0.9, 0.0, None, None)  # no stats
    with pytest.raises(_hip.HipError, match="workspace too small"):
        lib.dk_lars_norms_multi_f32(p, 1, 5, 0.001, 0.0, 1e-8, p, p, 64, None)  # 5 blocks need 80 bytes
    with pytest.raises(_hip.HipError, match="workspace too small"):
        lib.dk_lars_norms_multi_f32(p, 1, 1, 0.001, 0.0, 1e-8, p, None, 64, None)
    assert lib.dk_lars_norms_multi_f32(None, 0, 0, 0.001, 0.0, 1e-8, p, None, 0, None) == 0  # nothing to do
    assert lib.dk_lars_multi_f32(None, 0, 0, 0.1, 0.9, 0.0, p, None) == 0
    assert lib.dk_lars_workspace_bytes(100) == 1600 and lib.dk_lars_workspace_bytes(1) == 16
    assert lib.dk_lars_workspace_bytes(0) == 0 and lib.dk_lars_workspace_bytes(-3) == 0


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


HYPER = ("learning_rate", "momentum", "trust_coefficient", "weight_decay", "eps")


def _snapshot(opt):
    return ({h: getattr(opt, h) for h in HYPER if hasattr(opt, h)},
            {(l.layer_name, k): np.array(opt.grad_cache[l][k]) for l in opt.learnable_layers
             for k in opt.grad_cache[l]})


def _same(a, b):
    return a[0] == b[0] and a[1].keys() == b[1].keys() and all(np.array_equal(a[1][k], b[1][k]) for k in a[1])


@needs_h5
def test_state_file_layout_and_host_round_trip(tmp_path):
    net = _small_net()
    fname = str(tmp_path / "lars.h5")
    opt = _filled(LARS(net, 0.25, momentum=0.75, trust_coefficient=0.125, weight_decay=0.5, eps=1e-6,
                       adapt_params=("weights", "gamma")), 1)
    opt.save_state_to_h5(fname)
    with checkpoint.open_h5(fname, "r") as f:
        assert list(f.keys()) == ["optimiser"]
        a = f["optimiser"].attrs
        assert set(a.keys()) == {"type", "learning_rate", "momentum", "trust_coefficient", "weight_decay", "eps",
                                 "update_skip_projections"}  # adapt_params is not stored
        assert checkpoint._as_str(a["type"]) == "LARS"
        assert [float(a[h]) for h in HYPER] == [0.25, 0.75, 0.125, 0.5, 1e-6]
        assert bool(a["update_skip_projections"]) is False
        assert sorted(f["optimiser"].keys()) == ["bn", "conv", "dense"]
        assert sorted(f["optimiser/bn"].keys()) == ["beta", "gamma"]
        for layer in opt.learnable_layers:
            for k in layer.learned_params:
                d = f["optimiser/{}/{}".format(layer.layer_name, k)]
                want = opt.grad_cache[layer][k]
                assert tuple(d.shape) == want.shape and d.dtype == np.float32 and np.array_equal(d[:], want)
    # the datasets are the ones SGDMomentum writes
    sgd_file = str(tmp_path / "sgdm.h5")
    sgd = SGDMomentum(net, 0.25, 0.75)
    sgd.save_state_to_h5(sgd_file)
    assert [p for p, _ in sgd._state_items()] == [p for p, _ in opt._state_items()]
    fresh = LARS(net, 0.5, momentum=0.5)
    tensors = {(l.layer_name, k): id(fresh.grad_cache[l][k]) for l in fresh.learnable_layers
               for k in fresh.grad_cache[l]}
    fresh.load_state_from_h5(fname)
    assert _same(_snapshot(fresh), _snapshot(opt)) and fresh.adapt_params == ("weights",)
    assert all(id(fresh.grad_cache[l][k]) == tensors[(l.layer_name, k)]  # loaded in place
               for l in fresh.learnable_layers for k in fresh.grad_cache[l])


@needs_h5
def test_state_file_refusals(tmp_path):
    net = _small_net()
    saved = _filled(LARS(net, 0.25, weight_decay=0.125), 1)
    good = str(tmp_path / "lars.h5")
    saved.save_state_to_h5(good)

    def refused(opt, fname):
        before = _snapshot(opt)
        with pytest.raises(ValueError):
            opt.load_state_from_h5(fname)
        assert _same(_snapshot(opt), before)

    # the stored type differs from the optimiser's class, both ways: the datasets alone would fit
    sgd_file = str(tmp_path / "sgdm.h5")
    _filled(SGDMomentum(net, 0.25, 0.75), 3).save_state_to_h5(sgd_file)
    refused(_filled(LARS(net, 0.5), 2), sgd_file)
    refused(_filled(SGDMomentum(net, 0.5, 0.5), 2), good)
    # saved with another update_skip_projections
    refused(_filled(LARS(net, 0.5, update_skip_projections=True), 2), good)

    def rewrite(fname, skip=None, reshape=None, drop_attr=None):
        with checkpoint.open_h5(good, "r") as src, checkpoint.open_h5(fname, "w") as dst:
            g = dst.create_group("optimiser")
            for k in src["optimiser"].attrs.keys():
                if k != drop_attr:
                    g.attrs[k] = src["optimiser"].attrs[k]
            for path, _ in saved._state_items():
                if path == skip:
                    continue
                a = src[path][:]
                if path == reshape:
                    a = a.reshape(-1)
                dst.create_dataset(path, a.shape, dtype=np.float32)[:] = a

    # an attribute is missing
    for attr in ("trust_coefficient", "eps"):
        fname = str(tmp_path / "attr_{}.h5".format(attr))
        rewrite(fname, drop_attr=attr)
        refused(_filled(LARS(net, 0.5), 2), fname)
    # a dataset's shape differs (same element count)
    fname = str(tmp_path / "shape.h5")
    rewrite(fname, reshape="optimiser/dense/weights")
    refused(_filled(LARS(net, 0.5), 2), fname)
    # a dataset is missing (the last one: everything before it has been read by then)
    fname = str(tmp_path / "missing.h5")
    rewrite(fname, skip="optimiser/dense/bias")
    refused(_filled(LARS(net, 0.5), 2), fname)
    # the rewritten file is otherwise loadable: the refusals above are about what was changed
    fname = str(tmp_path / "copy.h5")
    rewrite(fname)
    ok = _filled(LARS(net, 0.5), 2)
    ok.load_state_from_h5(fname)
    assert _same(_snapshot(ok), _snapshot(saved))
