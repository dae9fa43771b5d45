"""Adam / AdamW and global-norm clipping without a GPU: the definition (tests/_adam_twin.py) against
torch.optim.Adam / AdamW on the CPU, the fp32 twin against its fp64 version, parameter discovery, the
DataParallel handshake, the refusal of host tensors, the C entries' argument checks, the decay flags
and the state file."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import dorknet_amd
from dorknet_amd import _hip
from dorknet_amd.network import checkpoint
from dorknet_amd.optimisers import clip
from dorknet_amd.optimisers.Adam import Adam, AdamW, adam_scalars
from dorknet_amd.optimisers.RMSProp import RMSProp
from dorknet_amd.optimisers.SGDMomentum import SGDMomentum
from examples.resnet18_depsep import ResNet18
from tests import _adam_twin as twin

try:
    checkpoint._backend().File  # noqa: B018
    from dorknet_amd.network import _h5lite
    if checkpoint._backend() is _h5lite:
        _h5lite._load()
    HAVE_H5 = True
except ImportError:  # pragma: no cover - environment dependent
    HAVE_H5 = False

needs_h5 = pytest.mark.skipif(not HAVE_H5, reason="neither h5py nor the HDF5 C library is available")

LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
CLASSES = [(Adam, (0.05,)), (AdamW, (0.05, 0.01))]
IDS = ["Adam", "AdamW"]


def _gradient(rng, n):
    """Magnitudes from 1e-6 to 1e1, either sign."""
    return rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-6, 1, n)


def _torch_cases():
    cases = [("Adam", torch.optim.Adam, 0.0, {}), ("AdamW", torch.optim.AdamW, 0.0, {}),
             ("AdamW", torch.optim.AdamW, 0.01, {})]
    # torch.optim.Adam's own weight_decay is the coupled l2 term; its decoupled form (newer torch) is AdamW's
    if "decoupled_weight_decay" in inspect.signature(torch.optim.Adam.__init__).parameters:
        cases.append(("Adam", torch.optim.Adam, 0.01, {"decoupled_weight_decay": True}))
    return cases


@pytest.mark.parametrize("name,cls,wd,kw", _torch_cases(),
                         ids=["{}-{}{}".format(c[0], c[2], "-decoupled" if c[3] else "") for c in _torch_cases()])
def test_fp64_twin_against_torch(name, cls, wd, kw):
    """The definition evaluated in fp64 against torch's CPU implementation in fp64 over ten steps:
    within 2 fp64 ulp of w (1 measured; the second is for another torch build's operation order)."""
    rng = np.random.default_rng(3)
    n = 20000
    W = rng.uniform(1, 2, n) * rng.choice([-1.0, 1.0], n)
    p = torch.nn.Parameter(torch.from_numpy(W.copy()))
    opt = cls([p], lr=LR, betas=(B1, B2), eps=EPS, weight_decay=wd, **kw)
    m, v = np.zeros(n), np.zeros(n)
    worst = 0.0
    for t in range(1, 11):
        g = _gradient(rng, n)
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        W, m, v = twin.adam_update_f64(W, g, m, v, LR, B1, B2, EPS, wd, t)
        got = p.detach().numpy()
        worst = max(worst, float((np.abs(got - W) / np.spacing(np.abs(W))).max()))
    print("{} weight_decay {}: worst |w - torch| = {:.2f} fp64 ulp".format(name, wd, worst))
    assert worst <= 2


def _ulps(got32, want64, at):
    """|got - want| in fp32 ulps at the magnitude `at`."""
    return np.abs(got32.astype(np.float64) - want64) / np.spacing(np.abs(at).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("wd", [0.0, 0.01], ids=["Adam", "AdamW"])
def test_fp32_twin_agrees_with_its_fp64_version(wd):
    """One step from the same fp32 state, fresh and after three twin steps, |w| in [1, 2), lr = 1e-3.

    w <= 3 fp32 ulp: the scalar keep is rounded to fp32 (up to 1 ulp of w through the product), the
    product keep * w adds half an ulp and the final sum half an ulp.  |step| is about lr = 2^-10, so
    each of the step's inner roundings (relative 2^-24 of the step) weighs under 2^-9 ulp of w.
    v <= 4 ulp: its terms are positive; beta2 * v carries two roundings (the scalar, the product),
    omb2 * (g * g) three (the scalar, the square, the product), the sum one: at most 4 x 2^-24
    relative, and an ulp is at least 2^-24 relative.
    m <= 4 units of 2^-24 * (|beta1 * m| + |omb1 * g|): each term carries two roundings (its scalar,
    its product) and the sum one, at most |m| <= the terms' magnitudes; the terms can cancel, so m
    is bounded against them and not against itself."""
    rng = np.random.default_rng(8)
    n = 20000
    W = (rng.uniform(1, 2, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    for t in range(1, 5):  # t = 1: fresh state; t = 4: the state three twin steps reached
        g = _gradient(rng, n).astype(np.float32)
        W32, m32, v32 = twin.adam_update(W, g, m, v, LR, B1, B2, EPS, wd, t)
        if t in (1, 4):
            W64, m64, v64 = twin.adam_update_f64(W, g, m, v, LR, B1, B2, EPS, wd, t)
            unit = 2.0 ** -24 * (np.abs(B1 * m.astype(np.float64)) + np.abs((1 - B1) * g.astype(np.float64)))
            ew, ev = _ulps(W32, W64, W32).max(), _ulps(v32, v64, v32).max()
            em = (np.abs(m32.astype(np.float64) - m64) / unit).max()
            print("weight_decay {} t {}: w {:.2f} ulp, v {:.2f} ulp, m {:.2f} units".format(wd, t, ew, ev, em))
            assert ew <= 3 and ev <= 4 and em <= 4
            assert np.abs(W64 - (1 - LR * wd) * W.astype(np.float64)).max() <= 1.01 * LR  # |step| is about lr
        W, m, v = W32, m32, v32


def test_written_order_and_single_scalar_rounding():
    """On values where they show: every scalar is formed in double and rounded to fp32 once."""
    f = np.float32
    lr, b1, b2, eps, wd, t = 0.1, 0.9, 0.999, 1e-8, 0.3, 2
    W1, m1, v1 = twin.adam_update(f([1.5]), f([3.0]), f([0.5]), f([0.25]), lr, b1, b2, eps, wd, t)
    m_want = f(b1) * f(0.5) + f(1 - b1) * f(3.0)
    v_want = f(b2) * f(0.25) + f(1 - b2) * (f(3.0) * f(3.0))
    den = np.sqrt(v_want) / f(np.sqrt(1 - b2 ** t)) + f(eps)
    w_want = f(1 - lr * wd) * f(1.5) + f(-(lr / (1 - b1 ** t))) * (m_want / den)
    assert m1[0] == m_want and v1[0] == v_want and W1[0] == w_want
    assert all(isinstance(x, np.float32) for x in (m_want, v_want, den, w_want))
    # the single rounding shows: the same scalars formed from fp32 pieces are other numbers
    assert f(1 - b1) != f(1) - f(b1) and f(1 - b2) != f(1) - f(b2)
    assert f(-(lr / (1 - b1 ** t))) != -(f(lr) / (f(1) - f(b1) * f(b1)))
    # no decay for an undecayed tensor or a zero weight_decay; a clip scale multiplies g first
    W2, _, _ = twin.adam_update(f([1.5]), f([3.0]), f([0.5]), f([0.25]), lr, b1, b2, eps, wd, t, decay=False)
    W3, _, _ = twin.adam_update(f([1.5]), f([3.0]), f([0.5]), f([0.25]), lr, b1, b2, eps, 0.0, t)
    assert W2[0] == W3[0] == f(1.5) + f(-(lr / (1 - b1 ** t))) * (m_want / den)
    _, m4, v4 = twin.adam_update(f([1.5]), f([3.0]), f([0.5]), f([0.25]), lr, b1, b2, eps, wd, t, scale=0.7)
    gs = f(0.7) * f(3.0)
    assert m4[0] == f(b1) * f(0.5) + f(1 - b1) * gs and v4[0] == f(b2) * f(0.25) + f(1 - b2) * (gs * gs)
    # the optimiser's scalars are the twin's
    assert adam_scalars(lr, b1, b2, wd, t) == twin.scalars(lr, b1, b2, wd, t)


def test_clip_scale_twin():
    f = np.float32
    assert twin.clip_scale(f(4.0), 2.0) == f(2.0) / (f(4.0) + f(1e-6)) < 1
    assert twin.clip_scale(f(1.0), 2.0) == 1 and twin.clip_scale(f(0.0), 2.0) == 1
    for measure_only in (None, 0.0, -1.0, float("inf")):
        assert twin.clip_scale(f(4.0), measure_only) == 1
    g = f([3.0, -4.0, 1e-30])
    assert twin.norm_f64([g[:2], g[2:]]) == 5.0
    assert np.array_equal(twin.scale_update(g, 0.1), f(0.1) * g)


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
    assert _counts(opt) == (104, 1336312)
    ref = SGDMomentum(net, 0.05, 0.9, update_skip_projections=True)
    opt = cls(net, *args, update_skip_projections=True)
    assert [id(l) for l in opt.learnable_layers] == [id(l) for l in ref.learnable_layers]
    assert sum(l.layer_name.endswith("_pw_skip") for l in opt.learnable_layers) == 3
    assert _counts(opt) == (107, 1336312 + 172032)


def test_signature_state_and_aliases():
    np.random.seed(0)
    net = ResNet18("r18")
    opt = Adam(net, 0.1)
    assert (opt.learning_rate, opt.beta1, opt.beta2, opt.eps, opt.weight_decay) == (0.1, 0.9, 0.999, 1e-8, 0.0)
    assert opt.decay_params == ("weights",) and opt.max_grad_norm is None and opt.step_count == 0
    assert opt.last_grad_norm is None and not hasattr(opt, "grad_cache")
    kw = Adam(network=net, learning_rate=0.2, beta1=0.8, beta2=0.99, eps=1e-6, weight_decay=0.1,
              decay_params=("weights", "gamma"), max_grad_norm=2.0, update_skip_projections=True)
    assert (kw.beta1, kw.beta2, kw.eps, kw.weight_decay, kw.max_grad_norm) == (0.8, 0.99, 1e-6, 0.1, 2.0)
    w = AdamW(net, 0.1, 0.05)
    assert isinstance(w, Adam) and w.weight_decay == 0.05 and type(w).__name__ == "AdamW"
    with pytest.raises(TypeError):
        AdamW(net, 0.1)  # the weight decay is required
    opt.set_learning_rate(0.5)
    opt.multiply_learning_rate(0.1)
    assert opt.learning_rate == 0.5 * 0.1
    for state in (opt.m, opt.v):
        assert set(state) == set(opt.learnable_layers)
        for layer in opt.learnable_layers:
            assert state[layer].keys() == layer.grads.keys()
            for k, g in layer.grads.items():
                s = np.asarray(state[layer][k])
                assert s.shape == np.shape(g) and s.dtype == np.float32 and not s.any()
    assert all(opt.m[l][k] is not opt.v[l][k] for l in opt.learnable_layers for k in opt.m[l])
    dorknet_amd.install_reference_aliases()
    from optimisers.Adam import Adam as A2
    from optimisers.clip import clip_grad_norm as c2
    assert A2 is Adam and c2 is clip.clip_grad_norm


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
    assert opt.step_count == 0  # a refused step is not counted
    with pytest.raises(RuntimeError, match="to_gpu"):
        clip.clip_grad_norm(opt, 1.0)
    with pytest.raises(RuntimeError, match="to_gpu"):
        clip.clip_grad_norm(RMSProp(net, 0.1, 0.9), 1.0)


def test_decay_flags():
    """Bit 0 of a row's flags: the tensors whose key is in decay_params -- by default conv and dense
    weights, never gamma, beta or bias."""
    np.random.seed(0)
    net = ResNet18("r18")
    opt = AdamW(net, 0.1, 0.01)
    keys = [k for l in opt.learnable_layers for k in l.learned_params]
    flags = [e[4] for e in opt._entries()]
    assert len(flags) == len(keys) == 104 and set(keys) == {"weights", "bias", "gamma", "beta"}
    assert flags == [1 if k == "weights" else 0 for k in keys] and 0 < sum(flags) < 104
    for (w, g, m, v, _), (l, k) in zip(opt._entries(), [(l, k) for l in opt.learnable_layers
                                                        for k in l.learned_params]):
        assert w is l.learned_params[k] and g is l.grads[k] and m is opt.m[l][k] and v is opt.v[l][k]
    opt = Adam(net, 0.1, weight_decay=0.01, decay_params=("gamma", "bias"))
    assert [e[4] for e in opt._entries()] == [1 if k in ("gamma", "bias") else 0 for k in keys]
    assert not any(e[4] for e in Adam(net, 0.1, weight_decay=0.01, decay_params=())._entries())


@pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="run __graft_entry__.build() first")
def test_argument_errors_without_a_device():
    lib = _hip.lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    adam = (0.9, 0.1, 0.999, 0.001, -0.01, 0.03, 1e-8, 1.0, None, None)
    for table, ntens, blocks in [(None, 1, 1), (p, -1, 1), (p, 1, -1), (p, 1, 1 << 31)]:
        with pytest.raises(_hip.HipError, match="bad arguments"):
            lib.dk_adam_multi_f32(table, ntens, blocks, *adam)
        with pytest.raises(_hip.HipError, match="bad arguments"):
            lib.dk_grad_norm_multi_f32(table, ntens, blocks, 1.0, p, p, 64, None)
        with pytest.raises(_hip.HipError, match="bad arguments"):
            lib.dk_grad_scale_multi_f32(table, ntens, blocks, p, None)
    with pytest.raises(_hip.HipError, match="bad arguments"):
        lib.dk_grad_norm_multi_f32(p, 1, 1, 1.0, None, p, 64, None)  # no output
    with pytest.raises(_hip.HipError, match="bad arguments"):
        lib.dk_grad_scale_multi_f32(p, 1, 1, None, None)  # no scale
    with pytest.raises(_hip.HipError, match="workspace too small"):
        lib.dk_grad_norm_multi_f32(p, 1, 9, 1.0, p, p, 64, None)  # 9 partials need 72 bytes
    with pytest.raises(_hip.HipError, match="workspace too small"):
        lib.dk_grad_norm_multi_f32(p, 1, 1, 1.0, p, None, 64, None)
    assert lib.dk_adam_multi_f32(None, 0, 0, *adam) == 0  # nothing to do
    assert lib.dk_grad_scale_multi_f32(None, 0, 0, p, None) == 0
    assert lib.dk_grad_norm_workspace_bytes(100) == 800 and lib.dk_grad_norm_workspace_bytes(0) == 0
    assert clip.CHUNK == 2048


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


def _filled(opt, seed, steps=7):
    rng = np.random.default_rng(seed)
    for state in (opt.m, opt.v):
        for d in state.values():
            for k in d:
                d[k][...] = rng.standard_normal(d[k].shape).astype(np.float32)
    opt.step_count = steps
    return opt


HYPER = ("learning_rate", "beta1", "beta2", "eps", "weight_decay", "step_count")


def _snapshot(opt):
    return ({h: getattr(opt, h) for h in HYPER},
            {(l.layer_name, k, s): np.array(state[l][k]) for s, state in (("m", opt.m), ("v", opt.v))
             for l in opt.learnable_layers for k in state[l]})


def _same(a, b):
    return a[0] == b[0] and a[1].keys() == b[1].keys() and all(np.array_equal(a[1][k], b[1][k]) for k in a[1])


@needs_h5
@pytest.mark.parametrize("cls", [Adam, AdamW], ids=IDS)
def test_state_file_layout_and_host_round_trip(cls, tmp_path):
    net = _small_net()
    fname = str(tmp_path / "adam.h5")
    opt = _filled(cls(net, 0.25, weight_decay=0.125, beta1=0.75, beta2=0.875, eps=1e-6, max_grad_norm=3.0), 1)
    opt.save_state_to_h5(fname)
    with checkpoint.open_h5(fname, "r") as f:
        assert list(f.keys()) == ["optimiser"]
        a = f["optimiser"].attrs
        assert set(a.keys()) == {"type", "learning_rate", "beta1", "beta2", "eps", "weight_decay", "step_count",
                                 "update_skip_projections"}  # max_grad_norm and decay_params are not stored
        assert checkpoint._as_str(a["type"]) == cls.__name__
        assert [float(a[h]) for h in HYPER[:5]] == [0.25, 0.75, 0.875, 1e-6, 0.125] and int(a["step_count"]) == 7
        assert bool(a["update_skip_projections"]) is False
        assert sorted(f["optimiser"].keys()) == ["bn", "conv", "dense"]
        assert sorted(f["optimiser/bn"].keys()) == ["beta", "gamma"]
        assert sorted(f["optimiser/bn/gamma"].keys()) == ["m", "v"]
        for layer in opt.learnable_layers:
            for k in layer.learned_params:
                for s, state in (("m", opt.m), ("v", opt.v)):
                    d = f["optimiser/{}/{}/{}".format(layer.layer_name, k, s)]
                    want = state[layer][k]
                    assert tuple(d.shape) == want.shape and d.dtype == np.float32 and np.array_equal(d[:], want)
    fresh = cls(net, 0.5, weight_decay=0.5)
    tensors = {(l.layer_name, k, s): id(state[l][k]) for s, state in (("m", fresh.m), ("v", fresh.v))
               for l in fresh.learnable_layers for k in state[l]}
    fresh.load_state_from_h5(fname)
    assert _same(_snapshot(fresh), _snapshot(opt)) and isinstance(fresh.step_count, int)
    assert fresh.max_grad_norm is None and fresh.decay_params == ("weights",)
    assert all(id(state[l][k]) == tensors[(l.layer_name, k, s)]  # loaded in place
               for s, state in (("m", fresh.m), ("v", fresh.v)) for l in fresh.learnable_layers for k in state[l])


@needs_h5
def test_state_file_refusals(tmp_path):
    net = _small_net()
    saved = _filled(Adam(net, 0.25, weight_decay=0.125), 1)
    good = str(tmp_path / "adam.h5")
    saved.save_state_to_h5(good)

    def refused(opt, fname):
        before = _snapshot(opt) if isinstance(opt, Adam) else None
        with pytest.raises(ValueError):
            opt.load_state_from_h5(fname)
        assert before is None or _same(_snapshot(opt), before)

    # the stored type differs from the optimiser's class: Adam and AdamW are told apart, both ways
    refused(_filled(AdamW(net, 0.5, 0.5), 2), good)
    refused(RMSProp(net, 0.5, 0.5), good)
    w_file, rms_file = str(tmp_path / "adamw.h5"), str(tmp_path / "rms.h5")
    _filled(AdamW(net, 0.25, 0.125), 1).save_state_to_h5(w_file)
    RMSProp(net, 0.25, 0.75).save_state_to_h5(rms_file)
    refused(_filled(Adam(net, 0.5), 2), w_file)
    refused(_filled(Adam(net, 0.5), 2), rms_file)
    # saved with another update_skip_projections
    refused(_filled(Adam(net, 0.5, update_skip_projections=True), 2), good)

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

    # a dataset is missing (the last one: everything before it has been read by then)
    fname = str(tmp_path / "missing.h5")
    rewrite(fname, skip="optimiser/dense/bias/v")
    refused(_filled(Adam(net, 0.5), 2), fname)
    # a dataset's shape differs (same element count)
    fname = str(tmp_path / "shape.h5")
    rewrite(fname, reshape="optimiser/dense/weights/m")
    refused(_filled(Adam(net, 0.5), 2), fname)
    # an attribute is missing
    fname = str(tmp_path / "attr.h5")
    rewrite(fname, drop_attr="step_count")
    refused(_filled(Adam(net, 0.5), 2), fname)
    # the rewritten file is otherwise loadable: the refusals above are about what was changed
    fname = str(tmp_path / "copy.h5")
    rewrite(fname)
    ok = _filled(Adam(net, 0.5), 2)
    ok.load_state_from_h5(fname)
    assert _same(_snapshot(ok), _snapshot(saved))

    # two learnable layers share a layer_name
    dup = _small_net()
    dup.layers[2].layer_name = "conv"
    refused(_filled(Adam(dup, 0.5), 2), good)
    with pytest.raises(ValueError):
        Adam(dup, 0.5).save_state_to_h5(str(tmp_path / "dup.h5"))
