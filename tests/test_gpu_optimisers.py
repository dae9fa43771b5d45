"""SGD, SGD momentum and RMSProp on the GPU (dk_sgd_multi_f32, dk_sgd_momentum_multi_f32,
dk_rmsprop_multi_f32; dorknet_amd/optimisers) against the numpy twins of the reference's expressions
(tests/_optim_twin.py), bit for bit: every operation of an update is one correctly rounded fp32
operation and nothing is reduced, so there is no freedom of order and no tolerance.  A difference
means a contracted, reassociated or approximate operation.
Also: the optimiser state file (save_state_to_h5 / load_state_from_h5) through a training run."""
import numpy as np
import pytest
import torch

from dorknet_amd._hip import lib, stream_handle
from dorknet_amd.network import checkpoint
from dorknet_amd.optimisers.RMSProp import RMSProp
from dorknet_amd.optimisers.SGD import SGD
from dorknet_amd.optimisers.SGDMomentum import SGDMomentum
from tests import _optim_twin as twin

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 1000, 4099]  # the block edges (256 elements per block) and a multi-block tail
LR, DECAY = 0.01, 0.9


def _have_h5():
    try:
        b = checkpoint._backend()
        if b.__name__.endswith("_h5lite"):
            b._load()
        return True
    except ImportError:
        return False


needs_h5 = pytest.mark.skipif(not _have_h5(), reason="neither h5py nor the HDF5 C library is available")


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def host(t):
    return t.detach().cpu().numpy().copy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def table(ws, gs, cs=None):
    """The device table of the multi-tensor entries: {w, g, state, n, first_block} per tensor."""
    rows, block0 = [], 0
    for i, (w, g) in enumerate(zip(ws, gs)):
        rows.append((w.data_ptr(), g.data_ptr(), cs[i].data_ptr() if cs is not None else 0, w.numel(), block0))
        block0 += -(-w.numel() // 256)
    return torch.as_tensor(np.array(rows, dtype=np.int64).reshape(-1, 5), device="cuda"), block0


def rmsprop_call(tab, ntens, blocks, lr=LR, decay=DECAY):
    lib.dk_rmsprop_multi_f32(tab.data_ptr(), ntens, blocks, float(lr), float(decay), 1.0 - float(decay), 1e-5,
                             stream_handle())


def sgd_call(tab, ntens, blocks, lr=LR):
    lib.dk_sgd_multi_f32(tab.data_ptr(), ntens, blocks, float(lr), stream_handle())


# planted into the 4099-element tensor, the last three inside its tail block: (index, gradient, cache)
PLANTED = [(0, 0.0, 0.0),            # g = 0 with c = 0: the weight must not change
           (5, 1e-20, 0.0), (300, -1e-20, 0.0),      # the square is a denormal
           (4097, 1e20, None), (4098, -1e20, None),  # the square overflows: c = inf, the step is -+0
           (4096, 0.0, 0.0)]


def _inputs(rng, step):
    gs = [rng.standard_normal(n).astype(np.float32) for n in SIZES]
    for i, g, _ in PLANTED:
        gs[-1][i] = g
    return gs


def test_raw_entries_bit_for_bit():
    rng = np.random.default_rng(11)
    W = [rng.standard_normal(n).astype(np.float32) for n in SIZES]
    C = [(rng.standard_normal(n) ** 2).astype(np.float32) for n in SIZES]
    C[0][:] = 0  # a fresh cache
    for i, _, c in PLANTED:
        if c is not None:
            C[-1][i] = c
    Ws, Wr, Cr = [w.copy() for w in W], [w.copy() for w in W], [c.copy() for c in C]
    ws, wr, cr = [dev(w) for w in W], [dev(w) for w in W], [dev(c) for c in C]
    gs = [torch.empty(n, dtype=torch.float32, device="cuda") for n in SIZES]
    tab_s, blocks = table(ws, gs)
    tab_r, _ = table(wr, gs, cr)
    assert blocks == sum(-(-n // 256) for n in SIZES) == 1 + 1 + 1 + 2 + 4 + 17
    W_before = W[-1].copy()
    for step in range(3):  # consecutive steps: the cache (inf included) carries over
        G = _inputs(rng, step)
        for g, a in zip(gs, G):
            g.copy_(dev(a))
        sgd_call(tab_s, len(SIZES), blocks)
        rmsprop_call(tab_r, len(SIZES), blocks)
        torch.cuda.synchronize()
        for t, n in enumerate(SIZES):
            Ws[t] = twin.sgd_update(Ws[t], G[t], LR)
            Wr[t], Cr[t] = twin.rmsprop_update(Wr[t], G[t], Cr[t], LR, DECAY)
            assert same_bits(host(ws[t]), Ws[t]), ("sgd w", step, n)
            assert same_bits(host(cr[t]), Cr[t]), ("rmsprop c", step, n)
            assert same_bits(host(wr[t]), Wr[t]), ("rmsprop w", step, n)
            assert same_bits(host(gs[t]), G[t]), ("gradients are read only", step, n)
    # the planted cases did what they are there for
    w_s, w_r, c_r = host(ws[-1]), host(wr[-1]), host(cr[-1])
    for i in (0, 4096):
        assert same_bits(w_s[i:i + 1], W_before[i:i + 1]) and same_bits(w_r[i:i + 1], W_before[i:i + 1])
        assert c_r[i] == 0
    for i in (5, 300):  # a denormal survived: not flushed (as bits: the host may compare denormals as zero)
        assert 0 < int(c_r.view(np.uint32)[i]) < 0x00800000
    for i in (4097, 4098):
        assert np.isinf(c_r[i]) and same_bits(w_r[i:i + 1], W_before[i:i + 1])
    assert w_s[4097] < -1e17 and w_s[4098] > 1e17  # one gradient of each sign


def test_more_tensors_than_the_lds_table_holds():
    """1025 tensors (the owner search's LDS table holds 1024: the linear fallback), 3 elements each."""
    rng = np.random.default_rng(12)
    T, n = 1025, 3
    W = rng.standard_normal(T * n).astype(np.float32)
    G = rng.standard_normal(T * n).astype(np.float32)
    C = (rng.standard_normal(T * n) ** 2).astype(np.float32)
    ws, wr, cr, g = dev(W), dev(W), dev(C), dev(G)
    cut = lambda t: [t[i * n:(i + 1) * n] for i in range(T)]  # noqa: E731
    tab_s, blocks = table(cut(ws), cut(g))
    tab_r, _ = table(cut(wr), cut(g), cut(cr))
    assert blocks == T
    sgd_call(tab_s, T, blocks)
    rmsprop_call(tab_r, T, blocks)
    torch.cuda.synchronize()
    Wr, Cr = twin.rmsprop_update(W, G, C, LR, DECAY)
    assert same_bits(host(ws), twin.sgd_update(W, G, LR))
    assert same_bits(host(wr), Wr) and same_bits(host(cr), Cr)


def momentum_call(tab, ntens, blocks, gscale, lr=LR, mom=DECAY):
    lib.dk_sgd_momentum_multi_f32(tab.data_ptr(), ntens, blocks, float(lr), float(mom), float(gscale),
                                  stream_handle())


@pytest.mark.parametrize("gscale", [1.0, 0.5], ids=["plain", "grad_scale"])
def test_momentum_raw_entry_bit_for_bit(gscale):
    """dk_sgd_momentum_multi_f32 against its twin: g' = gscale * g (not at gscale = 1), d = (-lr) * g' +
    mom * v, w = w + d, v = d, one rounding per operation, nothing reduced: no tolerance.  Planted into
    the 4099-element tensor, on a velocity of 0: PLANTED's gradients (g = 0: the weight must not move;
    g = +-1e-20) and g = 1e-37 at index 7, whose product with lr is a denormal that must survive in v."""
    rng = np.random.default_rng(14)
    W = [rng.standard_normal(n).astype(np.float32) for n in SIZES]
    V = [rng.standard_normal(n).astype(np.float32) for n in SIZES]
    V[0][:] = 0  # a fresh velocity
    for i in (0, 5, 7, 300, 4096):
        V[-1][i] = 0
    ws, vs = [dev(w) for w in W], [dev(v) for v in V]
    gs = [torch.empty(n, dtype=torch.float32, device="cuda") for n in SIZES]
    tab, blocks = table(ws, gs, vs)
    W_first = [w.copy() for w in W]
    W_before = W_first[-1]
    for step in range(3):  # consecutive steps: the velocity carries over
        G = _inputs(rng, step)
        G[-1][7] = 1e-37
        for g, a in zip(gs, G):
            g.copy_(dev(a))
        momentum_call(tab, len(SIZES), blocks, gscale)
        torch.cuda.synchronize()
        for t, n in enumerate(SIZES):
            W[t], V[t] = twin.sgd_momentum_update(W[t], G[t], V[t], LR, DECAY, gscale)
            assert same_bits(host(vs[t]), V[t]), ("v", step, n)
            assert same_bits(host(ws[t]), W[t]), ("w", step, n)
            assert same_bits(host(gs[t]), G[t]), ("gradients are read only", step, n)
        w, v = host(ws[-1]), host(vs[-1])
        for i in (0, 4096):  # g = 0 on v = 0: nothing moves
            assert same_bits(w[i:i + 1], W_before[i:i + 1]) and v[i] == 0, (step, i)
        for i in (5, 300):  # the tiny step is kept in the velocity
            assert v[i] != 0 and abs(v[i]) < 1e-21, (step, i)
        # a denormal survived: not flushed (as bits: the host may compare denormals as zero)
        assert 0 < int(v.view(np.uint32)[7] & 0x7fffffff) < 0x00800000, step
    assert all(not same_bits(host(w), a) for w, a in zip(ws, W_first))  # and ordinary elements moved


def test_momentum_past_the_lds_table():
    """1025 tensors, 3 elements each: the owner search's linear fallback in the momentum kernel."""
    rng = np.random.default_rng(15)
    T, n = 1025, 3
    W = rng.standard_normal(T * n).astype(np.float32)
    G = rng.standard_normal(T * n).astype(np.float32)
    V = rng.standard_normal(T * n).astype(np.float32)
    w, g, v = dev(W), dev(G), dev(V)
    cut = lambda t: [t[i * n:(i + 1) * n] for i in range(T)]  # noqa: E731
    tab, blocks = table(cut(w), cut(g), cut(v))
    assert blocks == T
    momentum_call(tab, T, blocks, 0.5)
    torch.cuda.synchronize()
    W2, V2 = twin.sgd_momentum_update(W, G, V, LR, DECAY, 0.5)
    assert same_bits(host(w), W2) and same_bits(host(v), V2) and same_bits(host(g), G)
    assert not same_bits(W2, W)


def test_no_stray_writes():
    """Every w and c is carved out of a larger buffer between NaN guard words; the guards (and the
    gradients) are untouched."""
    rng = np.random.default_rng(13)
    guard = 64
    total = sum(n + guard for n in SIZES) + guard
    nan = np.float32(np.nan).view(np.uint32)

    def carve(values):
        buf = torch.full((total,), float("nan"), dtype=torch.float32, device="cuda")
        mask = np.ones(total, bool)
        views, off = [], guard
        for v in values:
            view = buf[off:off + v.size]
            view.copy_(dev(v))
            mask[off:off + v.size] = False
            views.append(view)
            off += v.size + guard
        return buf, views, mask

    W = [rng.standard_normal(n).astype(np.float32) for n in SIZES]
    G = [rng.standard_normal(n).astype(np.float32) for n in SIZES]
    C = [(rng.standard_normal(n) ** 2).astype(np.float32) for n in SIZES]
    bs, ws, mask = carve(W)
    br, wr, _ = carve(W)
    bc, cr, _ = carve(C)
    bg, gs, _ = carve(G)
    g_before = host(bg).view(np.uint32)
    tab_s, blocks = table(ws, gs)
    tab_r, _ = table(wr, gs, cr)
    sgd_call(tab_s, len(SIZES), blocks)
    rmsprop_call(tab_r, len(SIZES), blocks)
    torch.cuda.synchronize()
    for name, buf in (("sgd w", bs), ("rmsprop w", br), ("rmsprop c", bc)):
        b = host(buf).view(np.uint32)
        assert (b[mask] == nan).all(), name
        assert not np.isnan(host(buf)[~mask]).any(), name
    assert np.array_equal(host(bg).view(np.uint32), g_before)
    for t in range(len(SIZES)):  # and the carved tensors hold the update
        Wr, Cr = twin.rmsprop_update(W[t], G[t], C[t], LR, DECAY)
        assert same_bits(host(ws[t]), twin.sgd_update(W[t], G[t], LR))
        assert same_bits(host(wr[t]), Wr) and same_bits(host(cr[t]), Cr)


# ---- the table builder on the device ---------------------------------------------------------------

def test_device_table_rebuilds_only_on_change():
    """DeviceTable.ensure: the rows are this file's own statement of the layout; a second call with the
    same tensors keeps the device tensor and the signature object; a replaced pointer, a changed size or
    a flipped extra word (Adam's decay flag) rebuilds; sizes that disagree are refused."""
    from dorknet_amd._table import DeviceTable
    new = lambda n: torch.zeros(n, dtype=torch.float32, device="cuda")  # noqa: E731
    ws, gs, cs = [new(n) for n in SIZES], [new(n) for n in SIZES], [new(n) for n in SIZES]
    t = DeviceTable(256, "RMSProp", ("parameters, grads and caches", "grad / cache"), 3)
    assert t.ensure(list(zip(ws, gs, cs))) is True
    want, blocks = table(ws, gs, cs)
    assert torch.equal(t.rows, want) and (t.ntens, t.blocks) == (len(SIZES), blocks) and t.ptr == t.rows.data_ptr()
    rows, sig = t.rows, t.sig
    assert t.ensure(list(zip(ws, gs, cs))) is False and t.rows is rows and t.sig is sig
    cs[2] = cs[2].clone()  # a pointer
    assert t.ensure(list(zip(ws, gs, cs))) is True and t.rows is not rows and t.sig is not sig
    assert torch.equal(t.rows, table(ws, gs, cs)[0])
    ws[0], gs[0], cs[0] = new(300), new(300), new(300)  # a size: every later first_block moves
    assert t.ensure(list(zip(ws, gs, cs))) is True and torch.equal(t.rows, table(ws, gs, cs)[0])
    assert t.blocks == blocks + 1
    rows = t.rows
    gs[1] = new(SIZES[1] + 1)
    with pytest.raises(ValueError, match="^RMSProp: grad / cache size mismatch$"):
        t.ensure(list(zip(ws, gs, cs)))
    assert t.rows is rows  # a refused call leaves the table as it was
    # no state (plain SGD): 0 pointers
    s = DeviceTable(256, "SGD", ("parameters and grads", "grad"), 3)
    s.ensure([(w, g, None) for w, g in zip(ws, cs)])
    assert torch.equal(s.rows, table(ws, cs)[0])
    # an extra word per row
    a = DeviceTable(256, "Adam", ("parameters, grads and moments", "grad / moment"), 4)
    ms = [new(n) for n in (300, *SIZES[1:])]
    assert a.ensure([(w, c, m, c, 1) for w, c, m in zip(ws, cs, ms)]) is True
    assert a.rows.shape == (len(SIZES), 7) and a.rows[:, 6].tolist() == [1] * len(SIZES)
    assert a.rows[:, 5].tolist() == t.rows[:, 4].tolist() and a.rows[:, 2].tolist() == [m.data_ptr() for m in ms]
    rows = a.rows
    assert a.ensure([(w, c, m, c, 1) for w, c, m in zip(ws, cs, ms)]) is False and a.rows is rows
    assert a.ensure([(w, c, m, c, i & 1) for i, (w, c, m) in enumerate(zip(ws, cs, ms))]) is True
    assert a.rows is not rows and a.rows[:, 6].tolist() == [i & 1 for i in range(len(SIZES))]


# ---- through the layers ----------------------------------------------------------------------------

def _net(seed=20):
    """ConvLayer 3 -> 8 (3x3), BN, ReLU, a depthwise-separable ResidualBlock with a stride-2 skip
    projection, global average pooling, DenseLayer 8 -> 5."""
    from dorknet_amd.layers.activations import ReLu
    from dorknet_amd.layers.batch_norm import BatchNormLayer
    from dorknet_amd.layers.convolution import ConvLayer
    from dorknet_amd.layers.dense_layer import DenseLayer
    from dorknet_amd.layers.losses import SoftmaxWithCrossEntropy
    from dorknet_amd.layers.pooling import GlobalAveragePoolingLayer
    from examples.resnet18_depsep import ResNet18
    np.random.seed(seed)
    net = ResNet18("small", load_layers=False)
    net.add_layer(ConvLayer("conv", filter_block_shape=(8, 3, 3, 3), with_bias=False, stride=1, padding=1))
    net.add_layer(BatchNormLayer("conv_bn", input_dimension=4, incoming_chans=8))
    net.add_layer(ReLu("conv_relu"))
    net.add_res_block("res", (8, 8, 3, 3), downsample=True, depthwise_sep=True)
    net.add_layer(GlobalAveragePoolingLayer("pool"))
    net.add_layer(DenseLayer("dense", incoming_chans=8, output_dim=5))
    net.set_loss_layer(SoftmaxWithCrossEntropy("softmax"))
    return net


def _batch(seed, bf16=False):
    rng = np.random.default_rng(seed)
    X = dev(rng.uniform(-1, 1, size=(4, 3, 8, 8)))
    onehot = dev(np.eye(5, dtype=np.float32)[rng.integers(0, 5, 4)])
    return (X.to(torch.bfloat16) if bf16 else X), onehot


def _train_step(net, X, onehot):
    net.forward(X, onehot)
    net.backward()
    torch.cuda.synchronize()


def _expected(opt, lr=None, decay=None):
    """The twin applied to every listed (parameter, gradient, cache) as it is on the GPU now:
    {(layer name, param): (W, c or None)}."""
    lr = opt.learning_rate if lr is None else lr
    out = {}
    for layer in opt.learnable_layers:
        for k in layer.learned_params:
            W, g = host(layer.learned_params[k]), host(layer.grads[k])
            if isinstance(opt, RMSProp):
                W2, c2 = twin.rmsprop_update(W.ravel(), g.ravel(), host(opt.grad_cache[layer][k]).ravel(), lr,
                                             opt.decay_rate if decay is None else decay)
                out[(layer.layer_name, k)] = (W2.reshape(W.shape), c2.reshape(W.shape))
            else:
                out[(layer.layer_name, k)] = (twin.sgd_update(W.ravel(), g.ravel(), lr).reshape(W.shape), None)
    return out


def _check(opt, want, what):
    torch.cuda.synchronize()
    for layer in opt.learnable_layers:
        for k in layer.learned_params:
            W, c = want[(layer.layer_name, k)]
            assert same_bits(host(layer.learned_params[k]), W), (what, layer.layer_name, k)
            if c is not None:
                assert same_bits(host(opt.grad_cache[layer][k]), c), (what, "cache", layer.layer_name, k)


def _make(cls, net, **kw):
    return cls(net, 0.05, **kw) if cls is SGD else cls(net, 0.05, 0.9, **kw)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cls", [SGD, RMSProp], ids=["SGD", "RMSProp"])
def test_through_the_layers(cls, bf16):
    for flag in (False, True):
        net = _net()
        net.to_gpu()
        opt = _make(cls, net, update_skip_projections=flag)
        skip = net.layers[3].skip_projection
        assert skip.layer_name == "res_pw_skip" and ((skip in opt.learnable_layers) is flag)
        assert len(opt.learnable_layers) == 2 + 8 + 1 + flag  # conv, BN; the block's 8; dense [; the skip]
        skip0 = host(skip.learned_params["weights"])
        for step in range(3):
            X, onehot = _batch(30 + step, bf16)
            _train_step(net, X, onehot)
            assert all(p.dtype == torch.float32 and l.grads[k].dtype == torch.float32
                       for l in opt.learnable_layers for k, p in l.learned_params.items())
            want = _expected(opt)
            now = _weights(opt)
            moved = [k for k, (W, _) in want.items() if not same_bits(W, now[k])]
            assert 2 * len(moved) >= len(want), moved  # the step is not a no-op (checks the test, not the kernel)
            opt.update_weights()
            _check(opt, want, (flag, step))
        assert np.abs(host(skip.grads["weights"])).max() > 0
        assert same_bits(host(skip.learned_params["weights"]), skip0) is (not flag)


@pytest.mark.parametrize("cls", [SGD, RMSProp], ids=["SGD", "RMSProp"])
def test_scalars_travel_as_arguments_and_the_table_is_reused(cls):
    net = _net()
    net.to_gpu()
    opt = _make(cls, net)
    X, onehot = _batch(40)
    _train_step(net, X, onehot)
    opt.update_weights()
    tab, ptr = opt._table, opt._table.data_ptr()
    opt.multiply_learning_rate(0.5)
    assert opt.learning_rate == 0.025
    if cls is RMSProp:
        opt.decay_rate = 0.75
    _train_step(net, X, onehot)
    want = _expected(opt, lr=0.025, decay=0.75)
    assert any(not same_bits(W, _expected(opt, lr=0.05, decay=0.9)[k][0]) for k, (W, _) in want.items())
    opt.update_weights()
    _check(opt, want, "halved learning rate")
    assert opt._table is tab and opt._table.data_ptr() == ptr  # no rebuild
    # one parameter tensor replaced: the table is rebuilt and the update lands in the new tensor
    dense = net.layers[-1]
    old = dense.learned_params["weights"]
    old_bits = host(old)
    dense.learned_params["weights"] = old.clone()
    want = _expected(opt)
    opt.update_weights()
    _check(opt, want, "replaced tensor")
    assert opt._table is not tab
    assert same_bits(host(old), old_bits) and not same_bits(host(dense.learned_params["weights"]), old_bits)
    tab2 = opt._table
    opt.update_weights()
    assert opt._table is tab2


# ---- the state file ----------------------------------------------------------------------------------

def _state(opt):
    return {(l.layer_name, k): host(v) for l, d in opt.grad_cache.items() for k, v in d.items()}


def _weights(opt):
    return {(l.layer_name, k): host(v) for l in opt.learnable_layers for k, v in l.learned_params.items()}


@needs_h5
@pytest.mark.parametrize("cls,hyper", [(SGDMomentum, "momentum"), (RMSProp, "decay_rate")],
                         ids=["SGDMomentum", "RMSProp"])
def test_state_round_trip(cls, hyper, tmp_path):
    from dorknet_amd.network.feed_forward_network import FeedForwardNetwork
    net = _net()
    net.to_gpu()
    opt = cls(net, 0.05, 0.9)
    for step in range(2):
        _train_step(net, *_batch(50 + step))
        opt.update_weights()
    opt.multiply_learning_rate(0.5)
    _train_step(net, *_batch(52))  # gradients for the step both optimisers take below
    h5f, js, st = str(tmp_path / "w.h5"), str(tmp_path / "s.json"), str(tmp_path / "opt.h5")
    net.save_weights_to_h5(h5f)
    net.save_layer_structure_to_json(js)
    opt.save_state_to_h5(st)

    fresh = FeedForwardNetwork("x")
    fresh.load_network_from_json_and_h5(js, h5f)
    fresh.to_gpu()
    opt2 = cls(fresh, 0.5, 0.5)
    tensors = {(l.layer_name, k): v for l, d in opt2.grad_cache.items() for k, v in d.items()}
    assert all(not v.any() for v in _state(opt2).values())
    opt2.load_state_from_h5(st)
    assert all(opt2.grad_cache[l][k] is tensors[(l.layer_name, k)] for l in opt2.learnable_layers
               for k in opt2.grad_cache[l])  # loaded in place
    assert opt2.learning_rate == opt.learning_rate == 0.025 and getattr(opt2, hyper) == getattr(opt, hyper) == 0.9
    s1, s2 = _state(opt), _state(opt2)
    assert s1.keys() == s2.keys() and len(s1) == sum(len(l.learned_params) for l in opt.learnable_layers)
    assert all(same_bits(s1[k], s2[k]) for k in s1) and any(v.any() for v in s1.values())
    w1, w2 = _weights(opt), _weights(opt2)
    assert w1.keys() == w2.keys() and all(same_bits(w1[k], w2[k]) for k in w1)
    by_name = {l.layer_name: l for l in opt.learnable_layers}
    for l in opt2.learnable_layers:  # the first run's gradients
        for k in l.grads:
            l.grads[k].copy_(by_name[l.layer_name].grads[k])
    opt.update_weights()
    opt2.update_weights()
    torch.cuda.synchronize()
    w1b, w2b = _weights(opt), _weights(opt2)
    assert all(same_bits(w1b[k], w2b[k]) for k in w1b)
    assert 2 * sum(not same_bits(w1b[k], w1[k]) for k in w1) >= len(w1)  # and the step moved them
    s1, s2 = _state(opt), _state(opt2)
    assert all(same_bits(s1[k], s2[k]) for k in s1)


@needs_h5
def test_sgd_state_file_round_trips_its_attributes(tmp_path):
    net = _net()
    net.to_gpu()
    opt = SGD(net, 0.05, update_skip_projections=True)
    opt.multiply_learning_rate(0.5)
    st = str(tmp_path / "sgd.h5")
    opt.save_state_to_h5(st)
    with checkpoint.open_h5(st, "r") as f:
        a = f["optimiser"].attrs
        assert checkpoint._as_str(a["type"]) == "SGD" and float(a["learning_rate"]) == 0.025
        assert bool(a["update_skip_projections"]) is True and list(f["optimiser"].keys()) == []
    opt2 = SGD(net, 0.5, update_skip_projections=True)
    opt2.load_state_from_h5(st)
    assert opt2.learning_rate == 0.025
    with pytest.raises(ValueError):
        RMSProp(net, 0.5, 0.5, update_skip_projections=True).load_state_from_h5(st)
