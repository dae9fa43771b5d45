"""LARS on the GPU (dk_lars_norms_multi_f32, dk_lars_multi_f32; dorknet_amd/optimisers/LARS.py) against
the numpy twin (tests/_lars_twin.py).  The per-tensor norms are reductions: each is held to one fp32
spacing of numpy's fp64 norm (one rounding of an fp64 result) and to bit-identical repeats.  Everything
after them is single correctly rounded fp32 operations in a written order, so the ratio (from the
stored norms) and the update (from the stored ratio) are compared bit for bit: no tolerance."""
import numpy as np
import pytest
import torch

from dorknet_amd._hip import lib, stream_handle
from dorknet_amd.network import checkpoint
from dorknet_amd.optimisers import clip
from dorknet_amd.optimisers.LARS import LARS
from tests import _adam_twin as clip_twin
from tests import _lars_twin as twin

pytestmark = pytest.mark.gpu

CHUNK = 2048
# the chunk edges, a tensor of 257 partials (the final kernel's strided loop takes a second pass), and
# two small tensors that get an all-zero g and an all-zero w
SIZES = [1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5, 256 * CHUNK + 3, 300, CHUNK + 2, 10]
FLAGS = [1, 0, 1, 0, 1, 1, 1, 1, 1]
ZERO_G, ZERO_W, TINY = 6, 7, 8  # indices into SIZES
BIG = 4                         # g of this tensor holds 1e20, alone in the tensor's tail block
LR, MOM, TRUST, WD, EPS = 0.05, 0.9, 0.02, 0.01, 1e-8


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


def lars_table(ws, gs, vs, flags):
    """{w, g, v, n, first_block, flags} per tensor, CHUNK elements per block."""
    rows, block0 = [], 0
    for w, g, v, fl in zip(ws, gs, vs, flags):
        rows.append((w.data_ptr(), g.data_ptr(), v.data_ptr(), w.numel(), block0, fl))
        block0 += -(-w.numel() // CHUNK)
    return torch.as_tensor(np.array(rows, dtype=np.int64).reshape(-1, 6), device="cuda"), block0


def sgd_table(ws, gs, vs):
    """{w, g, v, n, first_block} per tensor, 256 elements per block (dk_sgd_momentum_multi_f32)."""
    rows, block0 = [], 0
    for w, g, v in zip(ws, gs, vs):
        rows.append((w.data_ptr(), g.data_ptr(), v.data_ptr(), w.numel(), block0))
        block0 += -(-w.numel() // 256)
    return torch.as_tensor(np.array(rows, dtype=np.int64).reshape(-1, 5), device="cuda"), block0


def norms_call(tab, ntens, blocks, stats, ws=None, trust=TRUST, wd=WD, eps=EPS):
    if ws is None:
        ws = torch.empty(max(16 * blocks, 16), dtype=torch.uint8, device="cuda")
    lib.dk_lars_norms_multi_f32(tab.data_ptr(), ntens, blocks, trust, wd, eps, stats.data_ptr(), ws.data_ptr(),
                                ws.numel() * ws.element_size(), stream_handle())
    torch.cuda.synchronize()
    return host(stats).reshape(-1, 4)


def update_call(tab, ntens, blocks, stats, lr=LR, mom=MOM, wd=WD):
    lib.dk_lars_multi_f32(tab.data_ptr(), ntens, blocks, lr, mom, wd, stats.data_ptr(), stream_handle())
    torch.cuda.synchronize()


def _inputs(seed):
    """(W, G, V) host lists over SIZES with the planted tensors and elements."""
    rng = np.random.default_rng(seed)
    W = [rng.standard_normal(n).astype(np.float32) for n in SIZES]
    V = [np.zeros(n, np.float32) for n in SIZES]
    W[ZERO_W][:] = 0.0
    W[5][:7] = 1e-30           # fp32 squares that vanish, among ordinary elements
    W[TINY][:] = 1e-30         # ... and alone: a norm the fp32 squares could not give
    return rng, W, _gradients(rng), V


def _gradients(rng):
    G = [rng.standard_normal(n).astype(np.float32) for n in SIZES]
    G[ZERO_G][:] = 0.0
    G[BIG][3 * CHUNK + 2] = 1e20  # its fp32 square overflows
    G[5][-3:] = -1e-30
    G[TINY][:] = -1e-30
    return G


def _check_stats(stats, W, G, flags, trust=TRUST, wd=WD, eps=EPS):
    """Norms within one fp32 spacing of numpy's fp64 norm; the ratio the twin's, from the stored norms."""
    assert stats.shape == (len(W), 4)
    for t, (w, g) in enumerate(zip(W, G)):
        for got, a in ((stats[t, 0], w), (stats[t, 1], g)):
            want = twin.norm_f64(a)
            assert abs(float(got) - want) <= np.spacing(np.float32(want)), (t, got, want)
        r = twin.trust_ratio(stats[t, 0], stats[t, 1], trust, wd, eps, adapt=bool(flags[t]))
        assert same_bits(stats[t, 2:3], [r]), (t, stats[t], r)
        assert same_bits(stats[t, 3:], [0.0])


def test_raw_entries_bit_for_bit():
    assert lib.dk_lars_workspace_bytes(7) == 112
    rng, W, G, V = _inputs(31)
    ws_, vs = [dev(a) for a in W], [dev(a) for a in V]
    gs = [torch.empty(n, dtype=torch.float32, device="cuda") for n in SIZES]
    tab, blocks = lars_table(ws_, gs, vs, FLAGS)
    assert blocks == sum(-(-n // CHUNK) for n in SIZES) == 1 + 1 + 1 + 2 + 4 + 257 + 1 + 2 + 1
    T = len(SIZES)
    stats = torch.full((T, 4), 7.0, dtype=torch.float32, device="cuda")
    W_first = [w.copy() for w in W]
    for step in range(5):  # consecutive steps: the velocities carry over, the norms of w move
        if step:
            G = _gradients(rng)
        for g, a in zip(gs, G):
            g.copy_(dev(a))
        s = norms_call(tab, T, blocks, stats)
        _check_stats(s, W, G, FLAGS)
        # the planted tensors did what they are there for
        assert s[ZERO_G, 1] == 0 and s[ZERO_G, 0] > 0 and s[ZERO_G, 2] == 1
        if step == 0:  # (ratio 1 then moves the zero weights: -lr * g)
            assert s[ZERO_W, 0] == 0 and s[ZERO_W, 1] > 0 and s[ZERO_W, 2] == 1
        assert 9e19 < s[BIG, 1] < 2e20 and 0 < s[BIG, 2] < 1e-18
        assert 0 < s[TINY, 0] < 1e-29 and 0 < s[TINY, 1] < 1e-29 and 0 < s[TINY, 2] < 1e-20
        assert all(s[t, 2] == 1 for t in range(T) if not FLAGS[t])
        assert all(s[t, 2] != 1 for t in range(T) if FLAGS[t] and t not in (ZERO_G, ZERO_W))
        if step == 0:
            # a second run gives the same bits, and the norms entry alone changes neither w nor g
            s2 = norms_call(tab, T, blocks, torch.zeros_like(stats))
            assert same_bits(s, s2)
            assert all(same_bits(host(w), a) for w, a in zip(ws_, W))
            assert all(same_bits(host(g), a) for g, a in zip(gs, G))
            assert all(not host(v).any() for v in vs)
        update_call(tab, T, blocks, stats)
        assert same_bits(host(stats).reshape(-1, 4), s)  # the update reads the stats only
        for k, n in enumerate(SIZES):
            W[k], V[k] = twin.lars_update(W[k], G[k], V[k], LR, MOM, WD, s[k, 2], adapt=bool(FLAGS[k]))
            assert same_bits(host(vs[k]), V[k]), ("v", step, n)
            assert same_bits(host(ws_[k]), W[k]), ("w", step, n)
            assert same_bits(host(gs[k]), G[k]), ("gradients are read only", step, n)
    # and the elements moved (but the 1e-30 weights, whose steps of 1e-55 vanish)
    assert all(not same_bits(host(w), a) for k, (w, a) in enumerate(zip(ws_, W_first)) if k != TINY)
    assert same_bits(host(ws_[TINY]), W_first[TINY])


def test_rows_that_are_not_adapted_are_sgd_momentum():
    """GPU against GPU, no twin: with no row adapted, dk_lars_multi_f32 leaves the bits that
    dk_sgd_momentum_multi_f32 with grad_scale 1 leaves on copies of the same data, whatever trust and
    weight_decay are."""
    rng, W, G, _ = _inputs(32)
    V = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in SIZES]
    a_w, a_g, a_v = ([dev(a) for a in X] for X in (W, G, V))
    b_w, b_g, b_v = ([dev(a) for a in X] for X in (W, G, V))
    T = len(SIZES)
    tab, blocks = lars_table(a_w, a_g, a_v, [0] * T)
    stats = torch.zeros((T, 4), dtype=torch.float32, device="cuda")
    s = norms_call(tab, T, blocks, stats)
    assert (s[:, 2] == 1).all() and (s[:, 1] > 0).sum() == T - 1
    update_call(tab, T, blocks, stats)
    stab, sblocks = sgd_table(b_w, b_g, b_v)
    lib.dk_sgd_momentum_multi_f32(stab.data_ptr(), T, sblocks, LR, MOM, 1.0, stream_handle())
    torch.cuda.synchronize()
    for k, n in enumerate(SIZES):
        assert same_bits(host(a_w[k]), host(b_w[k])), ("w", n)
        assert same_bits(host(a_v[k]), host(b_v[k])), ("v", n)
        assert same_bits(host(a_g[k]), G[k]) and not same_bits(host(a_w[k]), W[k]), n


def test_more_tensors_than_the_lds_table_holds():
    """1025 tensors of 3 elements (the index search's LDS table holds 1024: the linear fallback), every
    tensor at a scale of its own, so that a wrong index gives a wrong ratio."""
    rng = np.random.default_rng(33)
    T, n = 1025, 3
    wscale = np.repeat(1.0 + np.arange(T) / 64.0, n)
    gscale = np.repeat(0.5 + (np.arange(T) % 37) / 10.0, n)
    W = (wscale * rng.uniform(0.5, 1.0, T * n) * rng.choice([-1.0, 1.0], T * n)).astype(np.float32)
    G = (gscale * rng.uniform(0.5, 1.0, T * n) * rng.choice([-1.0, 1.0], T * n)).astype(np.float32)
    V = (0.1 * rng.standard_normal(T * n)).astype(np.float32)
    w, g, v = dev(W), dev(G), dev(V)
    cut = lambda t: [t[i * n:(i + 1) * n] for i in range(T)]  # noqa: E731
    flags = [1 if i % 3 else 0 for i in range(T)]
    tab, blocks = lars_table(cut(w), cut(g), cut(v), flags)
    assert blocks == T
    stats = torch.full((T, 4), 7.0, dtype=torch.float32, device="cuda")
    s = norms_call(tab, T, blocks, stats)
    _check_stats(s, cut(W), cut(G), flags)
    adapted = np.array(flags, bool)
    assert (s[~adapted, 2] == 1).all() and len(set(s[adapted, 2].tolist())) > 600  # distinct ratios
    assert same_bits(s, norms_call(tab, T, blocks, torch.zeros_like(stats)))
    update_call(tab, T, blocks, stats)
    W2, V2 = np.empty_like(W), np.empty_like(V)
    for t in range(T):
        sl = slice(t * n, (t + 1) * n)
        W2[sl], V2[sl] = twin.lars_update(W[sl], G[sl], V[sl], LR, MOM, WD, s[t, 2], adapt=bool(flags[t]))
    assert same_bits(host(w), W2) and same_bits(host(v), V2) and same_bits(host(g), G)
    # a neighbour's ratio would have shown: the update with the ratios shifted by one row differs
    W3 = np.concatenate([twin.lars_update(W[t * n:(t + 1) * n], G[t * n:(t + 1) * n], V[t * n:(t + 1) * n], LR, MOM,
                                          WD, s[t - 1, 2], adapt=bool(flags[t]))[0] for t in range(T)])
    assert (W3 != W2).reshape(T, n).any(axis=1).sum() > 600


def _carve(values, guard=64):
    """Each value carved out of one larger buffer between NaN guard words: (buffer, views, guard mask)."""
    total = sum(v.size + guard for v in values) + guard
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


NAN_BITS = np.float32(np.nan).view(np.uint32)


def _guards_intact(buf, mask):
    b = host(buf)
    return bool((b.view(np.uint32)[mask] == NAN_BITS).all()) and not np.isnan(b[~mask]).any()


def test_no_stray_writes():
    rng, W, G, _ = _inputs(34)
    V = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in SIZES]
    T = len(SIZES)
    bw, ws_, mask = _carve(W)
    bg, gs, _ = _carve(G)
    bv, vs, _ = _carve(V)
    bs, (stats,), smask = _carve([np.full(4 * T, 7.0, np.float32)])
    tab, blocks = lars_table(ws_, gs, vs, FLAGS)
    # the workspace: 16 bytes per block and not one more, NaN words behind it
    nws = 4 * blocks
    bws = torch.full((nws + 64,), float("nan"), dtype=torch.float32, device="cuda")
    wsmask = np.arange(nws + 64) >= nws
    assert 4 * nws == lib.dk_lars_workspace_bytes(blocks)
    before = [host(b).view(np.uint32) for b in (bw, bg, bv)]
    s = norms_call(tab, T, blocks, stats, ws=bws[:nws])
    _check_stats(s, W, G, FLAGS)
    assert _guards_intact(bs, smask)
    assert (host(bws).view(np.uint32)[wsmask] == NAN_BITS).all()  # (fp64 partials in front: any bits)
    for b, was in zip((bw, bg, bv), before):  # the norms entry alone: w, g and v bit-unchanged
        assert np.array_equal(host(b).view(np.uint32), was)
    update_call(tab, T, blocks, stats)
    assert _guards_intact(bw, mask) and _guards_intact(bv, mask)
    assert np.array_equal(host(bg).view(np.uint32), before[1])
    assert _guards_intact(bs, smask) and same_bits(host(stats).reshape(-1, 4), s)
    for k in range(T):  # and the carved tensors hold the update
        W2, V2 = twin.lars_update(W[k], G[k], V[k], LR, MOM, WD, s[k, 2], adapt=bool(FLAGS[k]))
        assert same_bits(host(ws_[k]), W2) and same_bits(host(vs[k]), V2)


# ---- through the layers ----------------------------------------------------------------------------

def _net(seed=20):
    """ConvLayer 3 -> 8 (3x3), BN, ReLU, a depthwise-separable ResidualBlock with a stride-2 skip
    projection, global average pooling, DenseLayer 8 -> 5 (the net of tests/test_gpu_optimisers.py)."""
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
    loss, _ = net.forward(X, onehot)
    net.backward()
    torch.cuda.synchronize()
    return float(loss)


def _snapshot(opt):
    torch.cuda.synchronize()
    return {(l.layer_name, k): (host(l.learned_params[k]), host(opt.grad_cache[l][k]))
            for l in opt.learnable_layers for k in l.learned_params}


def _grads(opt):
    return {(l.layer_name, k): host(l.grads[k]) for l in opt.learnable_layers for k in l.learned_params}


def _equal(a, b):
    return a.keys() == b.keys() and all(same_bits(x, y) for k in a for x, y in zip(a[k], b[k]))


def _replay(opt, before, grads, stats):
    """The twin's step from the state `before` with the gradients `grads` and the stored stats, after
    checking the stats against them: {(layer name, param): (W, v)}."""
    names = opt.stat_names
    assert list(before) == names and stats.shape == (len(names), 4)
    flags = [k in opt.adapt_params for _, k in names]
    _check_stats(stats, [before[key][0] for key in names], [grads[key] for key in names], flags,
                 opt.trust_coefficient, opt.weight_decay, opt.eps)
    out = {}
    for t, key in enumerate(names):
        W, v = before[key]
        W2, v2 = twin.lars_update(W.ravel(), grads[key].ravel(), v.ravel(), opt.learning_rate, opt.momentum,
                                  opt.weight_decay, stats[t, 2], adapt=flags[t])
        out[key] = (W2.reshape(W.shape), v2.reshape(W.shape))
    return out


def _check(opt, want, what):
    now = _snapshot(opt)
    for key in want:
        for name, x, y in zip("wv", now[key], want[key]):
            assert same_bits(x, y), (what, name, key)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_through_the_layers(bf16):
    net = _net()
    net.to_gpu()
    opt = LARS(net, 0.05, momentum=0.9, trust_coefficient=0.2, weight_decay=1e-4)
    X, onehot = _batch(30, bf16)
    losses = []
    for step in range(5):
        losses.append(_train_step(net, X, onehot))
        assert all(p.dtype == torch.float32 and l.grads[k].dtype == torch.float32
                   for l in opt.learnable_layers for k, p in l.learned_params.items())
        before, grads = _snapshot(opt), _grads(opt)
        opt.update_weights()
        stats = opt.last_stats
        assert isinstance(stats, torch.Tensor) and stats.is_cuda and tuple(stats.shape) == (len(opt.stat_names), 4)
        torch.cuda.synchronize()
        s = host(stats)
        want = _replay(opt, before, grads, s)
        _check(opt, want, step)
        assert _equal(_grads(opt), grads)  # the gradients are read only
        moved = [k for k in want if not same_bits(want[k][0], before[k][0])]
        assert 2 * len(moved) >= len(want), moved  # the step is not a no-op (checks the test, not the kernel)
        keys = [k for _, k in opt.stat_names]
        assert {"gamma", "beta", "bias", "weights"} <= set(keys)
        for t, k in enumerate(keys):  # BN's gamma and beta and the biases are not adapted
            assert bool(s[t, 2] == 1) == (k != "weights"), (opt.stat_names[t], s[t])
    flags = opt._table.cpu().numpy()[:, 5].tolist()  # bit 0 of the built rows
    assert flags == [1 if k == "weights" else 0 for k in keys]
    print("losses", losses)
    assert losses[-1] < losses[0]


def test_scalars_travel_as_arguments_and_the_table_is_reused():
    net = _net()
    net.to_gpu()
    opt = LARS(net, 0.05, trust_coefficient=0.2)
    X, onehot = _batch(40)
    _train_step(net, X, onehot)
    opt.update_weights()
    rows, stats, ws = opt._dev.rows, opt.last_stats, opt._ws
    ptrs = (rows.data_ptr(), stats.data_ptr(), ws.data_ptr())
    for change in ("learning_rate", "trust_coefficient", "weight_decay", "momentum", "eps"):
        setattr(opt, change, {"learning_rate": 0.025, "trust_coefficient": 0.1, "weight_decay": 0.02,
                              "momentum": 0.8, "eps": 1e-6}[change])
        _train_step(net, X, onehot)
        before, grads = _snapshot(opt), _grads(opt)
        opt.update_weights()
        # no rebuild and nothing allocated: the same table, stats tensor and workspace, where they were
        assert opt._dev.rows is rows and opt.last_stats is stats and opt._ws is ws
        assert (rows.data_ptr(), stats.data_ptr(), ws.data_ptr()) == ptrs
        _check(opt, _replay(opt, before, grads, host(opt.last_stats)), change)
    # one parameter tensor replaced: the table, the stats and the workspace are rebuilt, and the update
    # lands in the new tensor
    dense = net.layers[-1]
    old = dense.learned_params["weights"]
    old_bits = host(old)
    dense.learned_params["weights"] = old.clone()
    before, grads = _snapshot(opt), _grads(opt)
    opt.update_weights()
    _check(opt, _replay(opt, before, grads, host(opt.last_stats)), "replaced tensor")
    assert opt._dev.rows is not rows and opt.last_stats is not stats
    assert same_bits(host(old), old_bits) and not same_bits(host(dense.learned_params["weights"]), old_bits)
    rows2, stats2 = opt._dev.rows, opt.last_stats
    opt.update_weights()
    assert opt._dev.rows is rows2 and opt.last_stats is stats2


def test_measure_tensor_norms():
    net = _net()
    net.to_gpu()
    opt = LARS(net, 0.05, trust_coefficient=0.2, weight_decay=1e-4)
    for d in opt.grad_cache.values():  # velocities that are not zero
        for k in d:
            d[k].normal_()
    _train_step(net, *_batch(45))
    before, grads = _snapshot(opt), _grads(opt)
    assert opt.last_stats is None
    out = opt.measure_tensor_norms()
    assert out is opt.last_stats and out.is_cuda and tuple(out.shape) == (len(opt.stat_names), 4)
    assert _equal(_snapshot(opt), before) and _equal(_grads(opt), grads)  # w, v and g bit-unchanged
    s = host(out)
    _replay(opt, before, grads, s)  # checks the stats against numpy's norms and the twin's ratio
    assert (s[:, 0] > 0).any() and (s[:, 1] > 0).any()
    assert opt.measure_tensor_norms() is out and same_bits(host(out), s)
    # the update that follows uses the same table and stats tensor, and the same numbers
    rows = opt._dev.rows
    opt.update_weights()
    assert opt._dev.rows is rows and opt.last_stats is out and same_bits(host(out), s)
    _check(opt, _replay(opt, before, grads, s), "update after measuring")


def test_clip_grad_norm_then_update():
    """clip_grad_norm(opt, c) works unchanged on a LARS optimiser: the gradients are scaled in place by
    the clip twin's scale, and the update that follows is the LARS twin's on the scaled gradients."""
    net = _net()
    net.to_gpu()
    opt = LARS(net, 0.05, trust_coefficient=0.2, weight_decay=1e-4)
    _train_step(net, *_batch(60))
    opt.update_weights()
    _train_step(net, *_batch(61))
    G = _grads(opt)
    total = clip_twin.norm_f64(G.values())
    c = 0.5 * total
    norm = clip.clip_grad_norm(opt, c)
    assert abs(float(norm) - total) <= np.spacing(np.float32(total))
    s = clip_twin.clip_scale(host(norm), c)
    assert 0.4 < s < 0.6
    scaled = {key: clip_twin.scale_update(g, s) for key, g in G.items()}
    assert _equal({k: (v,) for k, v in _grads(opt).items()}, {k: (v,) for k, v in scaled.items()})
    before = _snapshot(opt)
    opt.update_weights()
    stats = host(opt.last_stats)
    _check(opt, _replay(opt, before, scaled, stats), "clipped step")  # gn is the scaled gradients'
    assert _equal({k: (v,) for k, v in _grads(opt).items()}, {k: (v,) for k, v in scaled.items()})


@needs_h5
def test_state_round_trip(tmp_path):
    from dorknet_amd.network.feed_forward_network import FeedForwardNetwork
    from dorknet_amd.optimisers.SGDMomentum import SGDMomentum
    net = _net()
    net.to_gpu()
    opt = LARS(net, 0.05, momentum=0.8, trust_coefficient=0.2, weight_decay=1e-4, eps=1e-7)
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
    opt2 = LARS(fresh, 0.5, momentum=0.5, trust_coefficient=0.5, weight_decay=0.5, eps=1e-3)
    tensors = {(l.layer_name, k): opt2.grad_cache[l][k] for l in opt2.learnable_layers for k in opt2.grad_cache[l]}
    assert not any(t.any() for t in tensors.values())
    opt2.load_state_from_h5(st)
    assert all(opt2.grad_cache[l][k] is tensors[(l.layer_name, k)]
               for l in opt2.learnable_layers for k in opt2.grad_cache[l])  # loaded in place
    assert opt2.learning_rate == opt.learning_rate == 0.025
    assert (opt2.momentum, opt2.trust_coefficient, opt2.weight_decay, opt2.eps) == (0.8, 0.2, 1e-4, 1e-7)
    s1 = _snapshot(opt)
    assert _equal(s1, _snapshot(opt2)) and any(v.any() for _, v in s1.values())
    by_name = {l.layer_name: l for l in opt.learnable_layers}
    for l in opt2.learnable_layers:  # the first run's gradients
        for k in l.grads:
            l.grads[k].copy_(by_name[l.layer_name].grads[k])
    opt.update_weights()
    opt2.update_weights()
    s1b, s2b = _snapshot(opt), _snapshot(opt2)
    assert _equal(s1b, s2b) and same_bits(host(opt.last_stats), host(opt2.last_stats))
    assert 2 * sum(not same_bits(s1b[k][0], s1[k][0]) for k in s1) >= len(s1)  # and the step moved them
    with pytest.raises(ValueError):  # the velocities alone would fit: the type tells the files apart
        SGDMomentum(fresh, 0.5, 0.5).load_state_from_h5(st)
