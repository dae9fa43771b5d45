"""Adam / AdamW and global-norm clipping on the GPU (dk_adam_multi_f32, dk_grad_norm_multi_f32,
dk_grad_scale_multi_f32; dorknet_amd/optimisers/Adam.py, clip.py) against the numpy twins
(tests/_adam_twin.py), bit for bit: every operation of an update is one correctly rounded fp32
operation and nothing is reduced, so there is no freedom of order and no tolerance.  A difference
means a contracted, reassociated or approximate operation.  Only the norm is a reduction: it is held
to 1 fp32 ulp of numpy's fp64 norm and to bit-identical repeats."""
import numpy as np
import pytest
import torch

from dorknet_amd._hip import lib, stream_handle
from dorknet_amd.network import checkpoint
from dorknet_amd.optimisers import clip
from dorknet_amd.optimisers.Adam import Adam, AdamW
from dorknet_amd.optimisers.RMSProp import RMSProp
from tests import _adam_twin as twin
from tests._optim_twin import ieee_host

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 1000, 4099]  # the block edges (256 elements per block) and a multi-block tail
DECAYED = [1, 0, 1, 0, 1, 0]            # flags bit 0 per tensor; the 4099-element tensor is not decayed
LR, B1, B2, EPS, WD = 0.01, 0.9, 0.999, 1e-8, 0.01
CHUNK = clip.CHUNK


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


def adam_table(ws, gs, ms, vs, flags):
    """{w, g, m, v, n, first_block, flags} per tensor, 256 elements per block."""
    rows, block0 = [], 0
    for w, g, m, v, fl in zip(ws, gs, ms, vs, flags):
        rows.append((w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), w.numel(), block0, fl))
        block0 += -(-w.numel() // 256)
    return torch.as_tensor(np.array(rows, dtype=np.int64).reshape(-1, 7), device="cuda"), block0


def grad_table(gs):
    """{g, n, first_block} per tensor, CHUNK elements per block."""
    rows, block0 = [], 0
    for g in gs:
        rows.append((g.data_ptr(), g.numel(), block0))
        block0 += -(-g.numel() // CHUNK)
    return torch.as_tensor(np.array(rows, dtype=np.int64).reshape(-1, 3), device="cuda"), block0


def adam_call(tab, ntens, blocks, t, scale_ptr=None, lr=LR, wd=WD):
    omb1, omb2, neg_step, sbc2, keep = twin.scalars(lr, B1, B2, wd, t)
    lib.dk_adam_multi_f32(tab.data_ptr(), ntens, blocks, B1, omb1, B2, omb2, neg_step, sbc2, EPS, keep, scale_ptr,
                          stream_handle())


# planted into the 4099-element tensor, three inside its tail block (4096..4098): index -> gradient
PLANTED = {0: 0.0, 4096: 0.0,            # g = 0 on fresh state: w unchanged
           5: 1e-20, 4097: -1e-20,       # g * g is a denormal: sqrt and the division see denormals
           300: 1e20, 4098: -1e20,       # g * g overflows: v = inf, the step is -+0, w unchanged
           7: 1e-39, 301: -1e-39}        # g itself is a denormal: so is m, and g * g is 0


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "grad_scale"])
def test_raw_entry_bit_for_bit(scaled):
    rng = np.random.default_rng(21)
    W = [rng.standard_normal(n).astype(np.float32) for n in SIZES]
    M = [np.zeros(n, np.float32) for n in SIZES]
    V = [np.zeros(n, np.float32) for n in SIZES]
    ws, ms, vs = [dev(a) for a in W], [dev(a) for a in M], [dev(a) for a in V]
    gs = [torch.empty(n, dtype=torch.float32, device="cuda") for n in SIZES]
    tab, blocks = adam_table(ws, gs, ms, vs, DECAYED)
    assert blocks == sum(-(-n // 256) for n in SIZES) == 1 + 1 + 1 + 2 + 4 + 17
    s = 0.37 if scaled else None
    scale = dev([s]) if scaled else None
    W_first = [w.copy() for w in W]
    W0 = W_first[-1]
    for t in range(1, 6):  # consecutive steps, t advancing: the state (inf included) carries over
        G = [rng.standard_normal(n).astype(np.float32) for n in SIZES]
        with ieee_host():  # (a flush-to-zero host would round the planted denormals to 0)
            for i, g in PLANTED.items():
                G[-1][i] = g
        for g, a in zip(gs, G):
            g.copy_(dev(a))
        adam_call(tab, len(SIZES), blocks, t, scale.data_ptr() if scaled else None)
        torch.cuda.synchronize()
        for k, n in enumerate(SIZES):
            W[k], M[k], V[k] = twin.adam_update(W[k], G[k], M[k], V[k], LR, B1, B2, EPS, WD, t,
                                                decay=bool(DECAYED[k]), scale=s)
            assert same_bits(host(ms[k]), M[k]), ("m", t, n)
            assert same_bits(host(vs[k]), V[k]), ("v", t, n)
            assert same_bits(host(ws[k]), W[k]), ("w", t, n)
            assert same_bits(host(gs[k]), G[k]), ("gradients are read only", t, n)
        w, m, v = host(ws[-1]), host(ms[-1]), host(vs[-1])
        for i in (0, 4096, 300, 4098):  # the planted cases did what they are there for, at every step
            assert same_bits(w[i:i + 1], W0[i:i + 1]), (t, i)
        assert v[0] == 0 and m[4096] == 0 and np.isinf(v[300]) and np.isinf(v[4098])
        for i in (5, 4097):  # a denormal survived (as bits: the host may compare denormals as zero)
            assert 0 < int(v.view(np.uint32)[i]) < 0x00800000, (t, i)
        for i in (7, 301):
            assert 0 < int(m.view(np.uint32)[i] & 0x7fffffff) < 0x00800000 and v[i] == 0, (t, i)
    assert all(not same_bits(host(w), a) for w, a in zip(ws, W_first))  # and ordinary elements moved


def test_more_tensors_than_the_lds_table_holds():
    """1025 tensors (the owner search's LDS table holds 1024: the linear fallback), 3 elements each."""
    rng = np.random.default_rng(22)
    T, n = 1025, 3
    W = rng.standard_normal(T * n).astype(np.float32)
    G = rng.standard_normal(T * n).astype(np.float32)
    M = (0.1 * rng.standard_normal(T * n)).astype(np.float32)
    V = (0.1 * rng.standard_normal(T * n) ** 2).astype(np.float32)
    w, g, m, v = dev(W), dev(G), dev(M), dev(V)
    cut = lambda t: [t[i * n:(i + 1) * n] for i in range(T)]  # noqa: E731
    flags = [i & 1 for i in range(T)]
    tab, blocks = adam_table(cut(w), cut(g), cut(m), cut(v), flags)
    assert blocks == T
    adam_call(tab, T, blocks, 3)
    gtab, gblocks = grad_table(cut(g))
    assert gblocks == T
    out = torch.zeros(2, dtype=torch.float32, device="cuda")
    ws = torch.empty(8 * gblocks, dtype=torch.uint8, device="cuda")
    lib.dk_grad_norm_multi_f32(gtab.data_ptr(), T, gblocks, 1.0, out.data_ptr(), ws.data_ptr(), ws.numel(),
                               stream_handle())
    lib.dk_grad_scale_multi_f32(gtab.data_ptr(), T, gblocks, out.data_ptr() + 4, stream_handle())
    torch.cuda.synchronize()
    dec = np.repeat(np.array(flags, bool), n)
    Wd, Md, Vd = twin.adam_update(W, G, M, V, LR, B1, B2, EPS, WD, 3, decay=True)
    Wn, _, _ = twin.adam_update(W, G, M, V, LR, B1, B2, EPS, WD, 3, decay=False)
    assert same_bits(host(w), np.where(dec, Wd, Wn)) and same_bits(host(m), Md) and same_bits(host(v), Vd)
    assert not same_bits(Wd, Wn)
    o = host(out)
    assert abs(float(o[0]) - twin.norm_f64([G])) <= np.spacing(np.float32(twin.norm_f64([G])))
    assert same_bits(o[1:], [twin.clip_scale(o[0], 1.0)]) and o[1] < 1
    assert same_bits(host(g), twin.scale_update(G, o[1]))


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
    rng = np.random.default_rng(23)
    W = [rng.standard_normal(n).astype(np.float32) for n in SIZES]
    G = [rng.standard_normal(n).astype(np.float32) for n in SIZES]
    M = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in SIZES]
    V = [(0.1 * rng.standard_normal(n) ** 2).astype(np.float32) for n in SIZES]
    bw, ws, mask = _carve(W)
    bg, gs, _ = _carve(G)
    bm, ms, _ = _carve(M)
    bv, vs, _ = _carve(V)
    g_before = host(bg).view(np.uint32)
    tab, blocks = adam_table(ws, gs, ms, vs, DECAYED)
    adam_call(tab, len(SIZES), blocks, 2)
    torch.cuda.synchronize()
    for name, buf in (("w", bw), ("m", bm), ("v", bv)):
        assert _guards_intact(buf, mask), name
    assert np.array_equal(host(bg).view(np.uint32), g_before)
    for k in range(len(SIZES)):  # and the carved tensors hold the update
        W2, M2, V2 = twin.adam_update(W[k], G[k], M[k], V[k], LR, B1, B2, EPS, WD, 2, decay=bool(DECAYED[k]))
        assert same_bits(host(ws[k]), W2) and same_bits(host(ms[k]), M2) and same_bits(host(vs[k]), V2)


# ---- the norm and the scale ------------------------------------------------------------------------

NORM_SIZES = [CHUNK - 1, CHUNK, CHUNK + 1, 1, 3 * CHUNK + 5]


def _norm_inputs(seed):
    rng = np.random.default_rng(seed)
    G = [rng.standard_normal(n).astype(np.float32) for n in NORM_SIZES]
    G[2][CHUNK] = 1e20          # its fp32 square overflows; alone in the tensor's second block
    G[0][:7] = 1e-30            # their fp32 squares vanish
    G[4][-3:] = -1e-30
    return G


def _norm_call(tab, ntens, blocks, max_norm, out, ws=None):
    ws = torch.empty(max(8 * blocks, 8), dtype=torch.uint8, device="cuda") if ws is None else ws
    lib.dk_grad_norm_multi_f32(tab.data_ptr(), ntens, blocks, float(max_norm), out.data_ptr(), ws.data_ptr(),
                               ws.numel(), stream_handle())
    torch.cuda.synchronize()
    return host(out)


def test_norm():
    assert lib.dk_grad_norm_workspace_bytes(7) == 56
    for big in (True, False):
        G = _norm_inputs(24)
        if not big:
            G[2][CHUNK] = 0.5
        gs = [dev(a) for a in G]
        tab, blocks = grad_table(gs)
        assert blocks == 1 + 1 + 2 + 1 + 4
        want = twin.norm_f64(G)
        assert np.isfinite(np.float32(want)) and (want > 9e19) is big
        out = torch.full((2,), 7.0, dtype=torch.float32, device="cuda")
        c = 0.25 * want  # below the norm: the scale is not 1
        o = _norm_call(tab, len(gs), blocks, c, out)
        assert abs(float(o[0]) - want) <= np.spacing(np.float32(want)), (o[0], want)
        assert same_bits(o[1:], [twin.clip_scale(o[0], c)]) and 0.2 < o[1] < 0.3
        o2 = _norm_call(tab, len(gs), blocks, c, torch.zeros_like(out))
        assert same_bits(o, o2)  # bit-identical from run to run
        for measure_only in (0.0, -1.0, float("inf")):
            o3 = _norm_call(tab, len(gs), blocks, measure_only, out)
            assert same_bits(o3[:1], o[:1]) and o3[1] == 1
        o4 = _norm_call(tab, len(gs), blocks, 4 * want, out)  # above the norm: no clipping
        assert o4[1] == 1 and same_bits(o4[:1], o[:1])
        assert all(same_bits(host(g), a) for g, a in zip(gs, G))  # the norm reads only
    # the tiny terms count: alone they give a norm the fp32 squares could not
    tiny = [dev(np.full(10, 1e-30, np.float32))]
    tab, blocks = grad_table(tiny)
    o = _norm_call(tab, 1, blocks, 1.0, torch.zeros(2, dtype=torch.float32, device="cuda"))
    want = twin.norm_f64([np.full(10, 1e-30, np.float32)])
    assert o[0] > 0 and abs(float(o[0]) - want) <= np.spacing(np.float32(want)) and o[1] == 1


def test_scale():
    G = _norm_inputs(25)
    G[2][CHUNK] = 3.0
    bg, gs, mask = _carve(G)
    tab, blocks = grad_table(gs)
    before = host(bg).view(np.uint32)
    one, s = dev([1.0]), dev([0.3])
    lib.dk_grad_scale_multi_f32(tab.data_ptr(), len(gs), blocks, one.data_ptr(), stream_handle())
    torch.cuda.synchronize()
    assert np.array_equal(host(bg).view(np.uint32), before)  # a scale of 1 changes no bit
    lib.dk_grad_scale_multi_f32(tab.data_ptr(), len(gs), blocks, s.data_ptr(), stream_handle())
    torch.cuda.synchronize()
    assert _guards_intact(bg, mask)
    for g, a in zip(gs, G):
        assert same_bits(host(g), twin.scale_update(a, 0.3)) and not same_bits(host(g), a)


def test_norm_and_scale_past_the_lds_table():
    """1025 gradient tensors, 3 elements each (the owner search's linear fallback over 24-byte rows): what
    test_norm and test_scale assert."""
    rng = np.random.default_rng(26)
    T, n = 1025, 3
    G = rng.standard_normal(T * n).astype(np.float32)
    G[:2] = 1e-30  # their fp32 squares vanish
    bg, (g,), mask = _carve([G])
    tab, blocks = grad_table([g[i * n:(i + 1) * n] for i in range(T)])
    assert blocks == T
    want = twin.norm_f64([G])
    c = 0.25 * want
    out = torch.full((2,), 7.0, dtype=torch.float32, device="cuda")
    o = _norm_call(tab, T, blocks, c, out)
    assert abs(float(o[0]) - want) <= np.spacing(np.float32(want)), (o[0], want)
    assert same_bits(o[1:], [twin.clip_scale(o[0], c)]) and 0.2 < o[1] < 0.3
    assert same_bits(o, _norm_call(tab, T, blocks, c, torch.zeros_like(out)))  # bit-identical from run to run
    o3 = _norm_call(tab, T, blocks, 0.0, out)  # measure only
    assert same_bits(o3[:1], o[:1]) and o3[1] == 1
    assert same_bits(host(g), G)  # the norm reads only
    one, s = dev([1.0]), dev([0.3])
    lib.dk_grad_scale_multi_f32(tab.data_ptr(), T, blocks, one.data_ptr(), stream_handle())
    torch.cuda.synchronize()
    assert same_bits(host(g), G)  # a scale of 1 changes no bit
    lib.dk_grad_scale_multi_f32(tab.data_ptr(), T, blocks, s.data_ptr(), stream_handle())
    torch.cuda.synchronize()
    assert _guards_intact(bg, mask)
    assert same_bits(host(g), twin.scale_update(G, 0.3)) and not same_bits(host(g), G)


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
    net.forward(X, onehot)
    net.backward()
    torch.cuda.synchronize()


def _expected(opt, t, scale=None, grads=None):
    """The twin applied to every listed (parameter, gradient, m, v) as it is on the GPU now, for step
    number t: {(layer name, param): (W, m, v)}."""
    out = {}
    for layer in opt.learnable_layers:
        for k in layer.learned_params:
            W = host(layer.learned_params[k])
            g = host(layer.grads[k]) if grads is None else grads[(layer.layer_name, k)]
            W2, m2, v2 = twin.adam_update(W.ravel(), g.ravel(), host(opt.m[layer][k]).ravel(),
                                          host(opt.v[layer][k]).ravel(), opt.learning_rate, opt.beta1, opt.beta2,
                                          opt.eps, opt.weight_decay, t, decay=k in opt.decay_params, scale=scale)
            out[(layer.layer_name, k)] = tuple(a.reshape(W.shape) for a in (W2, m2, v2))
    return out


def _snapshot(opt):
    torch.cuda.synchronize()
    return {(l.layer_name, k): (host(l.learned_params[k]), host(opt.m[l][k]), host(opt.v[l][k]))
            for l in opt.learnable_layers for k in l.learned_params}


def _equal(a, b):
    return a.keys() == b.keys() and all(same_bits(x, y) for k in a for x, y in zip(a[k], b[k]))


def _check(opt, want, what):
    now = _snapshot(opt)
    for key in want:
        for name, x, y in zip("wmv", now[key], want[key]):
            assert same_bits(x, y), (what, name, key)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("wd", [0.0, 0.01], ids=["Adam", "AdamW"])
def test_through_the_layers(wd, bf16):
    for flag in (False, True):
        net = _net()
        net.to_gpu()
        opt = (AdamW(net, 0.05, wd, update_skip_projections=flag) if wd
               else Adam(net, 0.05, update_skip_projections=flag))
        skip = net.layers[3].skip_projection
        assert skip.layer_name == "res_pw_skip" and ((skip in opt.learnable_layers) is flag)
        assert len(opt.learnable_layers) == 2 + 8 + 1 + flag  # conv, BN; the block's 8; dense [; the skip]
        skip0 = host(skip.learned_params["weights"])
        for step in range(3):
            _train_step(net, *_batch(30 + step, bf16))
            assert all(p.dtype == torch.float32 and l.grads[k].dtype == torch.float32
                       for l in opt.learnable_layers for k, p in l.learned_params.items())
            want = _expected(opt, step + 1)
            before = _snapshot(opt)
            moved = [k for k in want if not same_bits(want[k][0], before[k][0])]
            assert 2 * len(moved) >= len(want), moved  # the step is not a no-op (checks the test, not the kernel)
            opt.update_weights()
            assert opt.step_count == step + 1
            _check(opt, want, (flag, step))
            if wd:  # gamma, beta and bias are not decayed, the weights are
                undecayed = _expected_without_decay(opt, before, step + 1)
                for key in want:
                    assert same_bits(want[key][0], undecayed[key]) is (key[1] != "weights"), key
        flags = opt._table.cpu().numpy()[:, 6].tolist()  # bit 0 of the built rows: decay the weights only
        keys = [k for l in opt.learnable_layers for k in l.learned_params]
        assert flags == [1 if k == "weights" else 0 for k in keys] and {"gamma", "beta", "bias"} <= set(keys)
        assert np.abs(host(skip.grads["weights"])).max() > 0
        assert same_bits(host(skip.learned_params["weights"]), skip0) is (not flag)


def _expected_without_decay(opt, before, t):
    """The step from the state `before` with no tensor decayed: {(layer name, param): W}."""
    out = {}
    for layer in opt.learnable_layers:
        for k in layer.learned_params:
            W, m, v = before[(layer.layer_name, k)]
            out[(layer.layer_name, k)] = twin.adam_update(
                W.ravel(), host(layer.grads[k]).ravel(), m.ravel(), v.ravel(), opt.learning_rate, opt.beta1,
                opt.beta2, opt.eps, opt.weight_decay, t, decay=False)[0].reshape(W.shape)
    return out


def _copy_state(src, dst):
    """dst's parameters, gradients, m, v and step_count become src's (two optimisers over two equal nets)."""
    by_name = {l.layer_name: l for l in src.learnable_layers}
    for l in dst.learnable_layers:
        s = by_name[l.layer_name]
        for k in l.learned_params:
            l.learned_params[k].copy_(s.learned_params[k])
            l.grads[k].copy_(s.grads[k])
            dst.m[l][k].copy_(src.m[s][k])
            dst.v[l][k].copy_(src.v[s][k])
    dst.step_count = src.step_count


@pytest.mark.parametrize("cls", [Adam, RMSProp], ids=["Adam", "RMSProp"])
def test_clip_grad_norm_through_the_layers(cls):
    """clip_grad_norm on an optimiser's gradients: the norm within 1 fp32 ulp of numpy's fp64 norm, the
    gradients scaled by the twin's scale, bit for bit; a max_norm above the norm changes nothing."""
    net = _net()
    net.to_gpu()
    opt = Adam(net, 0.05) if cls is Adam else RMSProp(net, 0.05, 0.9)
    _train_step(net, *_batch(60))
    G = {(l.layer_name, k): host(l.grads[k]) for l in opt.learnable_layers for k in l.grads}
    want = twin.norm_f64(G.values())
    norm = clip.clip_grad_norm(opt, 4 * want)
    assert isinstance(norm, torch.Tensor) and norm.is_cuda and norm.dim() == 0
    assert abs(float(norm) - want) <= np.spacing(np.float32(want))
    assert all(same_bits(host(l.grads[k]), G[(l.layer_name, k)]) for l in opt.learnable_layers for k in l.grads)
    st = opt._clip_state
    tab, ws = st.table.rows, st.ws
    norm = clip.clip_grad_norm(opt, 0.5 * want)
    assert opt._clip_state is st and st.table.rows is tab and st.ws is ws  # the table and the workspace are reused
    s = twin.clip_scale(host(norm), 0.5 * want)
    assert 0.4 < s < 0.6 and same_bits(host(st.out)[1:], [s])
    for l in opt.learnable_layers:
        for k in l.grads:
            assert same_bits(host(l.grads[k]), twin.scale_update(G[(l.layer_name, k)], s)), (l.layer_name, k)
    # a replaced gradient tensor rebuilds the table
    dense = net.layers[-1]
    dense.grads["weights"] = dense.grads["weights"].clone()
    clip.clip_grad_norm(opt, 0.0)
    assert opt._clip_state.table.rows is not tab


@pytest.mark.parametrize("wd", [0.0, 0.01], ids=["Adam", "AdamW"])
def test_fused_clipping(wd):
    """Adam(max_grad_norm=c).update_weights() == clip_grad_norm(opt, c) followed by a plain update from
    the same state, bit for bit, with c below the measured norm."""
    net_a, net_b = _net(), _net()
    net_a.to_gpu()
    net_b.to_gpu()
    plain = Adam(net_b, 0.05, weight_decay=wd)
    for step in range(2):  # a state with history
        _train_step(net_b, *_batch(70 + step))
        plain.update_weights()
    _train_step(net_b, *_batch(72))
    G = {(l.layer_name, k): host(l.grads[k]) for l in plain.learnable_layers for k in l.grads}
    c = 0.5 * twin.norm_f64(G.values())
    fused = Adam(net_a, 0.05, weight_decay=wd, max_grad_norm=c)
    _copy_state(plain, fused)
    assert _equal(_snapshot(plain), _snapshot(fused)) and fused.step_count == 2
    fused.update_weights()
    norm = clip.clip_grad_norm(plain, c)
    plain.update_weights()
    torch.cuda.synchronize()
    assert _equal(_snapshot(plain), _snapshot(fused))
    assert fused.last_grad_norm.is_cuda and fused.last_grad_norm.dim() == 0
    assert same_bits(host(fused.last_grad_norm), host(norm)) and float(norm) > c
    s = host(fused._clip_state.out)[1]
    assert 0.4 < s < 0.6 and same_bits([s], [twin.clip_scale(host(norm), c)])
    # the fused update leaves the gradients as they were; and it is the twin's step with that scale
    by_name = {l.layer_name: l for l in fused.learnable_layers}
    assert all(same_bits(host(by_name[n].grads[k]), g) for (n, k), g in G.items())
    _copy_state(plain, fused)
    for l in fused.learnable_layers:
        for k in l.grads:
            l.grads[k].copy_(dev(G[(l.layer_name, k)]))
    want = _expected(fused, 4, scale=twin.clip_scale(host(norm), c))
    fused.update_weights()
    _check(fused, want, "fused step against the twin")


def test_scalars_travel_as_arguments_and_the_table_is_reused():
    net = _net()
    net.to_gpu()
    opt = Adam(net, 0.05, weight_decay=0.01, max_grad_norm=1e9)
    X, onehot = _batch(40)
    _train_step(net, X, onehot)
    opt.update_weights()
    tab, ptr, st = opt._table, opt._table.data_ptr(), opt._clip_state
    opt.multiply_learning_rate(0.5)
    opt.beta1, opt.beta2, opt.eps, opt.weight_decay = 0.8, 0.99, 1e-6, 0.02
    opt.step_count = 6
    _train_step(net, X, onehot)
    want = _expected(opt, 7, scale=1.0)
    opt.update_weights()
    _check(opt, want, "changed scalars")
    assert opt.step_count == 7 and opt.learning_rate == 0.025
    assert opt._table is tab and opt._table.data_ptr() == ptr and opt._clip_state is st  # no rebuild
    # one parameter tensor replaced: the table is rebuilt and the update lands in the new tensor
    dense = net.layers[-1]
    old = dense.learned_params["weights"]
    old_bits = host(old)
    dense.learned_params["weights"] = old.clone()
    want = _expected(opt, 8, scale=1.0)
    opt.update_weights()
    _check(opt, want, "replaced tensor")
    assert opt._table is not tab and opt._clip_state is st  # the gradients did not move
    assert same_bits(host(old), old_bits) and not same_bits(host(dense.learned_params["weights"]), old_bits)
    tab2 = opt._table
    opt.update_weights()
    assert opt._table is tab2


@needs_h5
@pytest.mark.parametrize("cls", [Adam, AdamW], ids=["Adam", "AdamW"])
def test_state_round_trip(cls, tmp_path):
    from dorknet_amd.network.feed_forward_network import FeedForwardNetwork
    net = _net()
    net.to_gpu()
    opt = cls(net, 0.05, weight_decay=0.01)
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
    opt2 = cls(fresh, 0.5, weight_decay=0.5, beta1=0.5, beta2=0.5, eps=1e-3)
    tensors = {(l.layer_name, k, s): state[l][k] for s, state in (("m", opt2.m), ("v", opt2.v))
               for l in opt2.learnable_layers for k in state[l]}
    assert not any(t.any() for t in tensors.values()) and opt2.step_count == 0
    opt2.load_state_from_h5(st)
    assert all(state[l][k] is tensors[(l.layer_name, k, s)] for s, state in (("m", opt2.m), ("v", opt2.v))
               for l in opt2.learnable_layers for k in state[l])  # loaded in place
    assert opt2.step_count == opt.step_count == 2 and opt2.learning_rate == opt.learning_rate == 0.025
    assert (opt2.beta1, opt2.beta2, opt2.eps, opt2.weight_decay) == (0.9, 0.999, 1e-8, 0.01)
    s1 = _snapshot(opt)
    assert _equal(s1, _snapshot(opt2)) and any(m.any() for _, m, _ in s1.values())
    by_name = {l.layer_name: l for l in opt.learnable_layers}
    for l in opt2.learnable_layers:  # the first run's gradients
        for k in l.grads:
            l.grads[k].copy_(by_name[l.layer_name].grads[k])
    opt.update_weights()
    opt2.update_weights()
    s1b, s2b = _snapshot(opt), _snapshot(opt2)
    assert _equal(s1b, s2b) and opt2.step_count == 3
    assert 2 * sum(not same_bits(s1b[k][0], s1[k][0]) for k in s1) >= len(s1)  # and the step moved them
    with pytest.raises(ValueError):  # Adam and AdamW are told apart
        (AdamW(fresh, 0.5, 0.5) if cls is Adam else Adam(fresh, 0.5)).load_state_from_h5(st)
