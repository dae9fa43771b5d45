"""MaxPoolLayer on the GPU (dk_maxpool_*, dorknet_amd/csrc/maxpool.hip).

Max and copy are exact, so every comparison here is bitwise -- fp32 as its int32 bits, bf16 as its
int16 bits -- against the numpy restatement of the rules (tests/_maxpool_twin.py), and fused (BN on
load) against DORKNET_FUSE=0.  Only the whole-network comparison with the fp64 oracle has a tolerance
(the project's normwise 1e-4 for the other layers' arithmetic), with the pools' locations replayed and
every disagreement with the fp64 arg-max asserted to be a tie.
"""
import numpy as np
import pytest
import torch

from dorknet_amd._hip import HipError, lib, stream_handle
from tests._maxpool_twin import OMaxPool, pool_bwd, pool_fwd, windows

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
DTYPES = [torch.float32, BF16]
# (N, C, H, W, stride)
CASES = [
    (2, 3, 7, 9, 2),      # scalar channels, a remainder row and column
    (2, 5, 10, 11, 3),    # stride 3, scalar channels, remainders 1 and 2
    (1, 4, 8, 8, 4),      # the generic-stride kernel on the vector path
    (2, 8, 6, 6, 1),      # stride 1: the identity
    (2, 68, 14, 14, 2),   # vector path, C not a multiple of 64
    (2, 64, 56, 56, 2),   # more than one block per image
    (1, 12, 33, 17, 16),  # the largest stride, a remainder row and column
    (1, 8, 7, 11, 3),     # stride 3 on the vector path, remainders 1 and 2
]


def bits(t):
    """The stored bits of a (logically NCHW) tensor, as a numpy integer array."""
    t = t.detach().contiguous()
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32).cpu().numpy()


def np_bits(a, dtype):
    """The bits a float32 numpy array has when stored as `dtype` (exact for the values used here)."""
    return bits(torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dtype))


def stored(a, dtype):
    """`a` (float32 numpy) rounded to what `dtype` storage holds, as float32 numpy."""
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dtype).float().numpy()


def cl(a, dtype):
    """numpy NCHW -> a channels-last device tensor of `dtype`."""
    t = torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda").to(dtype)
    return t.contiguous(memory_format=torch.channels_last)


def inputs(case, kind, dtype):
    N, C, H, W, s = case
    rng = np.random.RandomState(sum(case) + (kind == "continuous"))
    if kind == "tied":
        X = rng.randint(-1, 3, size=(N, C, H, W)).astype(np.float32)  # {-1, 0, 1, 2}: ties dominate
    else:
        X = stored(rng.randn(N, C, H, W), dtype)
    dY = stored(rng.randn(N, C, H // s, W // s), dtype)
    return X, dY


def pool(stride):
    from dorknet_amd.layers.pooling import MaxPoolLayer
    l = MaxPoolLayer("pool", stride=stride)
    l.to_gpu()
    return l


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["tied", "continuous"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_layer_matches_twin_bitwise(case, kind, dtype):
    N, C, H, W, s = case
    X, dY = inputs(case, kind, dtype)
    Y, idx = pool_fwd(X, s)
    dX = pool_bwd(idx, dY, s, H, W)
    layer = pool(s)
    # the tied run hands the layer plain NCHW tensors (its own layout conversion), the other channels-last
    x = cl(X, dtype) if kind == "continuous" else torch.as_tensor(X, device="cuda").to(dtype)
    dy = cl(dY, dtype) if kind == "continuous" else torch.as_tensor(dY, device="cuda").to(dtype)
    y = layer.forward(x)
    assert y.dtype == dtype and tuple(y.shape) == Y.shape and y.is_contiguous(memory_format=torch.channels_last)
    assert layer.max_locs.dtype == torch.uint8
    dx = layer.backward(dy)
    assert dx.dtype == dtype and tuple(dx.shape) == X.shape and dx.is_contiguous(memory_format=torch.channels_last)
    torch.cuda.synchronize()
    assert np.array_equal(bits(y), np_bits(Y, dtype))
    assert np.array_equal(layer.max_locs.contiguous().cpu().numpy(), idx)
    assert np.array_equal(bits(dx), np_bits(dX, dtype))
    # the raw entry point into a dx pre-filled with NaN: an element the kernel leaves unwritten
    # (a remainder row or column, say) would still be NaN
    dyc, dxn = cl(dY, dtype), cl(np.full(X.shape, np.nan), dtype)
    bwd = lib.dk_maxpool_bwd_bf16 if dtype == BF16 else lib.dk_maxpool_bwd_f32
    bwd(dyc.data_ptr(), layer.max_locs.data_ptr(), N, H, W, C, s, dxn.data_ptr(), stream_handle())
    torch.cuda.synchronize()
    assert not bool(torch.isnan(dxn).any())
    assert np.array_equal(bits(dxn), np_bits(dX, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_misaligned_pointers_take_the_scalar_path(dtype):
    """C % 4 == 0 but x / y / dx one element off a vector boundary and idx one byte off a word."""
    N, C, H, W, s = 2, 8, 5, 6, 2
    X, dY = inputs((N, C, H, W, s), "tied", dtype)
    Y, idx = pool_fwd(X, s)
    dX = pool_bwd(idx, dY, s, H, W)
    OH, OW = H // s, W // s
    nhwc = lambda a: np.ascontiguousarray(a.transpose(0, 2, 3, 1))  # noqa: E731

    def off(n, dt, fill=None):
        buf = torch.empty(n + 1, dtype=dt, device="cuda")
        if fill is not None:
            buf[1:] = torch.as_tensor(fill.ravel(), device="cuda").to(dt)
        return buf, buf[1:]

    _, x = off(X.size, dtype, nhwc(X))
    _, dy = off(dY.size, dtype, nhwc(dY))
    _, y = off(Y.size, dtype)
    _, loc = off(Y.size, torch.uint8)
    _, dx = off(X.size, dtype, np.full(X.size, np.nan, dtype=np.float32))
    fwd, bwd = ((lib.dk_maxpool_fwd_bf16, lib.dk_maxpool_bwd_bf16) if dtype == BF16 else
                (lib.dk_maxpool_fwd_f32, lib.dk_maxpool_bwd_f32))
    st = stream_handle()
    fwd(x.data_ptr(), N, H, W, C, s, y.data_ptr(), loc.data_ptr(), st)
    bwd(dy.data_ptr(), loc.data_ptr(), N, H, W, C, s, dx.data_ptr(), st)
    torch.cuda.synchronize()
    assert np.array_equal(bits(y).reshape(N, OH, OW, C), np_bits(nhwc(Y), dtype))
    assert np.array_equal(loc.cpu().numpy().reshape(N, OH, OW, C), nhwc(idx))
    assert np.array_equal(bits(dx).reshape(N, H, W, C), np_bits(nhwc(dX), dtype))


def test_element_index_past_2_31():
    """An input of more than 2^31 elements (bf16, 2 x 64 x 4101 x 4099, stride 2, a remainder row and
    column): every element index is 64-bit.  Checked on the device with torch's elementwise ops over
    the four strided window views (max, compare and select are exact)."""
    N, C, H, W, s = 2, 64, 4101, 4099, 2
    assert N * C * H * W > 2 ** 31
    OH, OW = H // s, W // s
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.empty((N, C, H, W), dtype=BF16, device="cuda", memory_format=torch.channels_last)
    x.copy_(torch.randint(-1, 3, (N, C, H, W), dtype=torch.int8, device="cuda", generator=g))
    dy = torch.empty((N, C, OH, OW), dtype=BF16, device="cuda", memory_format=torch.channels_last)
    dy.copy_(torch.randint(1, 100, (N, C, OH, OW), dtype=torch.int8, device="cuda", generator=g))  # never 0
    layer = pool(s)
    y = layer.forward(x)
    dx = layer.backward(dy)
    idx = layer.max_locs
    v = [x[:, :, m:OH * s:s, n:OW * s:s] for m in range(s) for n in range(s)]
    best, loc = v[0].clone(), torch.zeros_like(idx)
    for k in range(1, s * s):
        better = v[k] > best
        best = torch.where(better, v[k], best)
        loc.masked_fill_(better, k)
    assert torch.equal(y, best) and torch.equal(idx, loc)
    zero = torch.zeros((), dtype=BF16, device="cuda")
    for k in range(s * s):
        m, n = divmod(k, s)
        assert torch.equal(dx[:, :, m:OH * s:s, n:OW * s:s], torch.where(idx == k, dy, zero)), k
    assert not bool(dx[:, :, OH * s:, :].any()) and not bool(dx[:, :, :, OW * s:].any())
    # the last image's last window, spelled out: the far end of every buffer
    assert float(y[-1, -1, -1, -1]) == float(x[-1, -1, H - 3:H - 1, W - 3:W - 1].max())


def test_no_output_pixel_is_refused():
    """(1, 12, 33, 5) at stride 16: OW == 0."""
    layer = pool(16)
    x = cl(np.zeros((1, 12, 33, 5)), torch.float32)
    with pytest.raises(ValueError):
        layer.forward(x)
    y = torch.empty(64, device="cuda")
    with pytest.raises(HipError, match="bad arguments"):
        lib.dk_maxpool_fwd_f32(x.data_ptr(), 1, 33, 5, 12, 16, y.data_ptr(), 0, stream_handle())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_test_mode(dtype):
    case = (2, 8, 7, 9, 2)
    X, dY = inputs(case, "tied", dtype)
    layer = pool(2)
    y_train = layer.forward(cl(X, dtype))
    assert layer.max_locs is not None
    y_test = layer.forward(cl(X, dtype), test_mode=True)
    torch.cuda.synchronize()
    assert np.array_equal(bits(y_test), bits(y_train))
    assert layer.max_locs is None  # nothing recorded
    with pytest.raises(RuntimeError):
        layer.backward(cl(dY, dtype))


def test_backward_refuses_mixed_or_lattice_gradients():
    case = (2, 8, 6, 6, 2)
    X, dY = inputs(case, "tied", torch.float32)
    layer = pool(2)
    layer.forward(cl(X, torch.float32))
    with pytest.raises(ValueError):
        layer.backward(cl(dY, BF16))
    g = cl(dY, torch.float32)
    g._dk_lattice = 2
    with pytest.raises(ValueError):
        layer.backward(g)
    with pytest.raises(ValueError):
        layer.backward(cl(dY[:, :, :2], torch.float32))


# ---- BN on load ---------------------------------------------------------------------------------

class _Counter:
    """Counts the calls of some lib entry points (a wrapper set on the lib object)."""

    def __init__(self, monkeypatch, names):
        self.n = {k: 0 for k in names}
        for k in names:
            monkeypatch.setattr(lib, k, self._wrap(k, getattr(lib, k)), raising=False)

    def _wrap(self, name, fn):
        def call(*a):
            self.n[name] += 1
            return fn(*a)
        return call


POOL_FWD = ["dk_maxpool_fwd_f32", "dk_maxpool_fwd_bf16", "dk_maxpool_fwd_bnx_f32", "dk_maxpool_fwd_bnx_bf16"]


def _bn_chain(C, stride):
    from dorknet_amd.layers.activations import ReLu
    from dorknet_amd.layers.batch_norm import BatchNormLayer
    from dorknet_amd.layers.pooling import MaxPoolLayer
    r = np.random.RandomState(21)
    bn = BatchNormLayer("bn", incoming_chans=C)
    for k in ("gamma", "beta"):
        bn.learned_params[k] = r.randn(*bn.learned_params[k].shape).astype(np.float32)
    ls = [bn, ReLu("relu"), MaxPoolLayer("pool", stride=stride)]
    for l in ls:
        l.to_gpu()
    return ls


@pytest.mark.parametrize("shape,dtype", [((2, 8, 7, 9), torch.float32), ((2, 6, 7, 9), torch.float32),
                                         ((3, 68, 9, 8), torch.float32), ((2, 8, 7, 9), BF16),
                                         ((3, 68, 9, 8), BF16)],
                         ids=["f32-C8", "f32-C6-scalar", "f32-C68", "bf16-C8", "bf16-C68"])
def test_bn_relu_pool_fused_equals_unfused_bitwise(shape, dtype, monkeypatch):
    """BatchNormLayer + ReLu + MaxPoolLayer through the chain executor: with fusion the pool gets a
    BNOut and runs dk_maxpool_fwd_bnx_* (the BN output is never written); y, idx, the gradient at
    the BN input, dgamma and dbeta equal the layer-by-layer run bit for bit, in training and in
    test mode."""
    from dorknet_amd.layers._chain import chain_backward, chain_forward
    N, C, H, W = shape
    rng = np.random.RandomState(C + H)
    X = stored(rng.randn(*shape), dtype)
    dY = stored(rng.randn(N, C, H // 2, W // 2), dtype)
    bnx = "dk_maxpool_fwd_bnx_bf16" if dtype == BF16 else "dk_maxpool_fwd_bnx_f32"
    plain = "dk_maxpool_fwd_bf16" if dtype == BF16 else "dk_maxpool_fwd_f32"
    outs = []
    for fuse in ("1", "0"):
        monkeypatch.setenv("DORKNET_FUSE", fuse)
        ls = _bn_chain(C, 2)
        with monkeypatch.context() as m:
            cnt = _Counter(m, POOL_FWD)
            y, steps = chain_forward(ls, cl(X, dtype))
            idx = ls[2].max_locs
            dx = chain_backward(steps, cl(dY, dtype))
            y_test, _ = chain_forward(ls, cl(X, dtype), test_mode=True)
        torch.cuda.synchronize()
        want = {k: 0 for k in POOL_FWD}
        want[bnx if fuse == "1" else plain] = 2  # the training and the test-mode forward
        assert cnt.n == want, (fuse, cnt.n)
        assert y.dtype == dtype and dx.dtype == dtype and tuple(dx.shape) == shape
        outs.append({"y": bits(y), "idx": idx.contiguous().cpu().numpy(), "dx": bits(dx),
                     "dgamma": bits(ls[0].grads["gamma"]), "dbeta": bits(ls[0].grads["beta"]),
                     "y_test": bits(y_test)})
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k


def test_bnx_bf16_rounds_before_comparing():
    """Two window elements whose BN outputs differ in fp32 but round to the same bf16 value, the
    larger one later in scan order: the unfused path pools the rounded values, a tie that the first
    element wins, so the fused kernel must record the earlier location too."""
    N, C, H, W, s = 1, 8, 4, 4, 2
    X = np.zeros((N, C, H, W), dtype=np.float32)
    # bn(x) = 0.25 * x + 1 (mean 0, invstd 1): bn(1.0) = 1.25 and bn(1.0078125) = 1.251953125, both
    # exact in fp32; bf16 spacing at 1.25 is 2^-7, so both round to 1.25
    X[0, :, 0, 0] = 1.0            # k = 0
    X[0, :, 1, 1] = 1.0078125      # k = 3: larger in fp32, equal once rounded
    X[0, 0:4, 2, 3] = 1.0          # window (1, 1), k = 1 in channels 0-3
    X[0, 0:4, 3, 2] = 1.0078125    # ... and k = 2
    X[0, 4:8, 3, 3] = 1.5          # channels 4-7: a plain maximum at k = 3 (bn = 1.375, exact in bf16)
    x = cl(X, BF16)
    assert np.array_equal(x.float().cpu().numpy(), X)  # the inputs are exact in bf16
    one = lambda v: torch.full((C,), v, dtype=torch.float32, device="cuda")  # noqa: E731
    mean, invstd, gamma, beta = one(0.0), one(1.0), one(0.25), one(1.0)
    bn = (mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1)
    st = stream_handle()
    mk = lambda dt: torch.empty((N, C, H // s, W // s), dtype=dt, device="cuda",  # noqa: E731
                                memory_format=torch.channels_last)
    y1, i1, y0, i0 = mk(BF16), mk(torch.uint8), mk(BF16), mk(torch.uint8)
    lib.dk_maxpool_fwd_bnx_bf16(x.data_ptr(), N, H, W, C, s, *bn, y1.data_ptr(), i1.data_ptr(), st)
    xa = torch.empty_like(x)
    lib.dk_bn_apply_bf16(x.data_ptr(), x.numel(), C, *bn, xa.data_ptr(), 0, st)
    lib.dk_maxpool_fwd_bf16(xa.data_ptr(), N, H, W, C, s, y0.data_ptr(), i0.data_ptr(), st)
    torch.cuda.synchronize()
    a = xa.float().cpu().numpy()
    assert a[0, 0, 0, 0] == 1.25 and a[0, 0, 1, 1] == 1.25  # the stored BN outputs do tie
    i1 = i1.contiguous().cpu().numpy()
    assert (i1[0, :, 0, 0] == 0).all(), i1[0, :, 0, 0]
    assert (i1[0, 0:4, 1, 1] == 1).all() and (i1[0, 4:8, 1, 1] == 3).all(), i1[0, :, 1, 1]
    assert np.array_equal(i1, i0.contiguous().cpu().numpy())
    assert np.array_equal(bits(y1), bits(y0))
    Y, idx = pool_fwd(a, s)  # and the rules, over the stored BN output
    assert np.array_equal(i1, idx) and np.array_equal(bits(y1), np_bits(Y, BF16))


# ---- the network of examples/mnist_maxpool.py ---------------------------------------------------

def _batch(n, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, size=(n, 1, 28, 28)).astype(np.float32)
    onehot = np.eye(10, dtype=np.float32)[rng.integers(0, 10, n)]
    return X, onehot


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def test_network_step_fused_equals_unfused_bitwise(monkeypatch):
    """One training step (forward, backward, SGDMomentum.update_weights) of MNISTMaxPoolNet at
    batch 4: the loss, every gradient and every updated weight, fused against DORKNET_FUSE=0."""
    from dorknet_amd.optimisers.SGDMomentum import SGDMomentum
    from examples.mnist_maxpool import MNISTMaxPoolNet
    X, onehot = _batch(4, 31)
    outs = []
    for fuse in ("1", "0"):
        monkeypatch.setenv("DORKNET_FUSE", fuse)
        np.random.seed(30)
        net = MNISTMaxPoolNet("pooled")
        net.to_gpu()
        sgd = SGDMomentum(net, 0.01, 0.9)
        with monkeypatch.context() as m:
            cnt = _Counter(m, POOL_FWD)
            loss, _ = net.forward(dev(X), dev(onehot))
        want = {k: 0 for k in POOL_FWD}
        want["dk_maxpool_fwd_bnx_f32" if fuse == "1" else "dk_maxpool_fwd_f32"] = 2
        assert cnt.n == want, (fuse, cnt.n)
        net.backward()
        grads = {(l.layer_name, k): bits(l.grads[k]) for l in net.layers for k in (l.grads or {})}
        sgd.update_weights()
        torch.cuda.synchronize()
        weights = {(l.layer_name, k): bits(l.learned_params[k]) for l in net.layers for k in (l.learned_params or {})}
        idx = [l.max_locs.contiguous().cpu().numpy() for l in net.layers if type(l).__name__ == "MaxPoolLayer"]
        outs.append((bits(torch.as_tensor(loss).reshape(1)), grads, weights, idx))
    assert np.array_equal(outs[0][0], outs[1][0]), "loss"
    for which in (1, 2):
        assert outs[0][which].keys() == outs[1][which].keys() and len(outs[0][which]) >= 11
        bad = [k for k in outs[0][which] if not np.array_equal(outs[0][which][k], outs[1][which][k])]
        assert not bad, (("gradients", "weights")[which - 1], bad)
    assert all(np.array_equal(a, b) for a, b in zip(outs[0][3], outs[1][3]))


def test_network_step_matches_fp64_oracle():
    """MNISTMaxPoolNet at batch 8 against the fp64 oracle (oracle.net with OMaxPool for the pools).
    The oracle replays the GPU's ReLU decisions (tests/_ties.py) and the pools' recorded locations;
    the loss and every gradient are within the project's normwise 1e-4 (test_gpu_layers.check), and
    every pool location where the GPU's choice differs from the fp64 oracle's own arg-max is a tie:
    |v64[gpu] - v64[oracle]| <= TIE_REL * rms_c(v64)."""
    from dorknet_amd.layers.pooling import MaxPoolLayer
    from examples.mnist_maxpool import MNISTMaxPoolNet
    from oracle import net as O
    from tests._convert import layer_to_oracle
    from tests._ties import TIE_REL, replay_gpu_decisions, tie_report
    from tests.test_gpu_layers import TOL, check
    np.random.seed(40)
    net = MNISTMaxPoolNet("pooled")
    onet = O.ONetwork([OMaxPool(l.layer_name, l.stride) if isinstance(l, MaxPoolLayer) else layer_to_oracle(l)
                       for l in net.layers], layer_to_oracle(net.loss_layer))
    net.to_gpu()
    X, onehot = _batch(8, 41)
    loss, P = net.forward(dev(X), dev(onehot))
    states = replay_gpu_decisions(net, [onet])
    pools = [(l, ol) for l, ol in zip(net.layers, onet.layers) if isinstance(l, MaxPoolLayer)]
    assert len(pools) == 2
    for l, ol in pools:
        ol.replay = l.max_locs.contiguous().cpu().numpy()
    net.backward()
    torch.cuda.synchronize()
    oloss, oP = onet.forward(X.astype(np.float64), onehot.astype(np.float64))
    nrelu, worst, rows = tie_report(states, onet)
    assert worst <= TIE_REL, rows[:8]
    onet.backward()
    # pool locations: the GPU's against the fp64 oracle's own arg-max
    differ, worst_pool = 0, 0.0
    for l, ol in pools:
        v = windows(ol.X, ol.stride)
        rms = np.sqrt((ol.X ** 2).mean(axis=(0, 2, 3)))[None, :, None, None]
        at = lambda i: np.take_along_axis(v, i[..., None].astype(np.int64), axis=-1)[..., 0]  # noqa: E731
        gap = np.abs(at(ol.idx) - at(ol.own_idx)) / np.maximum(rms, 1e-300)
        bad = ol.idx != ol.own_idx
        differ += int(bad.sum())
        if bad.any():
            worst_pool = max(worst_pool, float(gap[bad].max()))
    print("{} ReLU decision(s) and {} pool location(s) differ from the fp64 oracle's own; worst pool gap "
          "{:.2e} of the channel rms".format(nrelu, differ, worst_pool))
    assert worst_pool <= TIE_REL, "{} pool location(s) differ from the fp64 arg-max, worst gap {:.3e} of rms".format(
        differ, worst_pool)
    assert abs(float(loss) - oloss) <= TOL * abs(oloss), (float(loss), oloss)
    check("P", P, oP)
    n = 0
    for l, ol in zip(net.layers, onet.layers):
        for k in (ol.grads or {}):
            check("{}.{}".format(l.layer_name, k), l.grads[k], ol.grads[k])
            n += 1
    assert n >= 11
