"""ReshapeLayer on the GPU (dk_flatten_*, dorknet_amd/csrc/reshape.hip).

Copies and widenings are exact, so every comparison here is bitwise -- fp32 as its int32 bits, bf16 as
its int16 bits -- against the numpy restatement of the rules (tests/_reshape_twin.py), and fused (BN on
load) against DORKNET_FUSE=0.  Only the DenseLayer cases and the whole-network comparison with the fp64
oracle have a tolerance (the project's normwise 1e-4, or FP32_SLACK times the fp32 restatement's own
error), the latter with the ReLU decisions and the pool's locations replayed and every disagreement
with the fp64 oracle asserted to be a tie.
"""
import numpy as np
import pytest
import torch

from dorknet_amd._hip import HipError, lib, stream_handle
from tests._reshape_twin import OReshape, flatten, unflatten

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
DTYPES = [torch.float32, BF16]
# (N, C, H, W); the tile is 64 pixels x 64 channels
CASES = [
    (2, 3, 5, 5),       # scalar channels, odd HW
    (2, 4, 7, 7),       # vector channels, HW = 49: no flat row is 16-byte aligned
    (1, 68, 14, 14),    # more than one tile each way, C not a multiple of 64
    (2, 130, 3, 3),     # many channel tiles, one short pixel tile
    (1, 16, 33, 17),    # many pixel tiles with a remainder
    (2, 8, 1, 1),       # HW = 1
    (3, 512, 7, 7),     # the workload's own last shape at a small batch
    (1, 64, 8, 8),      # exactly one tile each way
    (1, 63, 9, 7),      # one below the tile edge each way (scalar channels)
    (1, 65, 5, 13),     # one above the tile edge each way (scalar channels)
    (1, 60, 5, 13),     # vector channels: a short channel tile, one pixel past the pixel tile
]
HALF_DOWN, HALF_UP = 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8  # halfway between bf16 values: to 1.0 and to 1 + 2^-6


def bits(t):
    """The stored bits of a tensor in its logical order, as a numpy integer array."""
    t = t.detach().contiguous()
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32).cpu().numpy()


def np_bits(a, dtype=torch.float32):
    """The bits a float32 numpy array has when stored as `dtype` (round-to-nearest-even for bf16)."""
    return bits(torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dtype))


def stored(a, dtype):
    """`a` rounded to what `dtype` storage holds, as float32 numpy."""
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dtype).float().numpy()


def cl(a, dtype=torch.float32):
    """numpy NCHW -> a channels-last device tensor of `dtype`."""
    t = torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda").to(dtype)
    return t.contiguous(memory_format=torch.channels_last)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def inputs(case, dtype):
    N, C, H, W = case
    rng = np.random.RandomState(sum(case))
    X = stored(rng.randn(N, C, H, W), dtype)
    dY = rng.randn(N, C * H * W).astype(np.float32)
    dY[0, 0], dY[0, 1] = HALF_DOWN, HALF_UP
    return X, dY


def flat_layer(case, name="flat"):
    from dorknet_amd.layers.reshape import ReshapeLayer
    N, C, H, W = case
    l = ReshapeLayer(name, (-1, C, H, W), (-1, C * H * W))
    l.to_gpu()
    return l


def identity_bn(C):
    """bn(x) = 1 * ((x - 0) * 1) + 0 = x, no ReLU: (tensors to keep alive, the entry points' arguments)."""
    t = [torch.zeros(C, device="cuda"), torch.ones(C, device="cuda"), torch.ones(C, device="cuda"),
         torch.zeros(C, device="cuda")]
    return t, tuple(v.data_ptr() for v in t) + (0,)


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_layer_matches_twin_bitwise(case, dtype, layout):
    N, C, H, W = case
    X, dY = inputs(case, dtype)
    Y, dX = flatten(X), unflatten(dY, case)
    layer = flat_layer(case)
    # one run hands the layer a plain NCHW tensor (its own layout conversion), the other a channels-last one
    x = cl(X, dtype) if layout == "nhwc" else dev(X).to(dtype)
    y = layer.forward(x)
    assert y.dtype == torch.float32 and tuple(y.shape) == Y.shape and y.is_contiguous()
    dx = layer.backward(dev(dY))
    assert dx.dtype == dtype and tuple(dx.shape) == X.shape and dx.is_contiguous(memory_format=torch.channels_last)
    torch.cuda.synchronize()
    assert np.array_equal(bits(y), np_bits(Y))  # bf16 widened: X holds the widened values
    assert np.array_equal(bits(dx), np_bits(dX, dtype))  # fp32: the copy; bf16: torch's round-to-nearest-even
    if dtype == BF16:  # ties to even, spelled out
        got = flatten(dx.float().cpu().numpy())
        assert got[0, 0] == 1.0 and got[0, 1] == 1 + 2.0 ** -6, (got[0, 0], got[0, 1])
    # every raw entry once more into an output pre-filled with NaN: an element the kernel leaves unwritten
    # would still be NaN
    sfx = "bf16" if dtype == BF16 else "f32"
    st = stream_handle()
    xc, dyc = cl(X, dtype), dev(dY)
    keep, bn = identity_bn(C)
    for name, args in (("dk_flatten_fwd_" + sfx, ()), ("dk_flatten_fwd_bnx_" + sfx, bn)):
        yn = torch.full((N, C * H * W), float("nan"), device="cuda")
        getattr(lib, name)(xc.data_ptr(), N, H * W, C, *args, yn.data_ptr(), st)
        torch.cuda.synchronize()
        assert not bool(torch.isnan(yn).any()), name
        assert np.array_equal(bits(yn), np_bits(Y)), name
    dxn = cl(np.full(X.shape, np.nan), dtype)
    getattr(lib, "dk_flatten_bwd_" + sfx)(dyc.data_ptr(), N, H * W, C, dxn.data_ptr(), st)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(dxn).any())
    assert np.array_equal(bits(dxn), np_bits(dX, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_misaligned_pointers_take_the_scalar_path(dtype):
    """C % 4 == 0 but x, y and dx one element off a vector boundary."""
    case = N, C, H, W = 2, 8, 5, 5
    X, dY = inputs(case, dtype)
    Y, dX = flatten(X), unflatten(dY, case)
    nhwc = lambda a: np.ascontiguousarray(a.transpose(0, 2, 3, 1))  # noqa: E731

    def off(n, dt, fill=None):
        buf = torch.empty(n + 1, dtype=dt, device="cuda")
        if fill is not None:
            buf[1:] = torch.as_tensor(np.ascontiguousarray(fill, dtype=np.float32).ravel(), device="cuda").to(dt)
        return buf, buf[1:]

    nan = np.full(X.size, np.nan, dtype=np.float32)
    _, x = off(X.size, dtype, nhwc(X))
    _, dy = off(dY.size, torch.float32, dY)
    _, y = off(Y.size, torch.float32, nan)
    _, dx = off(X.size, dtype, nan)
    assert x.data_ptr() % (4 * x.element_size()) and dx.data_ptr() % (4 * dx.element_size()) and y.data_ptr() % 16
    sfx = "bf16" if dtype == BF16 else "f32"
    st = stream_handle()
    getattr(lib, "dk_flatten_fwd_" + sfx)(x.data_ptr(), N, H * W, C, y.data_ptr(), st)
    getattr(lib, "dk_flatten_bwd_" + sfx)(dy.data_ptr(), N, H * W, C, dx.data_ptr(), st)
    torch.cuda.synchronize()
    assert np.array_equal(bits(y).reshape(N, C * H * W), np_bits(Y))
    assert np.array_equal(bits(dx).reshape(N, H, W, C), np_bits(nhwc(dX), dtype))


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


FLAT_FWD = ["dk_flatten_fwd_f32", "dk_flatten_fwd_bf16", "dk_flatten_fwd_bnx_f32", "dk_flatten_fwd_bnx_bf16"]
BN_APPLY = ["dk_bn_apply_f32", "dk_bn_apply_bf16"]


def _bn_chain(shape, relu):
    from dorknet_amd.layers.activations import ReLu
    from dorknet_amd.layers.batch_norm import BatchNormLayer
    from dorknet_amd.layers.reshape import ReshapeLayer
    N, C, H, W = shape
    r = np.random.RandomState(21)
    bn = BatchNormLayer("bn", incoming_chans=C)
    for k in ("gamma", "beta"):
        bn.learned_params[k] = r.randn(*bn.learned_params[k].shape).astype(np.float32)
    ls = [bn] + ([ReLu("relu")] if relu else []) + [ReshapeLayer("flat", (-1, C, H, W), (-1, C * H * W))]
    for l in ls:
        l.to_gpu()
    return ls


def _bnx_bf16_scalar_equals_padded_unfused(X, relu):
    N, C, H, W = X.shape
    Cp = -(-C // 4) * 4
    r = np.random.RandomState(22)
    mean, invstd, gamma, beta = (dev(v) for v in (r.randn(Cp), r.rand(Cp) + 0.5, r.randn(Cp), r.randn(Cp)))
    bn = (mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), int(relu))
    Xp = np.zeros((N, Cp, H, W), dtype=np.float32)
    Xp[:, :C] = X
    x, xp = cl(X, BF16), cl(Xp, BF16)
    st = stream_handle()
    y1 = torch.full((N, C * H * W), float("nan"), device="cuda")
    lib.dk_flatten_fwd_bnx_bf16(x.data_ptr(), N, H * W, C, *bn, y1.data_ptr(), st)
    xa = torch.empty_like(xp)
    lib.dk_bn_apply_bf16(xp.data_ptr(), xp.numel(), Cp, *bn, xa.data_ptr(), 0, st)
    torch.cuda.synchronize()
    want = flatten(xa.float().cpu().numpy()[:, :C])
    assert not bool(torch.isnan(y1).any())
    assert np.array_equal(bits(y1), np_bits(want))
    if relu:
        assert (want == 0).any() and (want > 0).any()


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "norelu"])
@pytest.mark.parametrize("C", [8, 6], ids=["C8", "C6-scalar"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_bn_relu_flatten_fused_equals_unfused_bitwise(dtype, C, relu, monkeypatch):
    """BatchNormLayer [+ ReLu] + ReshapeLayer through the chain executor: with fusion the flatten gets a
    BNOut and runs dk_flatten_fwd_bnx_* (the BN output is never written: no dk_bn_apply_* launch); y, the
    gradient at the BN input, dgamma and dbeta equal the layer-by-layer run bit for bit, in training
    and in test mode."""
    from dorknet_amd.layers._chain import chain_backward, chain_forward
    shape = N, _, H, W = 3, C, 7, 5
    rng = np.random.RandomState(C + H)
    X = stored(rng.randn(*shape), dtype)
    dY = rng.randn(N, C * H * W).astype(np.float32)
    sfx = "bf16" if dtype == BF16 else "f32"
    if dtype == BF16 and C % 4:
        # BatchNormLayer (and ReLu's backward) have no bf16 path at C % 4 != 0 -- dk_bn_stats_bf16 and
        # dk_bn_apply_bf16 refuse it -- so neither chain exists at this size.  What does exist is compared
        # instead: the fused entry's scalar path on the C = 6 tensor against the unfused sequence (apply,
        # then flatten the stored bf16 output) run on the same values padded to 8 channels.
        _bnx_bf16_scalar_equals_padded_unfused(X, relu)
        return
    outs = []
    for fuse in ("1", "0"):
        monkeypatch.setenv("DORKNET_FUSE", fuse)
        ls = _bn_chain(shape, relu)
        with monkeypatch.context() as m:
            cnt = _Counter(m, FLAT_FWD + BN_APPLY)
            y, steps = chain_forward(ls, cl(X, dtype))
            dx = chain_backward(steps, dev(dY))
            y_test, _ = chain_forward(ls, cl(X, dtype), test_mode=True)
        torch.cuda.synchronize()
        want = {k: 0 for k in FLAT_FWD}
        want[("dk_flatten_fwd_bnx_" if fuse == "1" else "dk_flatten_fwd_") + sfx] = 2  # training and test mode
        assert {k: cnt.n[k] for k in FLAT_FWD} == want, (fuse, cnt.n)
        if fuse == "1":
            assert all(cnt.n[k] == 0 for k in BN_APPLY), cnt.n
        assert y.dtype == torch.float32 and dx.dtype == dtype and tuple(dx.shape) == shape
        outs.append({"y": bits(y), "dx": bits(dx), "dgamma": bits(ls[0].grads["gamma"]),
                     "dbeta": bits(ls[0].grads["beta"]), "y_test": bits(y_test)})
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k
    if relu:
        assert (outs[0]["y"] == 0).any() and (outs[0]["y"] > 0).any()  # the ReLU really cut something


def test_bnx_bf16_rounds_before_it_widens():
    """bn(x) = 0.25 * x + 1 at x = 1.0078125 is 1.251953125, exact in fp32 and no bf16 value (the spacing at
    1.25 is 2^-7): the unfused path flattens the stored bf16 BN output 1.25, so the fused entry must
    give 1.25 too, not the fp32 value."""
    N, C, H, W = 1, 8, 3, 3
    X = np.zeros((N, C, H, W), dtype=np.float32)
    X[0, :, 1, 2] = 1.0078125
    x = cl(X, BF16)
    assert np.array_equal(x.float().cpu().numpy(), X)  # the input is exact in bf16
    one = lambda v: torch.full((C,), v, dtype=torch.float32, device="cuda")  # noqa: E731
    mean, invstd, gamma, beta = one(0.0), one(1.0), one(0.25), one(1.0)
    bn = (mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1)
    st = stream_handle()
    y1 = torch.empty((N, C * H * W), device="cuda")
    y0 = torch.empty_like(y1)
    yf = torch.empty_like(y1)
    lib.dk_flatten_fwd_bnx_bf16(x.data_ptr(), N, H * W, C, *bn, y1.data_ptr(), st)
    xa = torch.empty_like(x)
    lib.dk_bn_apply_bf16(x.data_ptr(), x.numel(), C, *bn, xa.data_ptr(), 0, st)
    lib.dk_flatten_fwd_bf16(xa.data_ptr(), N, H * W, C, y0.data_ptr(), st)
    xf = cl(X)
    lib.dk_flatten_fwd_bnx_f32(xf.data_ptr(), N, H * W, C, *bn, yf.data_ptr(), st)
    torch.cuda.synchronize()
    f = 0 * H * W + 1 * W + 2
    assert float(yf[0, f]) == 1.251953125      # the fp32 entry keeps the fp32 value
    assert float(xa[0, 0, 1, 2]) == 1.25       # the stored bf16 BN output
    assert float(y1[0, f]) == 1.25, float(y1[0, f])
    assert np.array_equal(bits(y1), bits(y0))
    assert np.array_equal(bits(y1), np_bits(flatten(xa.float().cpu().numpy())))


# ---- unflatten, 4-D -> 4-D, the identity -----------------------------------------------------------

@pytest.mark.parametrize("case", [(2, 3, 5, 5), (2, 68, 9, 8), (2, 8, 1, 1)], ids=lambda c: "x".join(map(str, c)))
def test_unflatten_matches_twin_bitwise(case):
    from dorknet_amd.layers.reshape import ReshapeLayer
    N, C, H, W = case
    rng = np.random.RandomState(sum(case))
    Y = rng.randn(N, C * H * W).astype(np.float32)
    dX = rng.randn(N, C, H, W).astype(np.float32)
    layer = ReshapeLayer("unflat", (-1, C * H * W), (-1, C, H, W))
    layer.to_gpu()
    x = layer.forward(dev(Y))
    assert x.dtype == torch.float32 and tuple(x.shape) == case and x.is_contiguous(memory_format=torch.channels_last)
    dy = layer.backward(dev(dX))  # a plain NCHW gradient: the layer's own layout conversion
    assert tuple(dy.shape) == Y.shape and dy.is_contiguous()
    torch.cuda.synchronize()
    assert np.array_equal(bits(x), np_bits(unflatten(Y, case)))
    assert np.array_equal(bits(dy), np_bits(flatten(dX)))
    assert np.array_equal(bits(layer.backward(cl(dX))), np_bits(flatten(dX)))


def test_remap_and_identity_match_twin_bitwise(monkeypatch):
    from dorknet_amd.layers.reshape import ReshapeLayer
    rng = np.random.RandomState(3)
    X = rng.randn(2, 8, 6, 6).astype(np.float32)
    dY = rng.randn(2, 18, 4, 4).astype(np.float32)
    layer = ReshapeLayer("remap", (-1, 8, 6, 6), (-1, 18, 4, 4))
    layer.to_gpu()
    y = layer.forward(cl(X))
    dx = layer.backward(cl(dY))
    torch.cuda.synchronize()
    assert tuple(y.shape) == dY.shape and y.is_contiguous(memory_format=torch.channels_last)
    assert tuple(dx.shape) == X.shape and dx.is_contiguous(memory_format=torch.channels_last)
    assert np.array_equal(bits(y), np_bits(X.reshape(2, 18, 4, 4)))
    assert np.array_equal(bits(dx), np_bits(dY.reshape(2, 8, 6, 6)))
    ident = ReshapeLayer("same", (-1, 8, 6, 6), (2, 8, 6, 6))
    ident.to_gpu()
    cnt = _Counter(monkeypatch, FLAT_FWD + ["dk_flatten_bwd_f32", "dk_flatten_bwd_bf16"])
    x = cl(X)
    g = cl(X)
    assert ident.forward(x) is x and ident.backward(g) is g  # no launch
    assert not any(cnt.n.values()), cnt.n
    with pytest.raises(NotImplementedError, match="same"):
        ident.forward(cl(X, BF16))  # bf16 is taken by the flatten only


# ---- refusals -------------------------------------------------------------------------------------

def test_refusals():
    from dorknet_amd.layers.reshape import ReshapeLayer
    case = (2, 8, 3, 3)
    X, dY = inputs(case, torch.float32)
    layer = flat_layer(case)
    with pytest.raises(RuntimeError):
        layer.backward(dev(dY))  # backward before forward
    with pytest.raises(ValueError):
        layer.forward(cl(X[:, :6]))  # a feature count that does not match
    with pytest.raises(ValueError):
        layer.forward(dev(dY))  # a 2-D input into the flatten
    fixed = ReshapeLayer("fixed", (4, 8, 3, 3), (4, 72))
    fixed.to_gpu()
    with pytest.raises(ValueError):
        fixed.forward(cl(X))  # a batch of 2 where the shapes name 4
    layer.forward(cl(X), test_mode=True)
    with pytest.raises(RuntimeError):
        layer.backward(dev(dY))  # a test-mode forward records nothing
    layer.forward(cl(X, BF16))
    with pytest.raises(ValueError):
        layer.backward(dev(dY).to(BF16))  # a gradient of the other storage type: the output is fp32
    with pytest.raises(ValueError):
        layer.backward(dev(dY[:, :70]))  # a gradient of the wrong shape
    assert layer.backward(dev(dY)).dtype == BF16
    unflat = ReshapeLayer("unflat", (-1, 72), (-1, 8, 3, 3))
    unflat.to_gpu()
    with pytest.raises(NotImplementedError, match="unflat"):
        unflat.forward(dev(dY).to(BF16))  # bf16 into an unflatten
    unflat.forward(dev(dY))
    with pytest.raises(ValueError):
        unflat.backward(cl(X, BF16))
    with pytest.raises(ValueError):
        unflat.backward(cl(X[:, :4]))
    remap = ReshapeLayer("remap", (-1, 8, 3, 3), (-1, 2, 6, 6))
    remap.to_gpu()
    with pytest.raises(NotImplementedError, match="remap"):
        remap.forward(cl(X, BF16))
    odd = ReshapeLayer("odd", (-1, 8, 9), (-1, 72))
    odd.to_gpu()
    with pytest.raises(NotImplementedError, match="odd"):
        odd.forward(dev(dY).reshape(2, 8, 9))  # 3-D -> 2-D: no such form
    # the raw entries with N = 0
    x, y = cl(X), torch.empty((2, 72), device="cuda")
    keep, bn = identity_bn(8)
    st = stream_handle()
    for sfx in ("f32", "bf16"):
        with pytest.raises(HipError, match="bad arguments"):
            getattr(lib, "dk_flatten_fwd_" + sfx)(x.data_ptr(), 0, 9, 8, y.data_ptr(), st)
        with pytest.raises(HipError, match="bad arguments"):
            getattr(lib, "dk_flatten_fwd_bnx_" + sfx)(x.data_ptr(), 0, 9, 8, *bn, y.data_ptr(), st)
        with pytest.raises(HipError, match="bad arguments"):
            getattr(lib, "dk_flatten_bwd_" + sfx)(y.data_ptr(), 0, 9, 8, x.data_ptr(), st)


# ---- DenseLayer at flatten widths -------------------------------------------------------------------

@pytest.mark.parametrize("case", [(3, 75, 10, True, 0.0), (4, 3136, 32, True, 1e-4), (2, 25088, 10, False, 0.0)],
                         ids=lambda c: "x".join(map(str, c[:3])))
def test_dense_layer_at_flatten_widths(case):
    """DenseLayer with IN = C * H * W of a flattened map (IN % 4 != 0; 64 * 49; 512 * 49) against the
    fp64 oracle under tests/test_gpu_layers.check's rule: normwise 1e-4, or FP32_SLACK times the fp32
    restatement's own error."""
    from dorknet_amd.layers.dense_layer import DenseLayer
    from dorknet_amd.regularisers.l2 import l2
    from tests.test_gpu_layers import run_layer
    B, IN, OUT, bias, s = case
    rng = np.random.RandomState(7)
    np.random.seed(8)
    layer = DenseLayer("d", IN, OUT, with_bias=bias, weight_regulariser=l2(s) if s else None)
    if bias:
        layer.learned_params["bias"] = rng.randn(OUT).astype(np.float32)
    run_layer(layer, rng.randn(B, IN).astype(np.float32), rng.randn(B, OUT).astype(np.float32))


# ---- a small LeNet ----------------------------------------------------------------------------------

SMALL_CONVS = [((8, 1, 3, 3), True), ((16, 8, 3, 3), False)]


def small_lenet(name="lenet"):
    """Input 1x12x12: conv 1->8 + BN + ReLU + pool 2, conv 8->16 + BN + ReLU, reshape to 16 * 36,
    dense -> 32, ReLu, dense -> 10, softmax."""
    from examples.mnist_lenet import MNISTLeNet
    return MNISTLeNet(name, convs=SMALL_CONVS, side=12, hidden=32)


def _batch(n, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, size=(n, 1, 12, 12)).astype(np.float32)
    onehot = np.eye(10, dtype=np.float32)[rng.integers(0, 10, n)]
    return X, onehot


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_network_step_fused_equals_unfused_bitwise(dtype, monkeypatch):
    """One training step (forward, backward, SGDMomentum.update_weights) of the small LeNet at batch 4,
    from an fp32 and from a bf16 input: the loss, every gradient and every updated weight, fused
    against DORKNET_FUSE=0."""
    from dorknet_amd.optimisers.SGDMomentum import SGDMomentum
    X, onehot = _batch(4, 31)
    sfx = "bf16" if dtype == BF16 else "f32"
    outs = []
    for fuse in ("1", "0"):
        monkeypatch.setenv("DORKNET_FUSE", fuse)
        np.random.seed(30)
        net = small_lenet()
        net.to_gpu()
        sgd = SGDMomentum(net, 0.01, 0.9)
        with monkeypatch.context() as m:
            cnt = _Counter(m, FLAT_FWD)
            loss, _ = net.forward(dev(X).to(dtype), dev(onehot))
        want = {k: 0 for k in FLAT_FWD}
        want[("dk_flatten_fwd_bnx_" if fuse == "1" else "dk_flatten_fwd_") + sfx] = 1
        assert cnt.n == want, (fuse, cnt.n)
        net.backward()
        grads = {(l.layer_name, k): bits(l.grads[k]) for l in net.layers for k in (l.grads or {})}
        sgd.update_weights()
        torch.cuda.synchronize()
        weights = {(l.layer_name, k): bits(l.learned_params[k]) for l in net.layers for k in (l.learned_params or {})}
        outs.append((bits(torch.as_tensor(loss).reshape(1)), grads, weights))
    assert np.array_equal(outs[0][0], outs[1][0]), "loss"
    for which in (1, 2):
        assert outs[0][which].keys() == outs[1][which].keys() and len(outs[0][which]) == 10
        bad = [k for k in outs[0][which] if not np.array_equal(outs[0][which][k], outs[1][which][k])]
        assert not bad, (("gradients", "weights")[which - 1], bad)


def test_network_step_matches_fp64_oracle():
    """The small LeNet at batch 8 against the fp64 oracle (oracle.net with OMaxPool for the pool and
    OReshape for the flatten).  The oracle replays the GPU's ReLU decisions (tests/_ties.py) and the
    pool's recorded locations; the loss and every gradient are within the project's normwise 1e-4
    (test_gpu_layers.check), and every pool location where the GPU's choice differs from the fp64
    oracle's own arg-max is a tie: |v64[gpu] - v64[oracle]| <= TIE_REL * rms_c(v64)."""
    from dorknet_amd.layers.pooling import MaxPoolLayer
    from dorknet_amd.layers.reshape import ReshapeLayer
    from oracle import net as O
    from tests._convert import layer_to_oracle
    from tests._maxpool_twin import OMaxPool, windows
    from tests._ties import TIE_REL, replay_gpu_decisions, tie_report
    from tests.test_gpu_layers import TOL, check

    def to_oracle(l):
        if isinstance(l, MaxPoolLayer):
            return OMaxPool(l.layer_name, l.stride)
        if isinstance(l, ReshapeLayer):
            return OReshape(l.layer_name, l.input_shape, l.output_shape)
        return layer_to_oracle(l)

    np.random.seed(40)
    net = small_lenet()
    onet = O.ONetwork([to_oracle(l) for l in net.layers], layer_to_oracle(net.loss_layer))
    net.to_gpu()
    X, onehot = _batch(8, 41)
    loss, P = net.forward(dev(X), dev(onehot))
    states = replay_gpu_decisions(net, [onet])
    assert len(states) == 3
    pools = [(l, ol) for l, ol in zip(net.layers, onet.layers) if isinstance(l, MaxPoolLayer)]
    assert len(pools) == 1
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
    assert n == 10


def _have_h5():
    from dorknet_amd.network import checkpoint
    try:
        backend = checkpoint._backend()
        if backend.__name__.endswith("_h5lite"):
            backend._load()
        return True
    except ImportError:
        return False


@pytest.mark.skipif(not _have_h5(), reason="neither h5py nor the HDF5 C library is available")
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_checkpoint_round_trip_gives_the_same_bits(dtype, tmp_path):
    """The small LeNet after one training step, saved and loaded with load_network_from_json_and_h5 into a
    fresh object: a test-mode forward gives the same bits."""
    from dorknet_amd.layers.reshape import ReshapeLayer
    from dorknet_amd.network.feed_forward_network import FeedForwardNetwork
    from dorknet_amd.optimisers.SGDMomentum import SGDMomentum
    np.random.seed(50)
    net = small_lenet()
    net.to_gpu()
    X, onehot = _batch(4, 51)
    sgd = SGDMomentum(net, 0.01, 0.9)
    net.forward(dev(X), dev(onehot))
    net.backward()
    sgd.update_weights()
    _, scores = net.forward(dev(X).to(dtype), None, test_mode=True)
    h5f, js = str(tmp_path / "w.h5"), str(tmp_path / "s.json")
    net.save_weights_to_h5(h5f)
    net.save_layer_structure_to_json(js)
    fresh = FeedForwardNetwork("x")
    fresh.load_network_from_json_and_h5(js, h5f)
    fresh.to_gpu()
    flat = [l for l in fresh.layers if isinstance(l, ReshapeLayer)]
    assert len(flat) == 1 and flat[0].input_shape == (-1, 16, 6, 6) and flat[0].output_shape == (-1, 576)
    _, again = fresh.forward(dev(X).to(dtype), None, test_mode=True)
    torch.cuda.synchronize()
    assert np.array_equal(bits(again), bits(scores))
