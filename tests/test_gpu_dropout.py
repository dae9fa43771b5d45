"""DropoutLayer on the GPU (dk_dropout_*, dorknet_amd/csrc/dropout.hip).

The mask is a pure function of (seed, step, lane, element index) and the arithmetic is one fp32 multiply
(for bf16 storage rounded once), so every comparison here is bitwise -- fp32 as its int32 bits, bf16 as
its int16 bits -- against the numpy restatement of the rule (tests/_dropout_twin.py), the BN-on-load
entries against dk_bn_apply_* followed by the plain entry, and fused against DORKNET_FUSE=0.  Every
output buffer handed to an entry point is pre-filled with NaN: an element the kernel leaves unwritten
would still be NaN.  Only the whole-network comparison with the fp64 oracle has a tolerance (the
project's normwise 1e-4, tests/_convert.slack_bound).
"""
import numpy as np
import pytest
import torch

from dorknet_amd._hip import lib, stream_handle
from tests._dropout_twin import ODropout, dropout_bwd, dropout_fwd, keep_mask, threshold

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
F32 = torch.float32
STORAGE = {F32: "f32", BF16: "bf16"}
PLAIN = {F32: ("dk_dropout_fwd_f32", "dk_dropout_bwd_f32"), BF16: ("dk_dropout_fwd_bf16", "dk_dropout_bwd_bf16")}
BNX = {F32: "dk_dropout_fwd_bnx_f32", BF16: "dk_dropout_fwd_bnx_bf16"}
APPLY = {F32: "dk_bn_apply_f32", BF16: "dk_bn_apply_bf16"}
ENTRIES = ["dk_dropout_fwd_f32", "dk_dropout_fwd_bf16", "dk_dropout_fwd_bnx_f32", "dk_dropout_fwd_bnx_bf16"]


def bits(t):
    """The stored bits of a tensor in its logical order, as a numpy integer array."""
    t = t.detach().contiguous()
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32).cpu().numpy()


def np_bits(a, dtype):
    """The bits a float32 numpy array has when stored as `dtype` (exact for the values used here)."""
    return bits(torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dtype))


def stored(a, dtype):
    """`a` rounded to what `dtype` storage holds, as float32 numpy."""
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dtype).float().numpy()


def storage_order(a):
    """A logically NCHW (or 2-D) numpy array as the flat array its NHWC (row-major) bytes hold."""
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1) if a.ndim == 4 else a).ravel()


def logical(flat, shape):
    """The inverse of storage_order."""
    if len(shape) == 4:
        N, C, H, W = shape
        return np.ascontiguousarray(flat.reshape(N, H, W, C).transpose(0, 3, 1, 2))
    return flat.reshape(shape)


def dev(a, dtype):
    """numpy (logical shape) -> a device tensor of `dtype`, channels-last when 4-D."""
    t = torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda").to(dtype)
    return t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t.contiguous()


def nan_like(t):
    return torch.full_like(t, float("nan"))


def dropout(p, seed):
    from dorknet_amd.layers.dropout import DropoutLayer
    l = DropoutLayer("drop", p, seed=seed)
    l.to_gpu()
    return l


def inputs(shape, dtype, p, seed, step):
    """Random X and dY of `shape` as `dtype` stores them.  X also holds an infinity at a kept and at a
    dropped element and NaNs at dropped elements only (a dropped element is +0.0 whatever x was; a kept
    NaN's payload is not part of the rule)."""
    rng = np.random.RandomState(sum(shape) + int(p * 10))
    X = stored(rng.randn(*shape), dtype)
    dY = stored(rng.randn(*shape), dtype)
    keep = keep_mask(X.size, p, seed, step, 0)
    flat = storage_order(X)
    kept, dropped = np.flatnonzero(keep), np.flatnonzero(~keep)
    flat[kept[len(kept) // 2]] = np.inf
    if len(dropped):
        flat[dropped[0]] = -np.inf
        flat[dropped[1::5]] = np.nan
    return logical(flat, shape), dY


# (shape, storage type, drop probabilities)
CASES = [
    ((3, 37), F32, [0.5]),                 # n = 111: a tail of 7
    ((5, 4099), F32, [0.0, 0.5, 0.9]),     # odd, and more than one block of 256 threads x 8 elements
    ((2, 6, 5, 5), F32, [0.5]),            # C not a multiple of 4
    ((2, 8, 7, 7), BF16, [0.0, 0.5, 0.9]),
    ((3, 4, 5, 5), BF16, [0.5]),           # n = 300: a tail of 4
]
CASE_PARAMS = [pytest.param(s, d, p, id="{}-{}-p{}".format("x".join(map(str, s)), STORAGE[d], p))
               for s, d, ps in CASES for p in ps]


@pytest.mark.parametrize("shape,dtype,p", CASE_PARAMS)
def test_layer_and_entries_match_twin_bitwise(shape, dtype, p):
    seed, T = 1234567 + len(shape), threshold(p)
    layer = dropout(p, seed)
    layer.step = 3
    X, dY = inputs(shape, dtype, p, seed, 3)
    Y = logical(dropout_fwd(storage_order(X), p, seed, 3, storage=STORAGE[dtype]), shape)
    dX = logical(dropout_bwd(storage_order(dY), p, seed, 3, storage=STORAGE[dtype]), shape)
    # the layer, handed plain (NCHW-contiguous) tensors: its own layout conversion
    x = torch.as_tensor(X, device="cuda").to(dtype)
    y = layer.forward(x)
    assert layer.step == 4
    dx = layer.backward(torch.as_tensor(dY, device="cuda").to(dtype))
    dx2 = layer.backward(dev(dY, dtype))  # the recorded step, a second time
    torch.cuda.synchronize()
    for got in (y, dx, dx2):
        assert got.dtype == dtype and tuple(got.shape) == shape
        assert len(shape) == 2 or got.is_contiguous(memory_format=torch.channels_last)
    assert np.array_equal(bits(y), np_bits(Y, dtype))
    assert np.array_equal(bits(dx), np_bits(dX, dtype)) and np.array_equal(bits(dx2), np_bits(dX, dtype))
    if p == 0.0:
        assert np.array_equal(bits(y), np_bits(X, dtype))  # the input bits
    # the raw entry points into NaN-filled outputs: every element is written
    xd, dyd = dev(X, dtype), dev(dY, dtype)
    yn, dxn = nan_like(xd), nan_like(xd)
    fwd, bwd = PLAIN[dtype]
    getattr(lib, fwd)(xd.data_ptr(), xd.numel(), T, seed, 3, 0, 0, yn.data_ptr(), stream_handle())
    getattr(lib, bwd)(dyd.data_ptr(), xd.numel(), T, seed, 3, 0, 0, dxn.data_ptr(), stream_handle())
    torch.cuda.synchronize()
    assert np.array_equal(bits(yn), np_bits(Y, dtype)) and np.array_equal(bits(dxn), np_bits(dX, dtype))
    assert not bool(torch.isnan(dxn).any())


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_misaligned_pointers_take_the_scalar_path(dtype):
    """x and y one element off a 16-byte boundary: every element goes the element-by-element way."""
    n, p, seed = 1003, 0.5, 99
    a = stored(np.random.RandomState(4).randn(n), dtype)
    want = dropout_fwd(a, p, seed, 7, lane=2, storage=STORAGE[dtype])
    xbuf = torch.zeros(n + 1, dtype=dtype, device="cuda")
    xbuf[1:] = torch.as_tensor(a, device="cuda").to(dtype)
    ybuf = torch.full((n + 2,), float("nan"), dtype=dtype, device="cuda")
    x, y = xbuf[1:], ybuf[1:n + 1]
    assert x.data_ptr() % 16 != 0 and y.data_ptr() % 16 != 0
    getattr(lib, PLAIN[dtype][0])(x.data_ptr(), n, threshold(p), seed, 7, 2, 0, y.data_ptr(), stream_handle())
    torch.cuda.synchronize()
    assert np.array_equal(bits(y), np_bits(want, dtype))
    assert bool(torch.isnan(ybuf[0])) and bool(torch.isnan(ybuf[n + 1]))  # nothing written beside the buffer


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_first_index_crosses_the_32_bit_block_boundary(dtype):
    """first_index = 2^35 - 32, n = 64: blocks 2^32 - 4 .. 2^32 + 3, the upper counter word is used."""
    n, p, seed, first = 64, 0.5, 1, 2 ** 35 - 32
    keep = keep_mask(n, p, seed, 0, 0, first_index=first)
    assert int(keep.sum()) == 37
    a = stored(np.random.RandomState(5).randn(n), dtype)
    x = dev(a, dtype)
    for which in (0, 1):  # forward and backward entry
        want = (dropout_fwd, dropout_bwd)[which](a, p, seed, 0, first_index=first, storage=STORAGE[dtype])
        y = nan_like(x)
        getattr(lib, PLAIN[dtype][which])(x.data_ptr(), n, threshold(p), seed, 0, 0, first, y.data_ptr(),
                                          stream_handle())
        torch.cuda.synchronize()
        assert np.array_equal(bits(y), np_bits(want, dtype))
        assert np.array_equal(bits(y) != 0, keep)  # (no input element is zero)


# ---- BN on load ---------------------------------------------------------------------------------

# the issue's shapes, then C = 12 (a thread's second group of four channels wraps to channel 0) and
# C = 6 (C % 4 != 0: the element-by-element kernel; dk_bn_apply_bf16 takes 4-channel vectors only)
BNX_CASES = [((2, 8, 5, 5), F32), ((2, 8, 5, 5), BF16), ((4, 24), F32), ((2, 12, 3, 3), F32), ((2, 12, 3, 3), BF16),
             ((2, 6, 5, 5), F32)]


@pytest.mark.parametrize("relu", [1, 0], ids=["relu", "norelu"])
@pytest.mark.parametrize("shape,dtype", BNX_CASES,
                         ids=["{}-{}".format("x".join(map(str, s)), STORAGE[d]) for s, d in BNX_CASES])
def test_bnx_equals_apply_then_drop_bitwise(shape, dtype, relu):
    C, p, seed, step, lane = shape[1], 0.5, 31, 2, 1
    rng = np.random.RandomState(C + len(shape))
    x = dev(stored(rng.randn(*shape), dtype), dtype)
    mean, gamma, beta = (torch.as_tensor(rng.randn(C).astype(np.float32), device="cuda") for _ in range(3))
    invstd = torch.as_tensor((rng.rand(C) + 0.5).astype(np.float32), device="cuda")
    bn = (mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), relu)
    st, n, T = stream_handle(), x.numel(), threshold(p)
    fused, applied, unfused = nan_like(x), nan_like(x), nan_like(x)
    getattr(lib, BNX[dtype])(x.data_ptr(), n, T, seed, step, lane, 0, C, *bn, fused.data_ptr(), st)
    getattr(lib, APPLY[dtype])(x.data_ptr(), n, C, *bn, applied.data_ptr(), 0, st)
    getattr(lib, PLAIN[dtype][0])(applied.data_ptr(), n, T, seed, step, lane, 0, unfused.data_ptr(), st)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(fused).any())
    assert np.array_equal(bits(fused), bits(unfused))
    # and the rule over the stored BatchNorm output
    a = storage_order(applied.float().cpu().numpy())
    want = logical(dropout_fwd(a, p, seed, step, lane=lane, storage=STORAGE[dtype]), shape)
    assert np.array_equal(bits(fused), np_bits(want, dtype))


# ---- layer behaviour ----------------------------------------------------------------------------

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


def _bn_chain(C, dims):
    from dorknet_amd.layers.activations import ReLu
    from dorknet_amd.layers.batch_norm import BatchNormLayer
    from dorknet_amd.layers.dropout import DropoutLayer
    r = np.random.RandomState(21)
    bn = BatchNormLayer("bn", input_dimension=dims, incoming_chans=C)
    for k in ("gamma", "beta"):
        bn.learned_params[k] = r.randn(*bn.learned_params[k].shape).astype(np.float32)
    ls = [bn, ReLu("relu"), DropoutLayer("drop", 0.5, seed=8)]
    for l in ls:
        l.to_gpu()
    return ls


@pytest.mark.parametrize("shape,dtype", [((2, 8, 5, 5), F32), ((2, 8, 5, 5), BF16), ((4, 24), F32)],
                         ids=["f32-map", "bf16-map", "f32-rows"])
def test_bn_relu_dropout_fused_equals_unfused_bitwise(shape, dtype, monkeypatch):
    """BatchNormLayer + ReLu + DropoutLayer through the chain executor: with fusion the dropout gets a
    BNOut and runs dk_dropout_fwd_bnx_* (the BN output is never written); y, the gradient at the BN
    input, dgamma and dbeta equal the layer-by-layer run bit for bit, and dx of the dropout is +0.0
    exactly where y was dropped."""
    from dorknet_amd.layers._chain import chain_backward, chain_forward
    rng = np.random.RandomState(sum(shape))
    X, dY = stored(rng.randn(*shape), dtype), stored(rng.randn(*shape), dtype)
    keep = logical(keep_mask(X.size, 0.5, 8, 0, 0), shape)
    outs = []
    for fuse in ("1", "0"):
        monkeypatch.setenv("DORKNET_FUSE", fuse)
        ls = _bn_chain(shape[1], len(shape))
        with monkeypatch.context() as m:
            cnt = _Counter(m, ENTRIES)
            y, steps = chain_forward(ls, dev(X, dtype))
            g = ls[2].backward(dev(dY, dtype))  # the dropout's own gradient
            dx = chain_backward(steps, dev(dY, dtype))
            x_test = dev(X, dtype)
            y_test, _ = chain_forward(ls, x_test, test_mode=True)
        torch.cuda.synchronize()
        want = {k: 0 for k in ENTRIES}
        want[BNX[dtype] if fuse == "1" else PLAIN[dtype][0]] = 1  # the training forward only
        assert cnt.n == want, (fuse, cnt.n)
        assert ls[2].step == 1
        assert y.dtype == dtype and dx.dtype == dtype and tuple(dx.shape) == shape
        assert not bits(y)[~keep].any() and not bits(g)[~keep].any()  # +0.0 where dropped
        assert (bits(g)[keep] != 0).all()                               # dy * scale elsewhere (no dy is 0)
        from dorknet_amd._tensor import as_device
        outs.append({"y": bits(y), "g": bits(g), "dx": bits(dx), "dgamma": bits(ls[0].grads["gamma"]),
                     "dbeta": bits(ls[0].grads["beta"]), "y_test": bits(as_device(y_test, dtype))})
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k


def test_steps_and_test_mode():
    layer = dropout(0.5, 17)
    X = np.random.RandomState(6).randn(5, 4099).astype(np.float32)
    x = dev(X, F32)
    y0, y1 = layer.forward(x), layer.forward(x)
    assert layer.step == 2
    torch.cuda.synchronize()
    k0, k1 = bits(y0) != 0, bits(y1) != 0
    assert np.array_equal(k0.ravel(), keep_mask(X.size, 0.5, 17, 0, 0))
    assert np.array_equal(k1.ravel(), keep_mask(X.size, 0.5, 17, 1, 0))
    assert 0.4 < float((k0 != k1).mean()) < 0.6
    # the backward belongs to the last training forward (step 1)
    dx = layer.backward(x)
    assert np.array_equal(bits(dx), bits(y1))
    state = layer._state
    assert layer.forward(x, test_mode=True) is x and layer.step == 2 and layer._state is state
    layer.lane = 1  # another rank's mask
    y2 = layer.forward(x)
    torch.cuda.synchronize()
    assert np.array_equal((bits(y2) != 0).ravel(), keep_mask(X.size, 0.5, 17, 2, 1))


def test_backward_refusals():
    layer = dropout(0.5, 1)
    g = dev(np.ones((2, 8, 4, 4)), F32)
    with pytest.raises(RuntimeError):
        layer.backward(g)  # no training forward yet
    layer.forward(g, test_mode=True)
    with pytest.raises(RuntimeError):
        layer.backward(g)  # a test-mode forward records nothing
    layer.forward(g)
    with pytest.raises(ValueError):
        layer.backward(dev(np.ones((2, 8, 4, 4)), BF16))
    with pytest.raises(ValueError):
        layer.backward(dev(np.ones((2, 8, 4, 2)), F32))
    tagged = dev(np.ones((2, 8, 4, 4)), F32)
    tagged._dk_lattice = 2
    with pytest.raises(ValueError):
        layer.backward(tagged)
    with pytest.raises(ValueError):
        layer.forward(torch.ones((4, 8), dtype=BF16, device="cuda"))  # bf16 rows
    with pytest.raises(ValueError):
        layer.forward(torch.ones((4, 8, 2), device="cuda"))
    assert layer.step == 1


def test_checkpoint_resumes_the_mask_sequence(tmp_path):
    """Saved after two steps and loaded into a fresh layer: the third forward is the original's."""
    from dorknet_amd.layers.dropout import DropoutLayer
    from dorknet_amd.network.checkpoint import open_h5
    x = dev(np.random.RandomState(7).randn(2, 8, 7, 7), BF16)
    layer = dropout(0.25, 2 ** 40 + 5)
    layer.forward(x)
    layer.forward(x)
    with open_h5(str(tmp_path / "d.h5"), "w") as f:
        layer.save_to_h5(f)
    fresh = DropoutLayer("drop")
    with open_h5(str(tmp_path / "d.h5"), "r") as f:
        fresh.load_from_h5(f)
    fresh.to_gpu()
    assert (fresh.drop_prob, fresh.seed, fresh.step) == (0.25, 2 ** 40 + 5, 2)
    a, b = layer.forward(x), fresh.forward(x)
    torch.cuda.synchronize()
    assert np.array_equal(bits(a), bits(b)) and fresh.step == 3
    # (no input element is zero, so the non-zero outputs are the kept elements: those of step 2)
    assert np.array_equal(bits(b) != 0, logical(keep_mask(x.numel(), 0.25, 2 ** 40 + 5, 2, 0), tuple(x.shape)))


# ---- a small network against the fp64 oracle ----------------------------------------------------

def test_network_step_matches_fp64_oracle():
    """dense 24 -> 16, ReLu, Dropout(0.5), dense 16 -> 5, softmax cross-entropy at batch 6: one step
    against the fp64 oracle layers with ODropout in place (the same mask).  The oracles replay the GPU's
    ReLU decisions (tests/_ties.py); the loss, the probabilities and every gradient are within
    tests/_convert.slack_bound with 1e-4, the fp32 oracle bounding what vanishes in exact arithmetic."""
    from dorknet_amd.layers.activations import ReLu
    from dorknet_amd.layers.dense_layer import DenseLayer
    from dorknet_amd.layers.dropout import DropoutLayer
    from dorknet_amd.layers.losses import SoftmaxWithCrossEntropy
    from dorknet_amd.network.feed_forward_network import FeedForwardNetwork
    from oracle import net as O
    from tests._convert import layer_to_oracle, slack_bound
    from tests._ties import TIE_REL, replay_gpu_decisions, tie_report
    np.random.seed(50)
    net = FeedForwardNetwork("dropped")
    net.add_layer(DenseLayer("dense_1", incoming_chans=24, output_dim=16))
    net.add_layer(ReLu("relu"))
    net.add_layer(DropoutLayer("drop", 0.5, seed=2024))
    net.add_layer(DenseLayer("dense_2", incoming_chans=16, output_dim=5))
    net.set_loss_layer(SoftmaxWithCrossEntropy("softmax"))

    def oracle(dtype):
        ls = [ODropout(l.layer_name, l.drop_prob, l.seed) if isinstance(l, DropoutLayer) else layer_to_oracle(l, dtype)
              for l in net.layers]
        return O.ONetwork(ls, layer_to_oracle(net.loss_layer, dtype))

    onet, o32 = oracle(np.float64), oracle(np.float32)
    net.to_gpu()
    rng = np.random.RandomState(51)
    X = rng.randn(6, 24).astype(np.float32)
    onehot = np.eye(5, dtype=np.float32)[rng.randint(0, 5, 6)]
    loss, P = net.forward(torch.as_tensor(X, device="cuda"), torch.as_tensor(onehot, device="cuda"))
    states = replay_gpu_decisions(net, [onet, o32])
    net.backward()
    torch.cuda.synchronize()
    oloss, oP = onet.forward(X.astype(np.float64), onehot.astype(np.float64))
    o32loss, o32P = o32.forward(X, onehot)
    nties, worst, rows = tie_report(states, onet)
    assert worst <= TIE_REL, rows[:8]
    onet.backward()
    o32.backward()
    assert net.layers[2].step == 1 and onet.layers[2].step == 1
    dropped = int((~onet.layers[2].keep).sum())
    assert 20 <= dropped <= 76  # 96 elements at p = 0.5: the step really drops (7 sigma around 48)

    def excess(got, want64, want32):
        want64 = np.asarray(want64, dtype=np.float64)
        err = np.linalg.norm((np.asarray(got, dtype=np.float64) - want64).ravel())
        return 0.0 if err == 0 else err / max(slack_bound(want64, want32, 1e-4), 1e-300)

    host = lambda t: t.detach().float().cpu().numpy()  # noqa: E731
    assert excess(float(loss), oloss, o32loss) <= 1.0, (float(loss), oloss)
    assert excess(host(P), oP, o32P) <= 1.0
    n = 0
    for l, ol, o3 in zip(net.layers, onet.layers, o32.layers):
        for k in (ol.grads or {}):
            e = excess(host(l.grads[k]), ol.grads[k], o3.grads[k])
            print("{}.{}: {:.3f} of its bound".format(l.layer_name, k, e))
            assert e <= 1.0, (l.layer_name, k, e)
            n += 1
    assert n == 4
