"""LeakyReLu, ReLu6, HardSwish and SiLu on the GPU (dk_act_*: dorknet_amd/csrc/act_math.h, activations.hip, and
act_bwd_bn_partial_kernel in batchnorm.hip).

The arithmetic is a fixed sequence of singly rounded fp32 operations, so the entries are compared bitwise -- fp32 as
int32 bits, bf16 as int16 bits -- with the numpy float32 twin (tests/_activation_twin.py, itself held to fp64 by
tests/test_activation_host.py), the BatchNorm-on-load entries with dk_bn_apply_* followed by the plain entry, and
fused with DORKNET_FUSE=0.  The payload of a NaN is not part of the rule: NaNs are compared by where they are.  Every
output buffer handed to an entry is pre-filled with NaN.  The fp64 partial sums are held to _bn_ref.sum_bound, and only
the whole-network comparison with torch fp64 has a tolerance, the project's normwise 1e-4 (tests/_convert.rel_err).
"""
import numpy as np
import pytest
import torch

from dorknet_amd import _hip
from dorknet_amd._hip import lib, stream_handle
from tests import _activation_twin as T
from tests._bn_ref import CASES as BN_CASES
from tests._bn_ref import make_inputs, sum_bound

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
F32 = torch.float32
STORAGE = {F32: "f32", BF16: "bf16"}
FWD = {F32: "dk_act_fwd_f32", BF16: "dk_act_fwd_bf16"}
FWD_BNX = {F32: "dk_act_fwd_bnx_f32", BF16: "dk_act_fwd_bnx_bf16"}
BWD = {F32: "dk_act_bwd_f32", BF16: "dk_act_bwd_bf16"}
BWD_BNX = {F32: "dk_act_bwd_bnx_f32", BF16: "dk_act_bwd_bnx_bf16"}
APPLY = {F32: "dk_bn_apply_f32", BF16: "dk_bn_apply_bf16"}
NAMES = sorted(T.KINDS)
ALPHA = 0.2
f32 = np.float32


def layer_of(name, layer_name="act"):
    from dorknet_amd.layers import activations as A
    l = A.LeakyReLu(layer_name, alpha=ALPHA) if name == "LeakyReLu" else getattr(A, name)(layer_name)
    l.to_gpu()
    return l


def bits(t):
    """The stored bits of a tensor in its logical order, as a numpy integer array."""
    t = t.detach().contiguous()
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32).cpu().numpy()


def host(t):
    return t.detach().float().cpu().numpy()


def want_bits(a, dtype):
    """The bits the float32 values `a` (bf16-representable for bf16 storage) have in `dtype` storage."""
    a = np.ascontiguousarray(a, dtype=f32)
    return T.bf16_bits(a).view(np.int16) if dtype == BF16 else a.view(np.int32)


def assert_same(got, want, dtype, what=""):
    """got (device tensor) holds `want` (float32 numpy) bit for bit; NaNs by position."""
    g, w = host(got), np.asarray(want, dtype=f32).reshape(tuple(got.shape))
    assert np.array_equal(np.isnan(g), np.isnan(w)), (what, "NaN positions differ")
    ok = ~np.isnan(w)
    gb, wb = bits(got), want_bits(w, dtype).reshape(w.shape)
    bad = np.flatnonzero((gb != wb).ravel() & ok.ravel())
    assert bad.size == 0, (what, bad[:5], g.ravel()[bad[:5]], w.ravel()[bad[:5]])


def flat_dev(a, dtype, offset=0):
    """A flat device buffer of `dtype` holding `a`, starting `offset` elements past a 16-byte boundary."""
    n = a.size
    buf = torch.zeros(n + 8, dtype=dtype, device="cuda")
    buf[offset:offset + n] = torch.as_tensor(np.ascontiguousarray(a, dtype=f32).ravel(), device="cuda").to(dtype)
    return buf, buf[offset:offset + n]


def nan_flat(n, dtype, offset=0):
    buf = torch.full((n + 8,), float("nan"), dtype=dtype, device="cuda")
    return buf, buf[offset:offset + n]


def dev(a, dtype):
    """numpy (logical shape) -> a device tensor of `dtype`, channels-last when 4-D."""
    t = torch.as_tensor(np.ascontiguousarray(a, dtype=f32), device="cuda").to(dtype)
    return t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t.contiguous()


# ---- 1. the plain entries against the twin ----------------------------------------------------------

# (shape, storage type, element offset of every pointer)
ENTRY_CASES = [
    ((3, 37), F32, 0),          # n = 111: a tail of 7
    ((5, 4099), F32, 0),        # odd, and more than one block of 256 threads x 8 elements
    ((2, 6, 5, 5), F32, 0),     # C % 4 != 0 (the plain entries see a flat buffer: n = 300, a tail of 4)
    ((2, 8, 7, 7), BF16, 0),
    ((3, 4, 5, 5), BF16, 0),    # n = 300: a tail of 4
    ((2, 8, 3, 3), F32, 1),     # every pointer one element off: the element-by-element route at C % 4 == 0
]
ENTRY_IDS = ["{}-{}{}".format("x".join(map(str, s)), STORAGE[d], "-off1" if o else "") for s, d, o in ENTRY_CASES]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("shape,dtype,offset", ENTRY_CASES, ids=ENTRY_IDS)
def test_entries_match_twin_bitwise(shape, dtype, offset, name):
    kind = T.KINDS[name]
    v, dy = T.entry_inputs(kind, shape, 0)
    v = T.with_edges(v)   # +-0, the kinks, +-inf, +-1e4, NaN
    bf = dtype == BF16
    n = v.size
    xb, x = flat_dev(v, dtype, offset)
    db, d = flat_dev(dy, dtype, offset)
    yb, y = nan_flat(n, dtype, offset)
    gb, g = nan_flat(n, dtype, offset)
    assert x.data_ptr() % 16 == (offset * x.element_size()) % 16
    getattr(lib, FWD[dtype])(x.data_ptr(), n, kind, ALPHA, y.data_ptr(), stream_handle())
    getattr(lib, BWD[dtype])(x.data_ptr(), d.data_ptr(), n, kind, ALPHA, g.data_ptr(), stream_handle())
    torch.cuda.synchronize()
    assert_same(y, T.forward_stored(kind, v.ravel(), ALPHA, bf), dtype, "forward")
    assert_same(g, T.backward_stored(kind, v.ravel(), dy.ravel(), ALPHA, bf), dtype, "backward")
    for buf in (yb, gb):   # nothing written beside the buffers
        assert bool(torch.isnan(buf[:offset]).all()) and bool(torch.isnan(buf[offset + n:]).all())


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("shape,dtype", [((3, 37), F32), ((2, 6, 5, 5), F32), ((2, 8, 7, 7), BF16)],
                         ids=["rows", "map-c6", "map-bf16"])
def test_layer_matches_twin_bitwise(shape, dtype, name):
    """The layer, handed plain (NCHW-contiguous) tensors: its own layout conversion; seeded by the kink margin."""
    kind = T.KINDS[name]
    seed, (v, dy) = T.seeded(kind, lambda s: T.entry_inputs(kind, shape, s))
    layer = layer_of(name)
    y = layer.forward(torch.as_tensor(v, device="cuda").to(dtype))
    dx = layer.backward(torch.as_tensor(dy, device="cuda").to(dtype))
    state = layer._state
    y_test = layer.forward(torch.as_tensor(v, device="cuda").to(dtype), test_mode=True)
    assert layer._state is state   # a test-mode forward records nothing
    torch.cuda.synchronize()
    for got in (y, dx, y_test):
        assert got.dtype == dtype and tuple(got.shape) == shape
        assert len(shape) == 2 or got.is_contiguous(memory_format=torch.channels_last)
    bf = dtype == BF16
    assert_same(y, T.forward_stored(kind, v, ALPHA, bf), dtype)
    assert_same(y_test, T.forward_stored(kind, v, ALPHA, bf), dtype)
    assert_same(dx, T.backward_stored(kind, v, dy, ALPHA, bf), dtype)
    assert layer._state[0] is None and layer._state[1].data_ptr() != y.data_ptr()   # a reference, no copy of y


# ---- 2. BatchNorm on load, forward --------------------------------------------------------------------

# C = 12: a thread's second group of four channels wraps to channel 0; C = 6: the element-by-element kernel
BNX_CASES = [((2, 8, 5, 5), F32), ((2, 8, 5, 5), BF16), ((4, 24), F32), ((2, 12, 3, 3), F32), ((2, 12, 3, 3), BF16),
             ((2, 6, 5, 5), F32), ((5, 4100), F32)]


def bn_params(rng, C):
    """Arbitrary fp32 (mean, invstd, gamma, beta) on the device, every third gamma negative."""
    gamma = 1 + 0.3 * rng.randn(C)
    gamma[::3] *= -1.0
    arrs = [rng.randn(C) * 0.3, rng.rand(C) + 0.5, gamma, 0.5 * rng.randn(C)]
    return [torch.as_tensor(a.astype(f32), device="cuda") for a in arrs]


@pytest.mark.parametrize("relu", [1, 0], ids=["relu", "norelu"])
@pytest.mark.parametrize("shape,dtype", BNX_CASES,
                         ids=["{}-{}".format("x".join(map(str, s)), STORAGE[d]) for s, d in BNX_CASES])
def test_bnx_forward_equals_apply_then_activate_bitwise(shape, dtype, relu):
    C = shape[1]
    rng = np.random.RandomState(C + len(shape))
    x = dev(T.to_bf16(2.0 * rng.randn(*shape)), dtype)
    params = bn_params(rng, C)
    bn = (*[p.data_ptr() for p in params], relu)
    st, n = stream_handle(), x.numel()
    applied = torch.full_like(x, float("nan"))
    getattr(lib, APPLY[dtype])(x.data_ptr(), n, C, *bn, applied.data_ptr(), 0, st)
    for name in NAMES:
        kind = T.KINDS[name]
        fused, unfused = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
        getattr(lib, FWD_BNX[dtype])(x.data_ptr(), n, C, *bn, kind, ALPHA, fused.data_ptr(), st)
        getattr(lib, FWD[dtype])(applied.data_ptr(), n, kind, ALPHA, unfused.data_ptr(), st)
        torch.cuda.synchronize()
        assert not bool(torch.isnan(fused).any()), name
        assert np.array_equal(bits(fused), bits(unfused)), name
        # and the rule over the stored BatchNorm output
        assert_same(fused, T.forward_stored(kind, host(applied), ALPHA, dtype == BF16), dtype, name)


# ---- 3. the backward that also writes stage 1 of the BatchNorm's backward -------------------------------

# the (P, C) of tests/_bn_ref.CASES that reach each edge of row_geom (the kernel keeps bn_bwd_partial_kernel's geometry
# with the 32-group cap of dk_relu_bwd_bn_partial_*): 1 two reduce blocks with a remainder, 2 idle threads, 4 fewer rows
# than lanes, 6 and 8 several channel slices, 9 the scalar route, 13 every pointer offset by one element
PART_CASES = [(1, F32), (1, BF16), (2, F32), (2, BF16), (4, F32), (4, BF16), (6, F32), (6, BF16), (8, F32), (8, BF16),
              (9, F32), (13, F32)]


@pytest.mark.parametrize("relu", [1, 0], ids=["relu", "norelu"])
@pytest.mark.parametrize("cid,dtype", PART_CASES, ids=["case{}-{}".format(c, STORAGE[d]) for c, d in PART_CASES])
def test_bwd_bnx_gradient_and_partials(cid, dtype, relu):
    d = make_inputs(cid)
    P, C = BN_CASES[cid]
    assert (P, C) == (d["P"], d["C"])
    off = 1 if cid == 13 else 0
    _, x = flat_dev(d["x"], dtype, off)
    _, dy = flat_dev(d["dy"], dtype, off)
    params = [torch.as_tensor(p, device="cuda") for p in d["bn"]]
    ptrs = [p.data_ptr() for p in params]
    st, n = stream_handle(), P * C
    rows, nb = lib.dk_bn_partial_blocks(P, C), lib.dk_bn_workspace_bytes(P, C)
    assert nb == rows * 2 * C * 8
    _, pre = nan_flat(n, dtype, off)       # BN(x) before the ReLU: its decisions
    _, v = nan_flat(n, dtype, off)         # the forward's v, materialised
    getattr(lib, APPLY[dtype])(x.data_ptr(), n, C, *ptrs, 0, pre.data_ptr(), 0, st)
    getattr(lib, APPLY[dtype])(x.data_ptr(), n, C, *ptrs, relu, v.data_ptr(), 0, st)
    torch.cuda.synchronize()
    if relu:
        # the decision is taken on the fp32 value before any bf16 rounding; for bf16 storage the stored sign agrees
        # (rounding keeps the sign, and no case has a positive value below the smallest bf16)
        dead = ~(host(pre) > 0)
    else:
        dead = np.zeros(n, dtype=bool)
    for name in NAMES:
        kind = T.KINDS[name]
        _, plain = nan_flat(n, dtype, off)
        gbuf, g = nan_flat(n, dtype, off)
        part = torch.full((rows, 2, C), float("nan"), dtype=torch.float64, device="cuda")
        getattr(lib, BWD[dtype])(v.data_ptr(), dy.data_ptr(), n, kind, ALPHA, plain.data_ptr(), st)
        r = getattr(lib, BWD_BNX[dtype])(x.data_ptr(), dy.data_ptr(), P, C, *ptrs, relu, kind, ALPHA, g.data_ptr(),
                                         part.data_ptr(), nb, st)
        torch.cuda.synchronize()
        assert r == 0   # nothing was armed: no fold
        want = np.where(dead, f32(0.0), host(plain))
        assert_same(g, want, dtype, name)
        assert bool(torch.isnan(gbuf[:off]).all()) and bool(torch.isnan(gbuf[off + n:]).all())
        # the twin's rule on the materialised v gives the same gradient
        gt, pt, apt = T.backward_bnx(kind, d["x"], d["dy"], d["bn"], relu, ALPHA, dtype == BF16, rows,
                                     v=host(v).reshape(P, C), dead=dead.reshape(P, C))
        assert_same(g, gt.ravel(), dtype, name + " twin")
        got = part.cpu().numpy()
        assert not np.isnan(got).any()
        bound = sum_bound(-(-P // rows), rows, 0, apt)
        err = np.abs(got - pt)
        worst = float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))))
        print("case {} {} {} relu {}: partials worst err / bound {:.3g}".format(cid, STORAGE[dtype], name, relu, worst))
        assert worst <= 1.0, (name, worst)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_bwd_bnx_undersized_workspace_writes_nothing(dtype):
    P, C = 98, 512
    rng = np.random.RandomState(1)
    x, dy = dev(T.to_bf16(rng.randn(P, C)), dtype), dev(T.to_bf16(rng.randn(P, C)), dtype)
    ptrs = [p.data_ptr() for p in bn_params(rng, C)]
    nb = lib.dk_bn_workspace_bytes(P, C)
    g = torch.full_like(x, float("nan"))
    part = torch.full((nb // 8,), float("nan"), dtype=torch.float64, device="cuda")
    with pytest.raises(_hip.HipError, match="workspace too small"):
        getattr(lib, BWD_BNX[dtype])(x.data_ptr(), dy.data_ptr(), P, C, *ptrs, 1, T.SILU, 0.0, g.data_ptr(),
                                     part.data_ptr(), nb - 8, stream_handle())
    torch.cuda.synchronize()
    assert bool(torch.isnan(g).all()) and bool(torch.isnan(part).all())


# ---- 4. the layers through the chain executor ----------------------------------------------------------

def _chain(name, C, dims, with_relu):
    from dorknet_amd.layers.activations import ReLu
    from dorknet_amd.layers.batch_norm import BatchNormLayer
    r = np.random.RandomState(21)
    bn = BatchNormLayer("bn", input_dimension=dims, incoming_chans=C)
    for k in ("gamma", "beta"):
        bn.learned_params[k] = r.randn(*bn.learned_params[k].shape).astype(f32)
    ls = [bn] + ([ReLu("relu")] if with_relu else []) + [layer_of(name)]
    for l in ls[:-1]:
        l.to_gpu()
    return ls


class _Calls:
    """Counts the calls of some lib entry points (a wrapper set on the lib object, not a change of the library)."""

    def __init__(self, monkeypatch, names):
        self.n = {k: 0 for k in names}
        for k in names:
            monkeypatch.setattr(lib, k, self._wrap(k, getattr(lib, k)), raising=False)

    def _wrap(self, name, fn):
        def call(*a):
            self.n[name] += 1
            return fn(*a)
        return call


def _watch_pending(monkeypatch):
    """Record BatchNormLayer._pending_bwd before and after each BatchNormLayer backward."""
    from dorknet_amd.layers.batch_norm import BatchNormLayer
    seen = []
    inner = BatchNormLayer._backward

    def watched(self, upstream_dx, relu, defer=False):
        before = getattr(self, "_pending_bwd", None)
        out = inner(self, upstream_dx, relu, defer=defer)
        seen.append((before, getattr(self, "_pending_bwd", None), upstream_dx))
        return out
    monkeypatch.setattr(BatchNormLayer, "_backward", watched)
    return seen


CHAIN_CASES = [((2, 8, 5, 5), F32, False), ((2, 8, 5, 5), F32, True), ((2, 8, 5, 5), BF16, False),
               ((2, 8, 5, 5), BF16, True), ((6, 24), F32, False), ((6, 24), F32, True), ((3, 6, 5, 5), F32, True)]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("shape,dtype,with_relu", CHAIN_CASES,
                         ids=["{}-{}{}".format("x".join(map(str, s)), STORAGE[d], "-relu" if r else "")
                              for s, d, r in CHAIN_CASES])
def test_bn_activation_fused_equals_unfused_bitwise(shape, dtype, with_relu, name, monkeypatch):
    """BatchNormLayer [+ ReLu] + activation through layers/_chain: fused, the activation takes a BNOut (the BN output
    is never written), its backward hands stage 1 of the BatchNorm's backward over, and the BatchNorm consumes it
    instead of running its one-shot dk_bn_bwd_*.  y, dx, dgamma and dbeta equal the layer-by-layer run bit for bit."""
    from dorknet_amd._tensor import as_device
    from dorknet_amd.layers._chain import chain_backward, execute
    from dorknet_amd.layers._bn_input import BNOut
    rng = np.random.RandomState(sum(shape))
    X, dY = T.to_bf16(2.0 * rng.randn(*shape)), T.to_bf16(rng.randn(*shape))
    watched = [FWD[dtype], FWD_BNX[dtype], BWD[dtype], BWD_BNX[dtype], "dk_bn_bwd_f32", "dk_bn_bwd_bf16",
               "dk_bn_apply_f32", "dk_bn_apply_bf16"]
    outs = []
    for fuse in ("1", "0"):
        monkeypatch.setenv("DORKNET_FUSE", fuse)
        ls = _chain(name, shape[1], len(shape), with_relu)
        with monkeypatch.context() as m:
            cnt = _Calls(m, watched)
            seen = _watch_pending(m)
            y, steps, _ = execute(ls, dev(X, dtype))
            dx = chain_backward(steps, dev(dY, dtype))
            state = ls[-1]._state
            y_test, _, _ = execute(ls, dev(X, dtype), test_mode=True)
        torch.cuda.synchronize()
        assert ls[-1]._state is state
        assert y.dtype == dtype and dx.dtype == dtype and tuple(dx.shape) == shape and tuple(y.shape) == shape
        assert len(seen) == 1
        before, after, g = seen[0]
        if fuse == "1":
            assert isinstance(state[0], BNOut) and state[0].owner is ls[0]
            assert state[1].data_ptr() == ls[0].X.data_ptr()   # the BatchNorm's raw input: a reference, no copy
            assert cnt.n[FWD_BNX[dtype]] == 2 and cnt.n[BWD_BNX[dtype]] == 1, cnt.n   # (training + test forward)
            assert cnt.n[FWD[dtype]] == 0 and cnt.n[BWD[dtype]] == 0, cnt.n
            assert cnt.n["dk_bn_apply_f32"] == 0 and cnt.n["dk_bn_apply_bf16"] == 0, cnt.n   # never materialised
            # the BatchNorm took the handed partials, not its one-shot backward
            assert before is not None and before[0] is g and before[1].dtype == torch.float64
            assert tuple(before[1].shape) == (lib.dk_bn_partial_blocks(X.size // shape[1], shape[1]), 2, shape[1])
            assert after is None
            assert cnt.n["dk_bn_bwd_f32"] == 0 and cnt.n["dk_bn_bwd_bf16"] == 0, cnt.n
        else:
            assert state[0] is None and before is None and after is None
            assert cnt.n[FWD[dtype]] == 2 and cnt.n[BWD[dtype]] == 1 and cnt.n[BWD_BNX[dtype]] == 0, cnt.n
            assert cnt.n["dk_bn_bwd_f32"] + cnt.n["dk_bn_bwd_bf16"] == 1, cnt.n
        outs.append({"y": bits(y), "dx": bits(dx), "dgamma": bits(ls[0].grads["gamma"]),
                     "dbeta": bits(ls[0].grads["beta"]), "y_test": bits(as_device(y_test, dtype))})
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k
    assert outs[0]["dgamma"].any() and outs[0]["dx"].any()


def test_stale_bnout_raises_and_errors_leave_no_arming(monkeypatch):
    """Every refusal is a Python exception before any launch and leaves no in-launch fold armed: the fused step that
    follows gives the bits of a run that met no error."""
    from dorknet_amd.layers._chain import chain_backward, execute
    monkeypatch.setenv("DORKNET_FUSE", "1")
    shape = (2, 8, 5, 5)
    rng = np.random.RandomState(3)
    X, dY = T.to_bf16(2.0 * rng.randn(*shape)), T.to_bf16(rng.randn(*shape))

    def step(ls):
        y, steps, _ = execute(ls, dev(X, F32))
        dx = chain_backward(steps, dev(dY, F32))
        torch.cuda.synchronize()
        return bits(y), bits(dx), bits(ls[0].grads["gamma"]), bits(ls[0].grads["beta"])

    clean = step(_chain("SiLu", 8, 4, False))
    ls = _chain("SiLu", 8, 4, False)
    bn, act = ls
    with monkeypatch.context() as m:
        cnt = _Calls(m, [BWD[F32], BWD_BNX[F32], BWD[BF16], BWD_BNX[BF16], FWD[BF16]])
        with pytest.raises(RuntimeError):
            act.backward(dev(dY, F32))   # no training forward yet
        act.forward(dev(X, F32), test_mode=True)
        with pytest.raises(RuntimeError):
            act.backward(dev(dY, F32))   # a test-mode forward records nothing
        execute(ls, dev(X, F32))
        with pytest.raises(ValueError):
            act.backward(dev(dY, BF16))  # mixed storage types
        with pytest.raises(ValueError):
            act.backward(dev(dY[:, :, :, :4], F32))   # a shape mismatch
        tagged = dev(dY, F32)
        tagged._dk_lattice = 2
        with pytest.raises(ValueError):
            act.backward(tagged)         # a lattice-form gradient
        with pytest.raises(ValueError):
            act.forward(torch.ones((4, 8), dtype=BF16, device="cuda"))   # bf16 rows
        with pytest.raises(ValueError):
            act.forward(torch.ones((4, 8, 2), device="cuda"))
        # a BNOut used after its owner's next forward
        execute(ls, dev(X, F32))
        bn.forward(dev(X + 1, F32))
        with pytest.raises(RuntimeError, match="next forward"):
            act.backward(dev(dY, F32))
        assert cnt.n == {k: 0 for k in cnt.n}, cnt.n   # no launch
    assert getattr(bn, "_pending_bwd", None) is None
    again = step(ls)
    for a, b in zip(clean, again):
        assert np.array_equal(a, b)


# ---- 5. a small network ---------------------------------------------------------------------------------

NET_MARGIN = 2.0 ** -13   # |v - kink| of every activation input: v < 16 carries far less fp32 error than this

# The network: conv 3x3 (pad 1) - BN - HardSwish - depthwise 3x3 (pad 0: 12 x 12 -> 10 x 10) - BN - ReLu6 - pointwise -
# BN - SiLu - GAP - dense - LeakyReLu - dense - loss; no bias in front of a BatchNorm (its gradient vanishes in exact
# arithmetic, so a normwise bound says nothing about it).  The depthwise layer is unpadded on purpose: a 3x3, padding 1,
# bias-free depthwise layer under DORKNET_FUSE=1 takes its own one-pass backward (dk_dwconv_bwd_bnbwd_*), whose weight
# gradient is summed in another order than dk_dwconv_wgrad_*'s (and which, for bf16, never stores dy), so fused and
# unfused differ in that layer's last bits with plain ReLu layers too -- measured on this network with ReLu in every
# activation's place: dw weights 4.5e-7 normwise (fp32).  Unpadded, every layer but the BatchNorm + activation pairs
# runs the same kernels either way, and the comparison is about what this file tests.


def _net_arrays(seed):
    """Weights and a batch for the network below, from one seed."""
    r = np.random.RandomState(31000 + seed)
    a = {"conv": 0.3 * r.randn(8, 8, 3, 3), "dw": 0.5 * r.randn(8, 3, 3), "pw": 0.5 * r.randn(8, 8),
         "d1": 0.6 * r.randn(8, 16), "b1": 0.3 * r.randn(16), "d2": 0.6 * r.randn(16, 5), "b2": 0.3 * r.randn(5)}
    for i in (1, 2, 3):
        a["gamma%d" % i] = 1 + 0.3 * r.randn(1, 8, 1, 1)
        a["beta%d" % i] = 0.5 * r.randn(1, 8, 1, 1)
    a = {k: v.astype(f32) for k, v in a.items()}
    a["X"] = T.to_bf16(r.randn(4, 8, 12, 12))
    a["onehot"] = np.eye(5, dtype=f32)[r.randint(0, 5, 4)]
    return a


def _build_net(a):
    from dorknet_amd.layers.activations import HardSwish, LeakyReLu, ReLu6, SiLu
    from dorknet_amd.layers.batch_norm import BatchNormLayer
    from dorknet_amd.layers.convolution import ConvLayer
    from dorknet_amd.layers.dense_layer import DenseLayer
    from dorknet_amd.layers.depthwise_convolution import DepthwiseConvLayer
    from dorknet_amd.layers.losses import SoftmaxWithCrossEntropy
    from dorknet_amd.layers.pointwise_convolution import PointwiseConvLayer
    from dorknet_amd.layers.pooling import GlobalAveragePoolingLayer
    from dorknet_amd.network.feed_forward_network import FeedForwardNetwork
    net = FeedForwardNetwork("acts")
    layers = [ConvLayer("conv", filter_block_shape=(8, 8, 3, 3), with_bias=False),
              BatchNormLayer("bn1", incoming_chans=8), HardSwish("hswish"),
              DepthwiseConvLayer("dw", filter_block_shape=(8, 3, 3), padding=0, with_bias=False),
              BatchNormLayer("bn2", incoming_chans=8), ReLu6("relu6"),
              PointwiseConvLayer("pw", filter_block_shape=(8, 8), with_bias=False),
              BatchNormLayer("bn3", incoming_chans=8), SiLu("silu"),
              GlobalAveragePoolingLayer("gap"),
              DenseLayer("dense_1", incoming_chans=8, output_dim=16), LeakyReLu("leaky", alpha=ALPHA),
              DenseLayer("dense_2", incoming_chans=16, output_dim=5)]
    for l in layers:
        net.add_layer(l)
    net.set_loss_layer(SoftmaxWithCrossEntropy("softmax"))
    by = {l.layer_name: l for l in layers}
    for name, key in (("conv", "conv"), ("dw", "dw"), ("pw", "pw"), ("dense_1", "d1"), ("dense_2", "d2")):
        by[name].learned_params["weights"] = a[key].copy()
    by["dense_1"].learned_params["bias"] = a["b1"].copy()
    by["dense_2"].learned_params["bias"] = a["b2"].copy()
    for i in (1, 2, 3):
        by["bn%d" % i].learned_params["gamma"] = a["gamma%d" % i].copy()
        by["bn%d" % i].learned_params["beta"] = a["beta%d" % i].copy()
    return net


def _torch_step(a):
    """The same step in torch CPU fp64 autograd: (loss, input gradient, parameter gradients, least kink margin)."""
    import torch.nn.functional as F
    t = {k: torch.tensor(np.asarray(v, dtype=np.float64), requires_grad=k != "onehot") for k, v in a.items()}
    margins = []

    def bn(x, i):
        m = x.mean(dim=(0, 2, 3), keepdim=True)
        var = ((x - m) ** 2).mean(dim=(0, 2, 3), keepdim=True)
        return t["gamma%d" % i] * (x - m) / torch.sqrt(var + 1e-5) + t["beta%d" % i]

    def act(kind, fn, v):
        margins.append(T.kink_margin(kind, v.detach().numpy()))
        return fn(v)

    h = F.conv2d(t["X"], t["conv"], padding=1)
    h = act(T.HARDSWISH, F.hardswish, bn(h, 1))
    h = F.conv2d(h, t["dw"].unsqueeze(1), padding=0, groups=8)
    h = act(T.RELU6, F.relu6, bn(h, 2))
    h = F.conv2d(h, t["pw"][:, :, None, None])
    h = act(T.SILU, F.silu, bn(h, 3))
    h = h.mean(dim=(2, 3))
    h = act(T.LEAKY, lambda v: F.leaky_relu(v, float(f32(ALPHA))), h @ t["d1"] + t["b1"])
    logits = h @ t["d2"] + t["b2"]
    loss = -(F.log_softmax(logits, dim=1) * t["onehot"]).sum(dim=1).mean()
    loss.backward()
    grads = {k: v.grad.numpy() for k, v in t.items() if v.requires_grad and k != "X"}
    return float(loss), t["X"].grad.numpy(), grads, min(margins)


GRAD_KEYS = {"conv": ("conv", "weights"), "dw": ("dw", "weights"), "pw": ("pw", "weights"), "d1": ("dense_1", "weights"),
             "b1": ("dense_1", "bias"), "d2": ("dense_2", "weights"), "b2": ("dense_2", "bias"),
             "gamma1": ("bn1", "gamma"), "beta1": ("bn1", "beta"), "gamma2": ("bn2", "gamma"), "beta2": ("bn2", "beta"),
             "gamma3": ("bn3", "gamma"), "beta3": ("bn3", "beta")}


def _gpu_step(a, dtype, fuse, monkeypatch):
    monkeypatch.setenv("DORKNET_FUSE", fuse)
    net = _build_net(a)
    net.to_gpu()
    X = dev(a["X"], dtype)
    loss, P = net.forward(X, torch.as_tensor(a["onehot"], device="cuda"))
    dX = net.backward(input_grad=True)
    torch.cuda.synchronize()
    by = {l.layer_name: l for l in net.layers}
    grads = {k: by[ln].grads[p] for k, (ln, p) in GRAD_KEYS.items()}
    return net, loss, P, dX, grads


@pytest.fixture(scope="module")
def net_case():
    """The first seed of 0, 1, 2, ... at which every activation input keeps NET_MARGIN from its kinks, its arrays and
    the torch fp64 step (computed once, shared, left unchanged)."""
    for seed in range(200):
        a = _net_arrays(seed)
        ref = _torch_step(a)
        if ref[3] >= NET_MARGIN:
            return seed, a, ref
    raise AssertionError("no seed below 200 keeps the kink margin")


def test_network_step_fused_unfused_and_fp64(net_case, monkeypatch):
    """The network above, batch 4, 8 channels, 12 x 12, fp32: fused equals unfused bit for bit, and the loss, the input gradient and every
    parameter gradient are within the normwise 1e-4 of torch CPU fp64 autograd."""
    from dorknet_amd.layers._bn_input import BNOut
    from tests._convert import rel_err
    seed, a, (rloss, rdX, rgrads, margin) = net_case
    print("network seed {} (least kink margin {:.3g})".format(seed, margin))
    assert margin >= NET_MARGIN
    net, loss, P, dX, grads = _gpu_step(a, F32, "1", monkeypatch)
    by = {l.layer_name: l for l in net.layers}
    for n in ("hswish", "relu6", "silu"):
        assert isinstance(by[n]._state[0], BNOut), n   # the three maps took their BatchNorm on load
    assert by["leaky"]._state[0] is None
    _, loss0, P0, dX0, grads0 = _gpu_step(a, F32, "0", monkeypatch)
    assert np.array_equal(bits(loss), bits(loss0)) and np.array_equal(bits(P), bits(P0))
    assert np.array_equal(bits(dX), bits(dX0))
    for k in grads:
        assert np.array_equal(bits(grads[k]), bits(grads0[k])), k
    assert abs(float(loss) - rloss) <= 1e-4 * abs(rloss), (float(loss), rloss)
    e = rel_err(host(dX), rdX)
    print("input gradient: {:.3g}".format(e))
    assert e <= 1e-4
    assert set(grads) == set(rgrads)
    for k in sorted(grads):
        e = rel_err(host(grads[k]).reshape(rgrads[k].shape), rgrads[k])
        print("{}: {:.3g}".format(k, e))
        assert e <= 1e-4, (k, e)


def test_network_step_bf16_fused_equals_unfused(net_case, monkeypatch):
    """The same network on a bf16 input (bf16 maps up to the pool, an fp32 head): fused equals unfused bit for bit."""
    _, a, _ = net_case
    net, loss, P, dX, grads = _gpu_step(a, BF16, "1", monkeypatch)
    by = {l.layer_name: l for l in net.layers}
    assert by["silu"]._state[3] == BF16 and by["leaky"]._state[3] == F32
    _, loss0, P0, dX0, grads0 = _gpu_step(a, BF16, "0", monkeypatch)
    assert dX.dtype == BF16 and np.isfinite(float(loss))
    assert np.array_equal(bits(loss), bits(loss0)) and np.array_equal(bits(P), bits(P0))
    assert np.array_equal(bits(dX), bits(dX0))
    for k in grads:
        assert np.array_equal(bits(grads[k]), bits(grads0[k])), k


# ---- 6. checkpoint --------------------------------------------------------------------------------------

def test_checkpoint_round_trip_on_the_gpu(net_case, tmp_path, monkeypatch):
    from dorknet_amd.layers.activations import HardSwish, LeakyReLu, ReLu6, SiLu
    from dorknet_amd.network.feed_forward_network import FeedForwardNetwork
    _, a, _ = net_case
    net, _, _, _, _ = _gpu_step(a, F32, "1", monkeypatch)   # one training step: the running statistics exist
    h5f, js = str(tmp_path / "w.h5"), str(tmp_path / "s.json")
    net.save_weights_to_h5(h5f)
    net.save_layer_structure_to_json(js)
    fresh = FeedForwardNetwork("x")
    fresh.load_network_from_json_and_h5(js, h5f)
    fresh.to_gpu()
    kinds = [type(l) for l in fresh.layers if type(l) in (HardSwish, LeakyReLu, ReLu6, SiLu)]
    assert kinds == [HardSwish, ReLu6, SiLu, LeakyReLu]
    assert [l.alpha for l in fresh.layers if type(l) is LeakyReLu] == [ALPHA]
    X = dev(a["X"], F32)
    _, p0 = net.forward(X, None, test_mode=True)
    _, p1 = fresh.forward(X, None, test_mode=True)
    torch.cuda.synchronize()
    assert np.array_equal(bits(p0), bits(p1)) and bool(torch.isfinite(p1).all())
