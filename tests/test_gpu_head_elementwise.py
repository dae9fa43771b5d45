"""Every output element of the classifier head's entry points -- dk_gap_{fwd,bwd}_{f32,bf16}, dk_gap_join_fwd_f32,
dk_dense_{fwd,dgrad,wgrad}_f32, dk_softmax_xent_{fwd,bwd}_f32, dk_colsum_{f32,bf16}, dk_l2_loss_f32,
dk_l2_loss_multi_f32 -- against the fp64 reference of the same operation under the bound derived in tests/_head_ref.py
from the kernel's arithmetic, none excluded; and the exact kernels around them -- dk_relu_{fwd,bwd}_{f32,bf16},
dk_add_{f32,bf16}, dk_scale_f32, dk_mask_to_f32, dk_cast_*, dk_nchw_to_nhwc_f32, dk_nhwc_unpad_f32 -- bit for bit
against numpy / torch-CPU / index arithmetic, special values included.  The cases (tables of tests/_head_ref.py) are
the smallest that reach each code path; their comments say which.

The dense entry points run twice: under the default knobs and with the row tile forced to configuration 16 and the
split-K tile to the one the shape does not pick (dk_debug_set_gemm_config, restored in a finally).

Outputs are guarded (tests/_guard.py): slices of sentinel-filled buffers whose 64-element margins must stay intact
and in which no element may remain unwritten; a refused call must leave all of it untouched.

Worst err / bound per family on an MI355X (recorded with DORKNET_SLACK_LOG; results, not tolerances):

    family                                      checks   worst
    gap forward, fp32 / bf16                     8 / 8   0.052 / 0.052
    gap backward dx, fp32 / bf16               12 / 12   0.774 / 1.000 (the interval form's end, attained by a
                                                         correct round-to-nearest-even store by construction)
    gap join (pooled ReLU(bnA(a) + bnB(b)))         16   0.090
    column sums, fp32 / bf16                     7 / 7   0.745 / 0.745 (the one fp32 cast against its half ulp)
    l2 overwrite / accumulate / multi        6 / 6 / 5   0.846 / 0.555 / 0.575 (the same: one cast)
    softmax P / loss / dx                 16 / 14 / 14   0.219 / 0.166 / 0.599
    dense y / dx / dw                     32 / 16 / 32   0.064 / 0.106 / 0.099
    exact kernels                                        bitwise, special values and subnormals included

P and the loss stay under a quarter of bounds that rest on the one-ulp ASSUMPTION for expf and logf
(tests/_head_ref.py), so that assumption is not strained; no bound was met only through it.  Subnormal operands and
results of relu, add, scale and both casts equal the IEEE reference bit for bit: nothing flushes them.  No kernel or
host defect was found; no fp32 entry point needed a new refusal.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

from dorknet_amd._hip import HipError, lib, stream_handle, workspace
from tests import _head_ref as R
from tests._guard import Guarded
from tests._optim_twin import ieee_host

pytestmark = pytest.mark.gpu

F32, BF16, U8 = torch.float32, torch.bfloat16, torch.uint8
f32 = np.float32
ROUTES = ("default", "forced")
ZERO5 = (0, 0, 0, 0, 0)
ARGS, WORKSPACE = 10001, 10002


def dev(a, dtype=F32, offset=0):
    """A host array on the device as `dtype`; offset: that many elements past a 16-byte-aligned address."""
    t = torch.as_tensor(np.ascontiguousarray(a))
    with ieee_host():   # (a host thread that flushes subnormals must not flush them in a conversion)
        t = t.to(torch.float32).to(dtype) if dtype in (F32, BF16) else t.to(dtype)
    buf = torch.empty(t.numel() + offset, dtype=dtype, device="cuda")
    out = buf[offset:]
    out.copy_(t.reshape(-1))
    assert (out.data_ptr() - offset * out.element_size()) % 16 == 0
    return out


def refused(code, fn, *args):
    with pytest.raises(HipError, match=str(code)):
        fn(*args)


def untouched(*bufs):
    for b in bufs:
        assert b.untouched(), "a refused call wrote its output"


def same(name, got, want):
    assert R.same_bits(got, want), "{}: first difference at {}".format(
        name, int(np.flatnonzero(np.ascontiguousarray(got, dtype=f32).view(np.uint32).ravel()
                                 != np.ascontiguousarray(want, dtype=f32).view(np.uint32).ravel())[0]))


# ---------------------------------------------------------------------------------------------------------
# global average pooling
# ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def gap_in(name):
    return R.gap_inputs(name)


@pytest.mark.parametrize("name", list(R.GAP))
def test_gap_forward(name):
    d, sh = gap_in(name), stream_handle()
    N, HW, C = d["N"], d["HW"], d["C"]
    r = R.gap_fwd(d["x"])
    for dtype, fn in ((F32, lib.dk_gap_fwd_f32), (BF16, lib.dk_gap_fwd_bf16)):
        x, out = dev(d["x"], dtype), Guarded((N, C), F32)
        assert fn(x.data_ptr(), N, HW, C, out.ptr, sh) == 0
        R.check("gap fwd {} {}".format(name, dtype), out.result(), r.ref, r.A)


def gap_backward_pair(name, tag, dy_off, dx_off):
    """Both storage types at the given dy / dx offsets (elements); the bf16 dx against its own bound and bitwise
    against what the fp32 entry's dx rounds to."""
    d, sh = gap_in(name), stream_handle()
    N, HW, C = d["N"], d["HW"], d["C"]
    r = R.gap_bwd(d["dy"], HW)
    dy = dev(d["dy"], F32, dy_off)
    dx = Guarded((N, HW, C), F32, dx_off)
    assert lib.dk_gap_bwd_f32(dy.data_ptr(), N, HW, C, dx.ptr, sh) == 0
    got = dx.result()
    R.check("gap bwd {} {} f32".format(name, tag), got, r.ref, r.A)
    dx16 = Guarded((N, HW, C), BF16, dx_off)
    assert lib.dk_gap_bwd_bf16(dy.data_ptr(), N, HW, C, dx16.ptr, sh) == 0
    got16 = dx16.result()
    R.check("gap bwd {} {} bf16".format(name, tag), got16, r.ref, r.b16)
    assert np.array_equal(got16.astype(f32), R.q16(got.astype(f32))), "bf16 dx is not the rounded fp32 dx"


@pytest.mark.parametrize("name", list(R.GAP))
def test_gap_backward(name):
    gap_backward_pair(name, "aligned", 0, 0)


@pytest.mark.parametrize("name", R.GAP_MISALIGNED)
def test_gap_backward_scalar_route_by_pointer(name):
    assert R.GAP[name][2] % 4 == 0
    gap_backward_pair(name, "dy+1", 1, 0)
    gap_backward_pair(name, "dx+1", 0, 1)


@pytest.mark.parametrize("variant", R.JOIN_VARIANTS)
@pytest.mark.parametrize("name", R.GAP_JOIN)
def test_gap_join(name, variant):
    d, sh = gap_in(name), stream_handle()
    N, HW, C = d["N"], d["HW"], d["C"]
    a_relu, b_relu = variant
    r = R.gap_join(d, a_relu, b_relu)
    assert r.margin > 1
    a, b = dev(d["a"]), dev(d["b"])
    pa, pb = [dev(v) for v in d["pa"]], [dev(v) for v in d["pb"]]
    aa = ZERO5 if a_relu is None else (*(t.data_ptr() for t in pa), a_relu)
    ba = ZERO5 if b_relu is None else (*(t.data_ptr() for t in pb), b_relu)
    for with_mask in (True, False):
        out, mask = Guarded((N, C), F32), Guarded((N, HW, C), U8)
        assert lib.dk_gap_join_fwd_f32(a.data_ptr(), *aa, b.data_ptr(), *ba, N, HW, C, mask.ptr if with_mask else 0,
                                       out.ptr, sh) == 0
        R.check("gap join {} {}".format(name, variant), out.result(), r.ref, r.A)
        if with_mask:
            assert np.array_equal(mask.raw(), r.mask)
        else:
            untouched(mask)


# ---------------------------------------------------------------------------------------------------------
# column sums
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.COLSUM))
def test_colsum(name):
    M, N = R.COLSUM[name]
    x, sh = R.colsum_inputs(name), stream_handle()
    r = R.colsum(x)
    nb = lib.dk_colsum_workspace_bytes(M, N)
    assert nb == R.colsum_chunks(M) * N * 8
    for dtype, fn in ((F32, lib.dk_colsum_f32), (BF16, lib.dk_colsum_bf16)):
        xd, out = dev(x, dtype), Guarded((N,), F32)
        assert fn(xd.data_ptr(), M, N, out.ptr, workspace.get(nb), nb, sh) == 0
        R.check("colsum {} {}".format(name, dtype), out.result(), r.ref, r.A)
        refused(WORKSPACE, fn, xd.data_ptr(), M, N, out.ptr, workspace.get(nb), nb - 1, sh)


# ---------------------------------------------------------------------------------------------------------
# l2
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", R.L2_N)
def test_l2(n):
    w, sh = R.l2_weights(n, n), stream_handle()
    wd = dev(w)
    out = Guarded((1,), F32)
    assert lib.dk_l2_loss_f32(wd.data_ptr(), n, R.L2, 0, out.ptr, sh) == 0
    r = R.l2(w, R.L2)
    R.check("l2 {} overwrite".format(n), out.result(), r.ref, r.A)
    out = Guarded((1,), F32)
    out.buf[out.lead] = R.L2_PRIOR
    assert lib.dk_l2_loss_f32(wd.data_ptr(), n, R.L2, 1, out.ptr, sh) == 0
    r = R.l2(w, R.L2, R.L2_PRIOR)
    R.check("l2 {} accumulate".format(n), out.result(), r.ref, r.A)


def l2_table(name):
    ws, strengths = R.l2_table_inputs(name)
    wd = [dev(w) for w in ws]
    sizes = [len(w) for w in ws]
    raw = R.l2_table_bytes([t.data_ptr() for t in wd], sizes, strengths)
    assert len(raw) == 32 * len(ws)
    table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    return ws, strengths, wd, table, R.l2_blocks(sizes)[1]


@pytest.mark.parametrize("with_add", (False, True))
@pytest.mark.parametrize("name", list(R.L2_TABLES))
def test_l2_multi(name, with_add):
    ws, strengths, wd, table, blocks = l2_table(name)
    sh = stream_handle()
    nb = lib.dk_l2_multi_workspace_bytes(blocks)
    assert nb == 8 * blocks
    add_to = dev(np.array([R.L2_ADD_TO], dtype=f32)) if with_add else None
    out = Guarded((1,), F32)
    assert lib.dk_l2_loss_multi_f32(table.data_ptr(), len(ws), blocks, add_to.data_ptr() if with_add else 0, out.ptr,
                                    workspace.get(nb), nb, sh) == 0
    r = R.l2_multi(ws, strengths, float(f32(R.L2_ADD_TO)) if with_add else None)
    R.check("l2 multi {} add_to={}".format(name, with_add), out.result(), r.ref, r.A)


# ---------------------------------------------------------------------------------------------------------
# softmax with cross-entropy
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.SOFTMAX))
def test_softmax_xent(name):
    c, sh = R.SOFTMAX[name], stream_handle()
    x, y = R.softmax_inputs(name)
    r = R.softmax(x, y)
    xd = dev(x, F32, 1 if c.offset == "x" else 0)
    yd = None if y is None else dev(y, F32, 1 if c.offset == "y" else 0)
    P, loss = Guarded((c.B, c.K), F32), Guarded((1,), F32)
    assert lib.dk_softmax_xent_fwd_f32(xd.data_ptr(), 0 if y is None else yd.data_ptr(), c.B, c.K, P.ptr,
                                       0 if y is None else loss.ptr, sh) == 0
    got = P.result()
    R.check("softmax {} P".format(name), got, r.ref, r.A)
    if y is None:
        untouched(loss)
        return
    R.check("softmax {} loss".format(name), loss.result(), r.loss, r.eloss)
    dx = Guarded((c.B, c.K), F32)
    assert lib.dk_softmax_xent_bwd_f32(P.ptr, yd.data_ptr(), c.B, c.K, dx.ptr, sh) == 0
    rb = R.softmax_bwd(got, y)
    R.check("softmax {} dx".format(name), dx.result(), rb.ref, rb.A)


# ---------------------------------------------------------------------------------------------------------
# dense layer
# ---------------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def routing(route, IN, OUT):
    """"forced": row tile 16 (128 x 128 x 32) and the split-K tile the shape does not pick."""
    if route == "default":
        yield
        return
    try:
        lib.dk_debug_set_gemm_config(0, 16)
        lib.dk_debug_set_gemm_config(1, 1 if R.dense_wgrad_config(IN, OUT) == 6 else 6)
        yield
    finally:
        lib.dk_debug_set_gemm_config(0, -1)
        lib.dk_debug_set_gemm_config(1, -1)


@functools.lru_cache(maxsize=None)
def dense_in(name):
    return R.dense_inputs(name)


def dense_calls(name, route, tag, in_off, out_off):
    d, sh = dense_in(name), stream_handle()
    B, IN, OUT = d["B"], d["IN"], d["OUT"]
    x, dy, w = dev(d["x"], F32, in_off), dev(d["dy"], F32, in_off), dev(d["w"], F32, in_off)
    bias = dev(d["bias"], F32, out_off)
    tag = "{} {} {}".format(name, route, tag)
    with routing(route, IN, OUT):
        for with_bias in (False, True):
            y = Guarded((B, OUT), F32, out_off)
            assert lib.dk_dense_fwd_f32(x.data_ptr(), B, IN, w.data_ptr(), OUT, bias.data_ptr() if with_bias else 0,
                                        y.ptr, sh) == 0
            r = R.dense_fwd(d, with_bias)
            R.check("dense fwd {} bias={}".format(tag, with_bias), y.result(), r.ref, r.A)
        dx = Guarded((B, IN), F32, out_off)
        assert lib.dk_dense_dgrad_f32(dy.data_ptr(), B, OUT, w.data_ptr(), IN, dx.ptr, sh) == 0
        r = R.dense_dgrad(d)
        R.check("dense dgrad {}".format(tag), dx.result(), r.ref, r.A)
        nb = lib.dk_dense_wgrad_workspace_bytes(B, IN, OUT)
        assert nb >= IN * OUT * 4
        for l2 in (0.0, R.L2):
            dw = Guarded((IN, OUT), F32, out_off)
            assert lib.dk_dense_wgrad_f32(x.data_ptr(), dy.data_ptr(), B, IN, OUT, w.data_ptr() if l2 else 0, l2, dw.ptr,
                                          workspace.get(nb), nb, sh) == 0
            r = R.dense_wgrad(d, l2)
            R.check("dense wgrad {} l2={}".format(tag, l2), dw.result(), r.ref, r.A)
        dw = Guarded((IN, OUT), F32, out_off)
        refused(WORKSPACE, lib.dk_dense_wgrad_f32, x.data_ptr(), dy.data_ptr(), B, IN, OUT, 0, 0.0, dw.ptr,
                workspace.get(nb), nb - 1, sh)
        untouched(dw)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", list(R.DENSE))
def test_dense(name, route):
    dense_calls(name, route, "aligned", 0, 0)


@pytest.mark.parametrize("route", ROUTES)
def test_dense_scalar_loaders_by_pointer(route):
    dense_calls(R.DENSE_OFFSET_IN, route, "inputs+1", 1, 0)


@pytest.mark.parametrize("route", ROUTES)
def test_dense_scalar_epilogue_by_pointer(route):
    dense_calls(R.DENSE_OFFSET_OUT, route, "outputs+1", 0, 1)


# ---------------------------------------------------------------------------------------------------------
# exact kernels
# ---------------------------------------------------------------------------------------------------------

def exact_vectors():
    """(name, fp32 vector): the sizes of EXACT_N and the special-value vector whole (4-wide route) and one short (a
    scalar tail of 3; for the casts the whole-array scalar fallback)."""
    out = [("n{}".format(n), (np.random.RandomState(27000 + n).randn(n) * 3).astype(f32)) for n in R.EXACT_N]
    return out + [("special24", R.special_values()), ("special23", R.special_values(23))]


VECTORS = exact_vectors()
IDS = [v[0] for v in VECTORS]
# which pointer is misaligned (4 bytes for fp32, 2 for bf16, 1 for a mask): forces the scalar route
RELU_OFFSETS = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1))


@pytest.mark.parametrize("vname,x", VECTORS, ids=IDS)
def test_relu_forward_f32(vname, x):
    sh, n = stream_handle(), len(x)
    wy, wm = R.relu_fwd(x)
    for xo, yo, mo in RELU_OFFSETS:
        for with_y, with_m in ((1, 1), (0, 1), (1, 0)):
            xd, y, m = dev(x, F32, xo), Guarded((n,), F32, yo), Guarded((n,), U8, mo)
            assert lib.dk_relu_fwd_f32(xd.data_ptr(), n, y.ptr if with_y else 0, m.ptr if with_m else 0, sh) == 0
            tag = "relu fwd {} off {} y {} mask {}".format(vname, (xo, yo, mo), with_y, with_m)
            if with_y:
                same(tag, y.raw(), wy)
            else:
                untouched(y)
            if with_m:
                assert np.array_equal(m.raw(), wm), tag
            else:
                untouched(m)


@pytest.mark.parametrize("vname,dyv", VECTORS, ids=IDS)
def test_relu_backward_f32(vname, dyv):
    sh, n = stream_handle(), len(dyv)
    mask = (np.random.RandomState(n).rand(n) < 0.5).astype(np.uint8) * np.uint8(1 + n % 3)
    want = R.relu_bwd(dyv, mask)
    for go, mo, xo in RELU_OFFSETS:
        g, m, dx = dev(dyv, F32, go), dev(mask, U8, mo), Guarded((n,), F32, xo)
        assert lib.dk_relu_bwd_f32(g.data_ptr(), m.data_ptr(), n, dx.ptr, sh) == 0
        same("relu bwd {} off {}".format(vname, (go, mo, xo)), dx.raw(), want)
    out = Guarded((n,), F32)
    assert lib.dk_mask_to_f32(dev(mask, U8).data_ptr(), n, out.ptr, sh) == 0
    same("mask_to_f32 {}".format(vname), out.raw(), R.mask_to_f32(mask))


@pytest.mark.parametrize("vname,x", VECTORS, ids=IDS)
def test_relu_bf16(vname, x):
    """bf16 storage: the widened value through the same contract; what is stored is bf16-representable."""
    sh, n = stream_handle(), len(x)
    xb = R.q16(x)
    wy, wm = R.relu_fwd(xb)
    mask = (np.random.RandomState(n + 1).rand(n) < 0.5).astype(np.uint8)
    wdx = R.relu_bwd(xb, mask)
    for xo, yo, mo in RELU_OFFSETS:
        xd, y, m = dev(xb, BF16, xo), Guarded((n,), BF16, yo), Guarded((n,), U8, mo)
        assert lib.dk_relu_fwd_bf16(xd.data_ptr(), n, y.ptr, m.ptr, sh) == 0
        assert R.same16(y.raw(), R.bits16(wy)), (vname, xo, yo, mo)
        assert np.array_equal(m.raw(), wm)
        md, dx = dev(mask, U8, mo), Guarded((n,), BF16, yo)
        assert lib.dk_relu_bwd_bf16(xd.data_ptr(), md.data_ptr(), n, dx.ptr, sh) == 0
        assert R.same16(dx.raw(), R.bits16(wdx)), (vname, xo, yo, mo)


def add_operands(vname, a):
    if vname.startswith("special"):
        return R.special_partner()[:len(a)]
    return (np.random.RandomState(len(a) + 7).randn(len(a)) * 3).astype(f32)


@pytest.mark.parametrize("vname,a", VECTORS, ids=IDS)
def test_add_f32(vname, a):
    sh, n = stream_handle(), len(a)
    b = add_operands(vname, a)
    for ao, bo, yo, mo in ((0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)):
        for relu, with_m in ((0, 0), (1, 1), (1, 0)):
            wy, wm = R.add(a, b, relu)
            ad, bd = dev(a, F32, ao), dev(b, F32, bo)
            y, m = Guarded((n,), F32, yo), Guarded((n,), U8, mo)
            assert lib.dk_add_f32(ad.data_ptr(), bd.data_ptr(), n, relu, y.ptr, m.ptr if with_m else 0, sh) == 0
            tag = "add {} off {} relu {} mask {}".format(vname, (ao, bo, yo, mo), relu, with_m)
            same(tag, y.raw(), wy)
            if with_m:
                assert np.array_equal(m.raw(), wm), tag
            else:
                untouched(m)


@pytest.mark.parametrize("vname,a", VECTORS, ids=IDS)
def test_add_bf16(vname, a):
    """The fp32 sum of the widened operands, rounded once; the mask from the fp32 sum."""
    sh, n = stream_handle(), len(a)
    a, b = R.q16(a), R.q16(add_operands(vname, a))
    for relu in (0, 1):
        v, wm = R.add(a, b, relu)
        ad, bd, y, m = dev(a, BF16), dev(b, BF16), Guarded((n,), BF16), Guarded((n,), U8)
        assert lib.dk_add_bf16(ad.data_ptr(), bd.data_ptr(), n, relu, y.ptr, m.ptr if relu else 0, sh) == 0
        assert R.same16(y.raw(), R.bits16(v)), "add bf16 {} relu {}".format(vname, relu)
        if relu:
            assert np.array_equal(m.raw(), wm)


@pytest.mark.parametrize("vname,x", VECTORS, ids=IDS)
def test_scale_f32(vname, x):
    sh, n = stream_handle(), len(x)
    for xo, yo in ((0, 0), (1, 0), (0, 1)):
        for s in R.SCALES:
            xd, y = dev(x, F32, xo), Guarded((n,), F32, yo)
            assert lib.dk_scale_f32(xd.data_ptr(), n, float(s), y.ptr, sh) == 0
            same("scale {} off {} s {}".format(vname, (xo, yo), s), y.raw(), R.scale(x, s))


@pytest.mark.parametrize("vname,x", VECTORS, ids=IDS)
def test_casts(vname, x):
    """n % 4 != 0 takes the scalar fallback for the whole array."""
    sh, n = stream_handle(), len(x)
    xd, y = dev(x), Guarded((n,), BF16)
    assert lib.dk_cast_f32_to_bf16(xd.data_ptr(), n, y.ptr, sh) == 0
    got = y.raw().view(np.uint16)
    want = R.bits16(x)
    assert R.same16(got, want), "cast to bf16 {}: {}".format(vname, np.flatnonzero(got != want)[:8])
    back = Guarded((n,), F32)
    assert lib.dk_cast_bf16_to_f32(y.ptr, n, back.ptr, sh) == 0
    assert np.array_equal(back.raw().view(np.uint32), R.widen16(got).view(np.uint32)), "cast to fp32 {}".format(vname)


@pytest.mark.parametrize("name", list(R.NCHW))
def test_nchw_to_nhwc(name):
    N, C, H, W, Cp, off = R.NCHW[name]
    x, sh = R.layout_input((N, C, H, W), list(R.NCHW).index(name)), stream_handle()
    y = Guarded((N, H, W, Cp), F32, 1 if off else 0)
    assert lib.dk_nchw_to_nhwc_f32(dev(x).data_ptr(), N, C, H, W, Cp, y.ptr, sh) == 0
    same("nchw_to_nhwc {}".format(name), y.raw(), R.nchw_to_nhwc(x, Cp))


@pytest.mark.parametrize("name", list(R.UNPAD))
def test_nhwc_unpad(name):
    P, Cp, C = R.UNPAD[name]
    x, sh = R.layout_input((P, Cp), 10 + list(R.UNPAD).index(name)), stream_handle()
    y = Guarded((P, C), F32)
    assert lib.dk_nhwc_unpad_f32(dev(x).data_ptr(), P, Cp, C, y.ptr, sh) == 0
    same("nhwc_unpad {}".format(name), y.raw(), R.nhwc_unpad(x, C))


def test_grid_stride_second_trip():
    """n = 16384 * 1024 + 1029: 257 float4 chunks past the capped grid and a tail of one (the only large case).  The
    references are formed on the device by torch (one IEEE add; v > 0 ? v : 0), the comparison is bitwise."""
    n, sh = R.GRID_STRIDE_N, stream_handle()
    g = torch.Generator(device="cuda").manual_seed(5)
    a = torch.randn(n, generator=g, device="cuda")
    b = torch.randn(n, generator=g, device="cuda")
    y, m = Guarded((n,), F32), Guarded((n,), U8)
    assert lib.dk_relu_fwd_f32(a.data_ptr(), n, y.ptr, m.ptr, sh) == 0
    torch.cuda.synchronize()
    lead = y.lead
    for buf in (y, m):
        ints = buf.buf.view(buf.itype)
        assert bool((ints[:lead] == buf.bits).all()) and bool((ints[lead + n:] == buf.bits).all())
    pos = a > 0
    assert torch.equal(y.buf[lead:lead + n].view(torch.int32), torch.where(pos, a, torch.zeros_like(a)).view(torch.int32))
    assert torch.equal(m.buf[lead:lead + n], pos.to(U8))
    del m
    y = Guarded((n,), F32)
    assert lib.dk_add_f32(a.data_ptr(), b.data_ptr(), n, 0, y.ptr, 0, sh) == 0
    torch.cuda.synchronize()
    ints = y.buf.view(y.itype)
    assert bool((ints[:lead] == y.bits).all()) and bool((ints[lead + n:] == y.bits).all())
    assert torch.equal(ints[lead:lead + n], (a + b).view(torch.int32))


# ---------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------

def test_join_refusals():
    """dk_add_bf16, dk_bn_add_f32 / _bf16: status 10001, the outputs untouched."""
    sh, n, C = stream_handle(), 64, 8
    rng = np.random.RandomState(3)
    a16, b16 = dev(rng.randn(n + 8), BF16), dev(rng.randn(n + 8), BF16)
    a32, b32 = dev(rng.randn(n + 8)), dev(rng.randn(n + 8))
    bn = [dev(v) for v in R.bn_params(C + 4, rng)]
    p = tuple(t.data_ptr() for t in bn)
    y16, y32, m = Guarded((n,), BF16), Guarded((n,), F32), Guarded((n,), U8)
    A, Bp = a16.data_ptr(), b16.data_ptr()
    for args in ((0, Bp, n, 1, y16.ptr, m.ptr), (A, 0, n, 1, y16.ptr, m.ptr), (A, Bp, n, 1, 0, m.ptr),
                 (A, Bp, 0, 1, y16.ptr, m.ptr), (A + 2, Bp, n, 1, y16.ptr, m.ptr), (A, Bp + 4, n, 1, y16.ptr, m.ptr),
                 (A, Bp, n, 1, y16.ptr + 2, m.ptr), (A, Bp, n, 1, y16.ptr, m.ptr + 1)):
        refused(ARGS, lib.dk_add_bf16, *args, sh)

    def bn_add(fn, a, b, y, esz, mptr=None, n_=n, C_=C, pa=(*p, 0), pb=(*p, 1)):
        refused(ARGS, fn, a, *pa, b, *pb, n_, C_, 1, y, m.ptr if mptr is None else mptr, sh)

    for fn, a, b, y, esz in ((lib.dk_bn_add_f32, a32.data_ptr(), b32.data_ptr(), y32.ptr, 4),
                             (lib.dk_bn_add_bf16, A, Bp, y16.ptr, 2)):
        bn_add(fn, a, b, y, esz, C_=2)                      # C < 4
        bn_add(fn, a, b, y, esz, C_=6, n_=60)               # C % 4
        bn_add(fn, a, b, y, esz, n_=n + 4)                  # n % C
        bn_add(fn, a, b, y, esz, n_=1 << 31)                # n >= 2^31
        bn_add(fn, a + esz, b, y, esz)                      # misaligned a, b, y, mask
        bn_add(fn, a, b + esz, y, esz)
        bn_add(fn, a, b, y + esz, esz)
        bn_add(fn, a, b, y, esz, mptr=m.ptr + 2)
        bn_add(fn, a, b, y, esz, pa=(p[0], 0, p[2], p[3], 0))      # a mean without its invstd
        bn_add(fn, a, b, y, esz, pb=(p[0] + 4, p[1], p[2], p[3], 0))   # a misaligned parameter vector
    for a, b, y, n_ in ((0, Bp, y16.ptr, n), (A, 0, y16.ptr, n), (A, Bp, 0, n), (A, Bp, y16.ptr, 0)):
        refused(ARGS, lib.dk_bn_add_bf16, a, *p, 0, b, *p, 0, n_, C, 1, y, m.ptr, sh)
    untouched(y16, y32, m)
    # the next call on the stream works
    assert lib.dk_add_bf16(A, Bp, n, 1, y16.ptr, m.ptr, sh) == 0
    v, wm = R.add(R.widen16(a16.cpu().view(torch.int16).numpy().view(np.uint16)[:n]),
                  R.widen16(b16.cpu().view(torch.int16).numpy().view(np.uint16)[:n]), 1)
    assert R.same16(y16.raw(), R.bits16(v)) and np.array_equal(m.raw(), wm)


def test_gap_refusals():
    sh = stream_handle()
    d = gap_in("g3")
    N, HW, C = d["N"], d["HW"], d["C"]
    x16, dy = dev(d["x"], BF16), dev(d["dy"])
    out, dx16, mask = Guarded((N, C), F32), Guarded((N, HW, C), BF16), Guarded((N, HW, C), U8)
    big = (1 << 16, 1 << 15, 1)     # N HW C = 2^31
    for x, shape, o in ((0, (N, HW, C), out.ptr), (x16.data_ptr(), (N, HW, C), 0), (x16.data_ptr(), (0, HW, C), out.ptr),
                        (x16.data_ptr(), (N, 0, C), out.ptr), (x16.data_ptr(), (N, HW, 0), out.ptr),
                        (x16.data_ptr(), big, out.ptr)):
        refused(ARGS, lib.dk_gap_fwd_bf16, x, *shape, o, sh)
    for g, shape, o in ((0, (N, HW, C), dx16.ptr), (dy.data_ptr(), (N, HW, C), 0), (dy.data_ptr(), (0, HW, C), dx16.ptr),
                        (dy.data_ptr(), (N, 0, C), dx16.ptr), (dy.data_ptr(), (N, HW, 0), dx16.ptr),
                        (dy.data_ptr(), big, dx16.ptr)):
        refused(ARGS, lib.dk_gap_bwd_bf16, g, *shape, o, sh)
    a, b = dev(d["a"]), dev(d["b"])
    p = tuple(t.data_ptr() for t in [dev(v) for v in d["pa"]])
    keep = (a, b)
    A, Bp = a.data_ptr(), b.data_ptr()
    for args in ((0, *p, 0, Bp, *ZERO5, N, HW, C), (A, *p, 0, 0, *ZERO5, N, HW, C), (A, *p, 0, Bp, *ZERO5, 0, HW, C),
                 (A, *p, 0, Bp, *ZERO5, N, 0, C), (A, *p, 0, Bp, *ZERO5, N, HW, 0), (A, *p, 0, Bp, *ZERO5, *big),
                 (A, p[0], 0, p[2], p[3], 0, Bp, *ZERO5, N, HW, C), (A, *ZERO5, Bp, p[0], p[1], 0, p[3], 1, N, HW, C),
                 (A, *ZERO5, Bp, p[0], p[1], p[2], 0, 1, N, HW, C)):
        refused(ARGS, lib.dk_gap_join_fwd_f32, *args, mask.ptr, out.ptr, sh)
    refused(ARGS, lib.dk_gap_join_fwd_f32, A, *p, 0, Bp, *ZERO5, N, HW, C, mask.ptr, 0, sh)
    untouched(out, dx16, mask)
    assert keep and lib.dk_gap_fwd_bf16(x16.data_ptr(), N, HW, C, out.ptr, sh) == 0
    r = R.gap_fwd(d["x"])
    R.check("gap fwd g3 after refusals", out.result(), r.ref, r.A)


def test_reduction_refusals():
    """dk_colsum_bf16 arguments; dk_l2_loss_multi_f32 arguments and workspace (the short workspaces of the column
    sums and of the dense weight gradient are refused in their own tests)."""
    sh = stream_handle()
    x = R.colsum_inputs("c4")
    M, N = x.shape
    xd, out = dev(x, BF16), Guarded((N,), F32)
    nb = lib.dk_colsum_workspace_bytes(M, N)
    for args in ((0, M, N, out.ptr), (xd.data_ptr(), M, N, 0), (xd.data_ptr(), 0, N, out.ptr), (xd.data_ptr(), M, 0, out.ptr)):
        refused(ARGS, lib.dk_colsum_bf16, *args, workspace.get(nb), nb, sh)
    refused(WORKSPACE, lib.dk_colsum_f32, dev(x).data_ptr(), M, N, out.ptr, workspace.get(nb), 0, sh)
    untouched(out)
    ws, strengths, wd, table, blocks = l2_table("t1")
    nb = lib.dk_l2_multi_workspace_bytes(blocks)
    out = Guarded((1,), F32)
    refused(ARGS, lib.dk_l2_loss_multi_f32, table.data_ptr(), 0, blocks, 0, out.ptr, workspace.get(nb), nb, sh)
    refused(ARGS, lib.dk_l2_loss_multi_f32, table.data_ptr(), -1, blocks, 0, out.ptr, workspace.get(nb), nb, sh)
    refused(ARGS, lib.dk_l2_loss_multi_f32, table.data_ptr(), len(ws), 0, 0, out.ptr, workspace.get(nb), nb, sh)
    refused(WORKSPACE, lib.dk_l2_loss_multi_f32, table.data_ptr(), len(ws), blocks, 0, out.ptr, workspace.get(nb), nb - 1,
            sh)
    untouched(out)
    assert lib.dk_l2_loss_multi_f32(table.data_ptr(), len(ws), blocks, 0, out.ptr, workspace.get(nb), nb, sh) == 0
    r = R.l2_multi(ws, strengths)
    R.check("l2 multi t1 after refusals", out.result(), r.ref, r.A)


def test_cast_refusals():
    """16-byte fp32 and 8-byte bf16 pointers (status 10001); n <= 0 is accepted and writes nothing."""
    sh, n = stream_handle(), 16
    x = dev(np.arange(n + 4, dtype=f32))
    xb = dev(np.arange(n + 4, dtype=f32), BF16)
    y16, y32 = Guarded((n,), BF16), Guarded((n,), F32)
    refused(ARGS, lib.dk_cast_f32_to_bf16, x.data_ptr() + 4, n, y16.ptr, sh)
    refused(ARGS, lib.dk_cast_f32_to_bf16, x.data_ptr(), n, y16.ptr + 2, sh)
    refused(ARGS, lib.dk_cast_f32_to_bf16, x.data_ptr(), n, y16.ptr + 4, sh)
    refused(ARGS, lib.dk_cast_bf16_to_f32, xb.data_ptr() + 2, n, y32.ptr, sh)
    refused(ARGS, lib.dk_cast_bf16_to_f32, xb.data_ptr() + 4, n, y32.ptr, sh)
    refused(ARGS, lib.dk_cast_bf16_to_f32, xb.data_ptr(), n, y32.ptr + 4, sh)
    assert lib.dk_cast_f32_to_bf16(x.data_ptr(), 0, y16.ptr, sh) == 0
    assert lib.dk_cast_bf16_to_f32(xb.data_ptr(), 0, y32.ptr, sh) == 0
    untouched(y16, y32)
    assert lib.dk_cast_f32_to_bf16(x.data_ptr(), n, y16.ptr, sh) == 0
    assert np.array_equal(y16.raw().view(np.uint16), R.bits16(np.arange(n, dtype=f32)))
