"""tests/_head_ref.py on the CPU: the fp64 references agree with the oracle, their per-element bounds admit an honest
implementation -- a numpy transcription of every kernel of the head in the kernel's own operation order (fp32 where
the kernel is fp32, fp64 sums where it widens, bf16 stores rounded to nearest even), each sum taken under two groupings
(the kernel's own: quad lanes and exchanges, 64 lanes and the wave tree, eight-at-a-time loads, row chunks, 256 strided
threads and their tree, k-tiles and split-K slabs; and another: reversed, pairwise or whole) -- on every case of the
tables, and they reject defective ones, each a mutation of that transcription of a kind such a kernel can have.  It
also asserts the element cap of the case tables and the ReLU margins of the pooled join.

Defects, the case, the check that must fail with its worst err / bound, and what the suite's normwise checks
(tests/test_gpu_layers.py: 1e-4 on a tensor, 1e-5 max(1, |loss|) on the loss) see of the same output:

    softmax sum without the second quad exchange    s2   P            2.1e5    0.96
    K % 4 tail columns dropped                      s10  P            1.3e5    0.14
    K = 129 taken on the quad path                  s13  P            1.2e5    1.2e-2
    rows past the first 256 dropped from the loss   s9   loss         3.3e3    2.1e-3
    loss divided by 256 instead of B = 257          s9   loss         6.2e3    3.9e-3
    pooling divides by 8 (HW // 8), HW = 9          g4   out          1.7e5    0.13
    pooling backward: n from HW C, not HW C / 4     g3   dx           inf      0.86    (HW = 8: the bound is 0)
    column sums accumulated in fp32                 c5   out          6.1e4    6.7e-4
                                                    c7   out          11       5.5e-4
    column-sum chunk one row short                  c5   out          1.5e10   1.6e2
    l2 multi without the chunk tails                t1   out          4.1e5    2.4e-2
    l2 multi: a block given to the previous tensor  t1   out          7.6e6    0.45
    dense bias skipped on the last column tile      d3   y            3.2e4    0.10
    dense l2 term with w transposed                 d3   dw           2.9      2.2e-5
    truncating bf16 store                           g7   dx, bf16     43       3.2e-3
    truncating bf16 cast                                 bits differ at the ties, above them, at overflow

What the normwise checks let through, asserted below: the transposed l2 term (l2 w is 1e-3 of a weight against
gradients of order one: 2.2e-5 of the tensor's norm).  Every other defect is above 1e-4 at these cases -- the fp32
column sums only through the ill-conditioned column, which no layer test has (on well-conditioned columns fp32
accumulation over 286 rows is of the order of 1e-6), and the lost rows and the wrong divisor of the loss only
because B = 257 is small: both are a relative 1 / B and fall under 1e-5 from B = 10^5 on, while the per-element bound
does not grow with B.  The layer tests had no case at all for K = 129, K < 4, a wave's second row, HW < 8 or HW = 8,
soft labels, misaligned operands, accumulate = 1, the multi-tensor l2 on its own or special values.
"""
import functools

import numpy as np
import pytest

from oracle import ref as oref
from tests import _head_ref as R
from tests._convert import rel_err
from tests._dw_ref import bf16_bound, worst

f32, f64 = np.float32, np.float64
GROUPINGS = ("kernel", "other")
OLD_TOL = 1e-4          # the normwise tolerance of tests/test_gpu_layers.py
OLD_LOSS_TOL = 1e-5     # its tolerance on the loss, relative to max(1, |loss|)


def ratio(got, r, bound=None):
    return worst(np.asarray(got, dtype=f64), r.ref, r.A if bound is None else bound)[0]


def seq(a, axis, dtype):
    """Sequential sum along an axis in `dtype` (0 for an empty axis)."""
    a = np.asarray(a, dtype=dtype)
    if a.shape[axis] == 0:
        return np.zeros(np.delete(a.shape, axis).astype(int), dtype=dtype)
    return np.take(np.cumsum(a, axis=axis, dtype=dtype), -1, axis=axis)


def tree(r):
    """The 256-leaf (or 64-lane) halving tree over axis 0: r[t] += r[t + o], o = n / 2 .. 1."""
    r = np.array(r)
    o = r.shape[0] // 2
    while o:
        r[:o] = r[:o] + r[o:2 * o]
        o >>= 1
    return r[0]


def trunc16(a):
    return (np.ascontiguousarray(a, dtype=f32).view(np.uint32) & np.uint32(0xFFFF0000)).view(f32)


# ---------------------------------------------------------------------------------------------------------
# softmax with cross-entropy (elementwise.hip:262-375)
# ---------------------------------------------------------------------------------------------------------

def expf(x):
    return np.exp(np.asarray(x, dtype=f64)).astype(f32)     # correctly rounded: within the assumed one ulp


def logf(x):
    return np.log(np.asarray(x, dtype=f64)).astype(f32)


def lane_columns(K, quad, v4, lane):
    if not quad:
        return list(range(lane, K, 64))
    if v4:
        return [4 * (lane + 4 * i) + u for i in range(8) for u in range(4) if 4 * (lane + 4 * i) + u < K]
    return [lane + 4 * j for j in range(32) if lane + 4 * j < K]


def combine(lanes, quad, defect):
    """[B][lanes] lane values -> the value each lane holds after the exchanges."""
    if not quad:
        t = tree(lanes.T.copy())
        return np.repeat(t[:, None], lanes.shape[1], axis=1)
    s01, s23 = lanes[:, 0] + lanes[:, 1], lanes[:, 2] + lanes[:, 3]
    if defect == "no_exchange":
        return np.stack([s01, s01, s23, s23], axis=1)
    return np.repeat((s01 + s23)[:, None], 4, axis=1)


def h_softmax(x, y, grouping, v4=None, defect=None):
    """(P, loss): fp32, the kernel's order.  v4: the float4 column assignment (default: K % 4 == 0)."""
    B, K = x.shape
    v4 = K % 4 == 0 if v4 is None else v4
    quad = K <= 128 or defect == "k129_quad"
    e = expf(x)
    P = np.zeros((B, K), dtype=f32)     # a column the defective kernel never writes reads as 0 here
    nl = 4 if quad else 64
    cols = [lane_columns(K, quad, v4 and quad, l) for l in range(nl)]
    if defect == "drop_tail":
        cols = [[c for c in cl if c < 4 * (K // 4)] for cl in cols]
    if grouping == "kernel":
        s = combine(np.stack([seq(e[:, cl], 1, f32) for cl in cols], axis=1), quad, defect)
    else:
        live = sorted(c for cl in cols for c in cl)
        s = np.repeat(seq(e[:, live[::-1]], 1, f32)[:, None], nl, axis=1)
    inv = f32(1) / s
    dots = np.zeros((B, nl), dtype=f32)
    for l, cl in enumerate(cols):
        P[:, cl] = inv[:, l:l + 1] * e[:, cl]
        if y is not None:
            dots[:, l] = seq(P[:, cl] * y[:, cl], 1, f32)
    if y is None:
        return P, None
    dot = combine(dots, quad, None)[:, 0] if grouping == "kernel" else seq(dots[:, ::-1], 1, f32)
    with np.errstate(divide="ignore"):
        rl = -logf(dot).astype(f64)
    rows = rl[:256] if defect == "loss_first256" else rl
    t = sum(rows[b0:b0 + 256].sum() for b0 in range(0, len(rows), 256))
    return P, f32((1.0 / (256 if defect == "loss_div256" else B)) * t)


@pytest.mark.parametrize("grouping", GROUPINGS)
@pytest.mark.parametrize("name", list(R.SOFTMAX))
def test_softmax_honest(name, grouping):
    c = R.SOFTMAX[name]
    x, y = R.softmax_inputs(name)
    r = R.softmax(x, y)
    P, loss = h_softmax(x, y, grouping, v4=c.K % 4 == 0 and c.offset is None)
    assert ratio(P, r) <= 1
    if y is not None:
        assert worst(np.array([loss], dtype=f64), r.loss, r.eloss)[0] <= 1
        dx = (f32(1) / f32(c.B)) * (P - y)
        rb = R.softmax_bwd(P, y)
        assert ratio(dx, rb) <= 1
        lo, Po = oref.softmax_xent_forward(x.astype(f64), y.astype(f64))
        np.testing.assert_allclose(r.ref, Po, rtol=1e-13)
        np.testing.assert_allclose(r.loss[0], lo, rtol=1e-13)
        np.testing.assert_allclose(rb.ref, oref.softmax_xent_backward(P.astype(f64), y.astype(f64)), rtol=1e-13, atol=0)
        if c.labels == "mixup" and c.K > 1:
            assert ((y > 0).sum(axis=1) == 2).all() and (y.astype(f64).sum(axis=1) == 1).all()


# ---------------------------------------------------------------------------------------------------------
# pooling (elementwise.hip:176-258)
# ---------------------------------------------------------------------------------------------------------

def h_gap_fwd(x, grouping, defect=None):
    x = np.asarray(x, dtype=f32)
    HW = x.shape[1]
    if grouping == "kernel":
        s = seq(x, 1, f32)
    else:   # eights summed on their own, the eights then added from the last to the first
        parts = np.stack([seq(x[:, k:k + 8], 1, f32) for k in range(0, HW, 8)], axis=1)
        s = seq(parts[:, ::-1], 1, f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return s / f32(8 * (HW // 8) if defect == "div8" else HW)


def h_gap_bwd(dy, HW, form="kernel", defect=None):
    dy = np.asarray(dy, dtype=f32)
    N, C = dy.shape
    if C % 4 == 0:      # gap_bwd4_kernel: float4 index i
        C4 = C // 4
        i = np.arange(N * HW * C4)
        n = i // (HW * C if defect == "n_index" else HW * C4)
        g = dy.reshape(N, C4, 4)[n, i % C4].reshape(N, HW, C)
    else:
        i = np.arange(N * HW * C)
        g = dy[i // (HW * C), i % C].reshape(N, HW, C)
    if form == "kernel":
        return (f32(1) / f32(HW)) * g
    return g / f32(HW)      # one correctly rounded division: also within two roundings


def h_join(d, a_relu, b_relu):
    def bn(x, p, relu):
        if relu is None:
            return np.asarray(x, dtype=f32)
        m, i, g, b = (np.asarray(v, dtype=f32)[None, None, :] for v in p)
        r = g * ((np.asarray(x, dtype=f32) - m) * i) + b
        return np.where(r > 0, r, f32(0)) if relu else r
    v = bn(d["a"], d["pa"], a_relu) + bn(d["b"], d["pb"], b_relu)
    return np.where(v > 0, v, f32(0)), (v > 0).astype(np.uint8)


@pytest.mark.parametrize("name", list(R.GAP))
def test_gap_honest(name):
    d = R.gap_inputs(name)
    N, HW, C = R.GAP[name]
    r = R.gap_fwd(d["x"])
    for grouping in GROUPINGS:
        assert ratio(h_gap_fwd(d["x"], grouping), r) <= 1
    np.testing.assert_allclose(r.ref, oref.gap_forward(d["x"].transpose(0, 2, 1)[..., None]), rtol=1e-13, atol=1e-16)
    rb = R.gap_bwd(d["dy"], HW)
    want = oref.gap_backward(d["dy"], (HW, 1))[..., 0].transpose(0, 2, 1)
    np.testing.assert_allclose(rb.ref, want, rtol=1e-13)
    for form in ("kernel", "division"):
        dx = h_gap_bwd(d["dy"], HW, form)
        assert ratio(dx, rb) <= 1
        assert ratio(R.q16(dx), rb, rb.b16) <= 1
    if HW & (HW - 1) == 0:
        assert not rb.A.any() and np.array_equal(h_gap_bwd(d["dy"], HW).astype(f64), rb.ref)


@pytest.mark.parametrize("variant", R.JOIN_VARIANTS)
@pytest.mark.parametrize("name", R.GAP_JOIN)
def test_gap_join_honest_and_margin(name, variant):
    d = R.gap_inputs(name)
    r = R.gap_join(d, *variant)
    assert r.margin > 1
    assert min(np.abs(d["pa"][3]).min(), np.abs(d["pb"][3]).min()) > 0
    y, mask = h_join(d, *variant)
    assert np.array_equal(mask, r.mask)
    for grouping in GROUPINGS:
        assert ratio(h_gap_fwd(y, grouping), r) <= 1


# ---------------------------------------------------------------------------------------------------------
# column sums and l2 (elementwise.hip: the colsum kernels, l2_loss_kernel; multi_tensor.hip: the l2 multi pair)
# ---------------------------------------------------------------------------------------------------------

def h_colsum(x, grouping, defect=None):
    x = np.asarray(x, dtype=f32)
    M, N = x.shape
    acc = f32 if defect == "fp32_acc" else f64
    if grouping == "other" and defect is None:
        return x.astype(f64)[::-1].sum(axis=0).astype(f32)
    chunks = R.colsum_chunks(M)
    rpc = R.cdiv(M, chunks)
    parts = []
    for k in range(chunks):
        r0 = k * rpc
        r1 = min(M, r0 + rpc - (1 if defect == "chunk_off" else 0))
        parts.append(seq(x[r0:max(r1, r0)], 0, acc))
    return seq(np.stack(parts), 0, acc).astype(f32)


@pytest.mark.parametrize("name", list(R.COLSUM))
def test_colsum_honest(name):
    x = R.colsum_inputs(name)
    M, N = R.COLSUM[name]
    r = R.colsum(x)
    for grouping in GROUPINGS:
        assert ratio(h_colsum(x, grouping), r) <= 1
    assert np.array_equal(x, R.q16(x).astype(f64))
    if M >= 7:
        assert np.abs(x[:, 0]).sum() > 1e6 * abs(r.ref[0]) > 0
    np.testing.assert_allclose(r.ref, oref.dense_backward(x, np.zeros((M, 1)), np.zeros((1, N)), True)[2], atol=1e-8)
    if name == "c7":
        assert (R.colsum_chunks(M), R.cdiv(M, R.colsum_chunks(M))) == (512, 65)


def strided256(terms):
    """Thread t adds terms t, t + 256, ... in order; then the tree."""
    pad = np.zeros(R.cdiv(max(len(terms), 1), 256) * 256)
    pad[:len(terms)] = terms
    return tree(seq(pad.reshape(-1, 256), 0, f64))


def h_l2(w, strength, grouping, prior=None):
    w = np.asarray(w, dtype=f64)
    s = strided256(w * w) if grouping == "kernel" else (w * w)[::-1].sum()
    v = f32(0.5 * float(strength) * s)
    return v if prior is None else f32(prior) + v


def h_l2_multi(ws, strengths, add_to, grouping, defect=None):
    sizes = [len(w) for w in ws]
    b0, total = R.l2_blocks(sizes)
    part = np.zeros(total)
    for b in range(total):
        t = 0
        while t + 1 < len(ws) and (b0[t + 1] < b if defect == "prev_tensor" else b0[t + 1] <= b):
            t += 1
        i0 = (b - b0[t]) * R.L2_CHUNK
        end = (sizes[t] // 256) * 256 if defect == "miss_tail" else sizes[t]
        w = np.asarray(ws[t][i0:max(min(i0 + R.L2_CHUNK, end), i0)], dtype=f64)
        part[b] = 0.5 * float(strengths[t]) * (strided256(w * w) if grouping == "kernel" else (w * w).sum())
    s = strided256(part) if grouping == "kernel" else part[::-1].sum()
    return f32((0.0 if add_to is None else float(add_to)) + s)


@pytest.mark.parametrize("grouping", GROUPINGS)
def test_l2_honest(grouping):
    for n in R.L2_N:
        w = R.l2_weights(n, n)
        for prior in (None, R.L2_PRIOR):
            r = R.l2(w, R.L2, prior)
            assert worst(np.array([h_l2(w, R.L2, grouping, prior)], dtype=f64), r.ref, r.A)[0] <= 1
        np.testing.assert_allclose(R.l2(w, R.L2).ref[0], oref.l2_forward(w.astype(f64), R.L2), rtol=1e-13)
    for name in R.L2_TABLES:
        ws, strengths = R.l2_table_inputs(name)
        assert len(set(strengths)) == len(strengths) and (name != "t1" or 0.0 in strengths)
        for add_to in (None, float(f32(R.L2_ADD_TO))):
            r = R.l2_multi(ws, strengths, add_to)
            assert worst(np.array([h_l2_multi(ws, strengths, add_to, grouping)], dtype=f64), r.ref, r.A)[0] <= 1
            want = (add_to or 0.0) + sum(oref.l2_forward(w.astype(f64), s) for w, s in zip(ws, strengths))
            np.testing.assert_allclose(r.ref[0], want, rtol=1e-13)
    assert R.l2_blocks(R.L2_TABLES["t1"][0]) == ([0, 1, 2, 3, 5], 8)
    assert R.l2_blocks(R.L2_TABLES["t2"][0])[1] > 256
    raw = R.l2_table_bytes([16, 32], [5, 3000], [0.5, 0.25])
    assert len(raw) == 64 and raw[32:40] == (32).to_bytes(8, "little") and raw[48:56] == (1).to_bytes(8, "little")


# ---------------------------------------------------------------------------------------------------------
# dense (gemm_dense.hip)
# ---------------------------------------------------------------------------------------------------------

def slabs(a, b, step, grouping):
    """a @ b in fp32, the reduction in slabs of `step` added in order (kernel) or whole (other)."""
    a, b = np.asarray(a, dtype=f32), np.asarray(b, dtype=f32)
    if grouping == "other":
        return a @ b
    acc = np.zeros((a.shape[0], b.shape[1]), dtype=f32)
    for k in range(0, a.shape[1], step):
        acc = acc + a[:, k:k + step] @ b[k:k + step]
    return acc


def h_dense_fwd(d, bias, grouping, defect=None):
    y = slabs(d["x"], d["w"], 16 if d["IN"] <= 128 else 32, grouping)
    if bias:
        b = d["bias"].copy()
        if defect == "bias_last_tile":
            b[64 * ((d["OUT"] - 1) // 64):] = 0
        y = y + b[None, :]
    return y


def h_dense_wgrad(d, l2, grouping, defect=None):
    dw = slabs(np.asarray(d["x"], dtype=f32).T, d["dy"], 32, grouping)
    w = d["w"].T.reshape(d["w"].shape) if defect == "l2_transposed" else d["w"]
    return dw + f32(l2) * w if l2 else dw


@pytest.mark.parametrize("grouping", GROUPINGS)
@pytest.mark.parametrize("name", list(R.DENSE))
def test_dense_honest(name, grouping):
    d = R.dense_inputs(name)
    w64 = d["w"].astype(f64)
    for bias in (False, True):
        r = R.dense_fwd(d, bias)
        assert ratio(h_dense_fwd(d, bias, grouping), r) <= 1
        np.testing.assert_allclose(r.ref, oref.dense_forward(d["x"], w64, d["bias"].astype(f64) if bias else None),
                                   rtol=1e-12, atol=1e-14)
    r = R.dense_dgrad(d)
    assert ratio(slabs(d["dy"], d["w"].T, 16 if d["OUT"] <= 128 else 32, grouping), r) <= 1
    for l2 in (0.0, R.L2):
        rw = R.dense_wgrad(d, l2)
        assert ratio(h_dense_wgrad(d, l2, grouping), rw) <= 1
        dx, dw, _ = oref.dense_backward(d["dy"], d["x"], w64, False, l2)
        np.testing.assert_allclose(rw.ref, dw, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(r.ref, dx, rtol=1e-12, atol=1e-14)


def test_dense_case_rules():
    """The routes the DENSE comments name, from the rules of gemm_engine.h quoted in tests/_head_ref.py."""
    def vec(*dims):
        return all(v % 4 == 0 for v in dims)
    got = {k: (vec(IN, OUT), 6 if IN <= 128 else 8, 6 if OUT <= 128 else 8, R.dense_wgrad_config(IN, OUT),
               min(R.cdiv(1024, R.cdiv(IN, 64) * R.cdiv(OUT, 128 if R.dense_wgrad_config(IN, OUT) == 6 else 64)),
                   R.cdiv(B, 32)))
           for k, (B, IN, OUT) in R.DENSE.items()}
    assert got == {"d1": (True, 6, 6, 1, 1), "d2": (False, 6, 6, 1, 1), "d3": (True, 6, 8, 6, 3),
                   "d4": (False, 6, 8, 6, 3), "d5": (True, 8, 6, 1, 3), "d6": (False, 8, 6, 1, 2)}


# ---------------------------------------------------------------------------------------------------------
# exact kernels
# ---------------------------------------------------------------------------------------------------------

def rne_bits(x):
    """fp32 -> bf16 bits by integer arithmetic: add 0x7FFF + the kept lsb, shift; a NaN keeps its top bits, quieted."""
    b = np.ascontiguousarray(x, dtype=f32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), ((b >> 16) | 0x40).astype(np.uint16), r)


def test_exact_references():
    v, p = R.special_values(), R.special_partner()
    assert len(v) == len(p) == 24 and len(R.special_values(23)) == 23
    y, m = R.relu_fwd(v)
    bits = y.view(np.uint32)
    assert bits[1] == 0 and bits[11] == 0 and bits[10] == 0 and m[10] == 0      # -0 -> +0; NaN -> 0, mask 0
    assert bits[2] == 1 and m[2] == 1 and bits[3] == 0 and m[3] == 0            # a positive subnormal passes
    s, _ = R.add(v, p, 0)
    assert s.view(np.uint32)[0] == 0 and s.view(np.uint32)[2] == 2 and np.isnan(s[8]) and np.isnan(s[10])
    assert R.scale(v, f32(0.5)).view(np.uint32)[2] == 0 and R.scale(v, f32(0.5)).view(np.uint32)[4] == 0x00400000
    rnd = (np.random.RandomState(1).randn(4096) * 3).astype(f32)
    for a in (v, p, rnd, R.scale(rnd, f32(1e-38))):
        assert R.same16(R.bits16(a), rne_bits(a))
        assert R.same_bits(R.widen16(R.bits16(a)), R.q16(a))
    assert np.isnan(R.widen16(R.bits16(v)[10:12])).all() and not R.same16(R.bits16(v)[:12], R.bits16(v)[:10])
    assert list(R.bits16(v)[12:18]) == [0x3F80, 0x3F82, 0xBF80, 0xBF82, 0x3F81, 0x3F80]
    assert list(R.bits16(v)[18:22]) == [0x7F80, 0xFF80, 0x0000, 0x0002]
    assert R.same_bits(v, v) and not R.same_bits(y, v)
    x = R.layout_input((2, 3, 5, 7), 0)
    y = R.nchw_to_nhwc(x, 4)
    assert y.shape == (2, 5, 7, 4) and y[1, 2, 3, 1] == x[1, 1, 2, 3] and not y[..., 3].any()
    assert np.array_equal(R.nhwc_unpad(y.reshape(-1, 4), 3).reshape(2, 5, 7, 3), x.transpose(0, 2, 3, 1))
    assert np.array_equal(R.mask_to_f32(np.array([0, 1, 7, 255], dtype=np.uint8)), np.array([0, 1, 1, 1], dtype=f32))
    assert np.array_equal(R.relu_bwd(v[:4], [0, 2, 0, 1]).view(np.uint32), [0, v.view(np.uint32)[1], 0, 0x80000001])


def test_case_tables():
    sizes = R.case_tensor_sizes()
    assert max(sizes.values()) <= R.MAX_ELEMENTS, max(sizes, key=sizes.get)
    assert R.GRID_STRIDE_N == 16384 * 1024 + 1029 and (R.GRID_STRIDE_N // 4) > 16384 * 256 and R.GRID_STRIDE_N % 4 == 1
    assert {hw for _, hw, _ in R.GAP.values()} >= {1, 7, 8, 9, 49, 64, 81}
    assert {c for _, _, c in R.GAP.values()} >= {1, 3, 6, 20, 512}
    assert any(n * c == 257 for n, _, c in R.GAP.values())
    assert all(R.GAP[k][2] % 4 == 0 for k in R.GAP_MISALIGNED)
    assert set(R.COLSUM.values()) >= {(1, 1), (7, 3), (64, 5), (65, 4), (286, 24), (130, 257), (33000, 3)}
    assert {(c.B, c.K) for c in R.SOFTMAX.values()} >= {(1, 4), (6, 120), (256, 128), (257, 8), (513, 12), (3, 1), (5, 3),
                                                         (257, 10), (300, 127), (3, 129), (17, 130), (2, 1000)}
    x, _ = R.softmax_inputs("s5")
    p = R.softmax(x).ref
    assert np.abs(x).max() <= 30 and p.min() > 2.0 ** -126 and p.max() / p.min() > 1e24
    assert R.L2 == float(f32(1e-3)) and R.EXPF == R.LOGF == 2 * R.U


# ---------------------------------------------------------------------------------------------------------
# seeded defects
# ---------------------------------------------------------------------------------------------------------

def softmax_defect(name, defect):
    """(worst ratio on P, on the loss; normwise error of P, relative error of the loss)."""
    x, y = R.softmax_inputs(name)
    r = R.softmax(x, y)
    P, loss = h_softmax(x, y, "kernel", defect=defect, v4=False if defect == "k129_quad" else None)
    return (ratio(P, r), worst(np.array([loss], dtype=f64), r.loss, r.eloss)[0], rel_err(P, r.ref),
            abs(float(loss) - r.loss[0]) / max(1.0, abs(r.loss[0])))


@functools.lru_cache(maxsize=None)
def defects():
    """{defect: (the per-element ratio that must exceed 1, what the old normwise check sees, its tolerance)}."""
    out = {}
    for name, defect in (("s2", "no_exchange"), ("s10", "drop_tail"), ("s13", "k129_quad")):
        rp, _, nw, _ = softmax_defect(name, defect)
        out[defect] = (rp, nw, OLD_TOL)
    for defect in ("loss_first256", "loss_div256"):
        _, rl, _, lw = softmax_defect("s9", defect)
        out[defect] = (rl, lw, OLD_LOSS_TOL)
    d = R.gap_inputs("g4")
    r = R.gap_fwd(d["x"])
    got = h_gap_fwd(d["x"], "kernel", "div8")
    out["gap_div8"] = (ratio(got, r), rel_err(got, r.ref), OLD_TOL)
    d = R.gap_inputs("g3")
    r = R.gap_bwd(d["dy"], d["HW"])
    got = h_gap_bwd(d["dy"], d["HW"], defect="n_index")
    out["gap_bwd_n_index"] = (ratio(got, r), rel_err(got, r.ref), OLD_TOL)
    for case in ("c5", "c7"):
        x = R.colsum_inputs(case)
        r = R.colsum(x)
        got = h_colsum(x, "kernel", "fp32_acc")
        out["colsum_fp32_acc_" + case] = (ratio(got, r), rel_err(got, r.ref), OLD_TOL)
    x = R.colsum_inputs("c5")
    r = R.colsum(x)
    got = h_colsum(x, "kernel", "chunk_off")
    out["colsum_chunk_off"] = (ratio(got, r), rel_err(got, r.ref), OLD_TOL)
    ws, st = R.l2_table_inputs("t1")
    r = R.l2_multi(ws, st)
    for defect in ("miss_tail", "prev_tensor"):
        got = np.array([h_l2_multi(ws, st, None, "kernel", defect)], dtype=f64)
        out["l2_" + defect] = (worst(got, r.ref, r.A)[0], rel_err(got, r.ref), OLD_TOL)
    d = R.dense_inputs("d3")
    r = R.dense_fwd(d, True)
    got = h_dense_fwd(d, True, "kernel", "bias_last_tile")
    out["dense_bias_last_tile"] = (ratio(got, r), rel_err(got, r.ref), OLD_TOL)
    r = R.dense_wgrad(d, R.L2)
    got = h_dense_wgrad(d, R.L2, "kernel", "l2_transposed")
    out["dense_l2_transposed"] = (ratio(got, r), rel_err(got, r.ref), OLD_TOL)
    d = R.gap_inputs("g7")
    r = R.gap_bwd(d["dy"], d["HW"])
    got = trunc16(h_gap_bwd(d["dy"], d["HW"]))
    out["bf16_truncating_store"] = (ratio(got, r, r.b16), rel_err(got, r.ref), OLD_TOL)
    return out


DEFECTS = ("no_exchange", "drop_tail", "k129_quad", "loss_first256", "loss_div256", "gap_div8", "gap_bwd_n_index",
           "colsum_fp32_acc_c5", "colsum_fp32_acc_c7", "colsum_chunk_off", "l2_miss_tail", "l2_prev_tensor",
           "dense_bias_last_tile", "dense_l2_transposed", "bf16_truncating_store")
# what the suite's normwise check lets through (module docstring): recorded, asserted below
PASSES_NORMWISE = ("dense_l2_transposed",)


@pytest.mark.parametrize("defect", DEFECTS)
def test_defect_fails(defect):
    r, _, _ = defects()[defect]
    assert r > 1, (defect, r)


def test_truncating_cast_differs():
    v = R.special_values()
    got = (v.view(np.uint32) >> 16).astype(np.uint16)
    assert not np.array_equal(got, R.bits16(v))
    assert set(np.flatnonzero(got != R.bits16(v))) >= {13, 15, 16, 18, 19}     # ties up, above a tie, overflow to inf


def test_what_normwise_lets_through():
    assert set(defects()) == set(DEFECTS)
    through = tuple(k for k in DEFECTS if defects()[k][1] <= defects()[k][2])
    for k in DEFECTS:
        print("{:28s} err / bound {:10.3g}   normwise {:.3g}".format(k, *defects()[k][:2]))
    assert through == PASSES_NORMWISE
