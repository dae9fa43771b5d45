"""tests/_conv_ref.py on the CPU: the fp64 reference agrees with the oracle's dense convolution, its dgrad and
wgrad are the adjoints of its forward, its per-element bounds admit an honest fp32 implementation in another
summation order (numpy fp32: bn_operand_f32, an im2col patch matrix with columns (c, r, s), one matmul, the
scatter-add of the reference for dx; fp64 sums of the fp32 y for the statistics), and they reject the defects they
exist for -- each a mutation of that implementation of a kind a convolution kernel can have.

The bf16 mode of the reference gets the same: an honest bf16 implementation (weights and any operand formed on load
rounded to bf16, exact products, fp32 accumulation one product at a time and in 32-deep k-tiles, one
round-to-nearest-even store of y and dx, dw kept in fp32) is admitted at every case, none excluded, and mutations of it
are rejected; what the derived bounds cannot reject is asserted as such (test_mutations_the_bf16_bounds_cannot_reject).

Worst err / bound of the honest implementation over the 34 cases (recorded with DORKNET_SLACK_LOG; results, not
tolerances):

    forward y, engine n   0.128     forward y, narrow n    0.106     statistics | stored  sum 0, squares 0.194
    dgrad dx, gemm        0.011     phase  0.128           sub-pixel  0.299    | reference  0.015, 0.021
    dw  plain / BatchNorm on load   0.476 / 0.476          dy formed on load (dense / lattice)   0.476 / 0.033
    (the 0.476 is the single-split case e10 with l2: 2 u |ref| is most of its bound)

Defects, worst err / bound (each must exceed 1):
    one tap dropped at one border pixel (e1)                       2.1e4
    the padding normalised, bn(0) instead of 0 (e1)                4.5e4
    one input row taken from the neighbouring image (n4)           5.0e4
      the same at every image boundary of the multi-row case nm1   42.7 -- the M-term of the dw bound grows with
      M^2 (M dwa), so at nm1's M = 4340 a single wrong row (2 pixels of 4340) can stay below it; a wrong ring slot
      at every image boundary does not.  This is why nm1 and nm2 keep OW = 2.
    one (c, r, s) column of dw missing one output row (n4)         2.2e4
    the padded channel leaking into dw (e4, BatchNorm on load)     6.6e2
    the statistics missing one row / counting it twice (e1)        1.8e11 of the sums-of-the-stored-outputs bound

The honest bf16 implementation, both accumulation orders (a bf16 store attains the interval form's end by
construction: 1.000 is at the bound; the closed form's figure in brackets):

    forward y    1.000 (0.994)       statistics | stored  sum 0, squares 0.0005     | reference  0.999, 0.994
    dgrad dx, gemm  1.000 (0.967)    phase  1.000 (0.975)
    dw  plain / BatchNorm on load   0.476 / 0.816   (the latter against the summed 2^-8 slack of the rounded operand)

bf16 defects, worst err / bound (each must exceed 1):
    the store truncating instead of rounding to nearest (e1)       1.3e4 of the interval form; 1.92 of the closed form
    one tap dropped at one border pixel (e1)                       9.6e3
    the padding normalised, rne_bf16(bn(0)) instead of 0 (e1)      98.6
    dw missing the first of its nine split-K slabs (e1)            3.2e3
    the padded channel leaking into dw (e4, BatchNorm on load)     5.28 (the rounded operand's slack is most of the bound)
    statistics of the fp32 accumulator, not of the stored y (e1)   9.5e9 (sum), 1.8e10 (squares) of the
      sums-of-the-stored-outputs bound; the check against the reference admits them
    a statistics row missing / counted twice (e1)                  rejected by the same check
Not rejected (facts about the bounds): a bn(x) operand truncated to bf16 (1.000); truncated weights behind a
BatchNorm on load are all but hidden (1.19), though rejected on raw bf16 x (2.7e4); no dw bound sees the weights'
rounding.
"""
import numpy as np
import pytest
import torch

from oracle import ref as oref
from tests import _conv_ref as R
from tests._dw_ref import bn_operand_f32

f = np.float32
NAMES = R.ORDER


# ---------------------------------------------------------------------------------------------------------
# the honest implementation
# ---------------------------------------------------------------------------------------------------------

def patches(a, c):
    """(N, OH, OW, C, R, S) fp32 view of the zero-padded operand."""
    OH, OW = R.case_hw(c)
    p = oref.im2col(oref.pad_input(np.asarray(a, dtype=f), c.pad), c.R, c.S, c.stride, OH, OW)
    assert p.dtype == f
    return p.reshape(a.shape[0], OH, OW, a.shape[1], c.R, c.S)


def h_operand(d, bn):
    return bn_operand_f32(d["x"], R.pi_of(d, bn))


def h_forward(d, bias=False, bn=None, p=None):
    c = d["case"]
    p = patches(h_operand(d, bn), c) if p is None else p
    y = p.reshape(d["M"], -1) @ d["w"].reshape(c.K, -1).T
    if bias:
        y = y + d["bias"]
    assert y.dtype == f
    return y.reshape(c.N, d["OH"], d["OW"], c.K).transpose(0, 3, 1, 2)


def h_dgrad(d):
    c = d["case"]
    rows = d["dy"].astype(f).transpose(0, 2, 3, 1).reshape(d["M"], c.K) @ d["w"].reshape(c.K, -1)
    full = oref.row2im(rows, c.N, c.C, c.H + 2 * c.pad, c.W + 2 * c.pad, c.R, c.S, c.stride, d["OH"], d["OW"])
    assert full.dtype == f
    return full[:, :, c.pad:c.pad + c.H, c.pad:c.pad + c.W]


def h_wgrad(d, dy32, l2=0.0, bn=None, p=None):
    c = d["case"]
    p = patches(h_operand(d, bn), c) if p is None else p
    dw = np.asarray(dy32, dtype=f).transpose(0, 2, 3, 1).reshape(d["M"], c.K).T @ p.reshape(d["M"], -1)
    dw = dw.reshape(d["w"].shape)
    return dw + f(l2) * d["w"] if l2 else dw


def h_dy(d, relu, lattice=1):
    """dy of the following BatchNorm's backward in fp32, bn_bwd_elem's operation order."""
    m, i, ga, b = (np.asarray(v, dtype=f)[None, :, None, None] for v in d["po"])
    K = d["K"]
    k1, k2 = d["k12"][:K][None, :, None, None], d["k12"][K:][None, :, None, None]
    g = d["g"] if lattice == 1 else R.widen_lattice(d["g"][:, :, ::2, ::2], d["OH"], d["OW"])
    x1, g = d["x1"].astype(f), g.astype(f)
    xh = (x1 - m) * i
    if relu:
        g = np.where(ga * xh + b > 0, g, f(0))
    return (ga * i) * ((g - k1) - xh * k2)


def h_stats(stored):
    s = R.P.rows(np.asarray(stored, dtype=np.float64))
    return np.stack([s.sum(0), (s * s).sum(0)])[None]


# ---------------------------------------------------------------------------------------------------------
# the honest bf16 implementation: operands rounded to bf16 (weights; an operand formed on load -- raw activations
# are bf16 already), products exact (two 8-bit significands: 16 bits, exact in fp32), fp32 accumulation in one of
# two orders, one round-to-nearest-even store (y, dx) or none (dw, fp32)
# ---------------------------------------------------------------------------------------------------------

ORDERS16 = ("seq", "ktile")


def q16(a):
    """fp32 -> bf16 (nearest even) -> fp32."""
    return torch.tensor(np.ascontiguousarray(a, dtype=f)).to(torch.bfloat16).float().numpy()


def trunc16(a):
    """fp32 -> bf16 by truncation -> fp32."""
    return (np.ascontiguousarray(a, dtype=f).view(np.uint32) & np.uint32(0xFFFF0000)).view(f)


def acc16(a, b, order):
    """a (M, n) @ b (n, N) in fp32 over bf16-valued operands.  "seq": one product at a time, k = 0, 1, ... (each
    product exact, one rounding per add); "ktile": 32-deep k-tiles, each one fp32 matmul, added in order."""
    a, b = np.ascontiguousarray(a, dtype=f), np.ascontiguousarray(b, dtype=f)
    acc = np.zeros((a.shape[0], b.shape[1]), f)
    if order == "seq":
        for k in range(a.shape[1]):
            acc = acc + a[:, k:k + 1] * b[k:k + 1, :]
    else:
        for k in range(0, a.shape[1], 32):
            acc = acc + a[:, k:k + 32] @ b[k:k + 32]
    assert acc.dtype == f
    return acc


def h_operand16(d, bn, rnd=q16):
    a = h_operand(d, bn)
    return a if bn is None else rnd(a)


def h_forward16(d, bn=None, order="seq", p=None, w=None):
    """The fp32 accumulator of y (N,K,OH,OW), before the bias and the store."""
    c = d["case"]
    p = patches(h_operand16(d, bn), c) if p is None else p
    y = acc16(p.reshape(d["M"], -1), (q16(d["w"]) if w is None else w).reshape(c.K, -1).T, order)
    return y.reshape(c.N, d["OH"], d["OW"], c.K).transpose(0, 3, 1, 2)


def h_store16(d, acc, bias=False, store=q16):
    return store(acc + d["bias"][None, :, None, None] if bias else acc)


def h_dgrad16(d, order):
    """dx as stored: the rows in the given order, the taps of a pixel added in fp32 (row2im), one rounding store."""
    c = d["case"]
    rows = acc16(d["dy"].astype(f).transpose(0, 2, 3, 1).reshape(d["M"], c.K), q16(d["w"]).reshape(c.K, -1), order)
    full = oref.row2im(rows, c.N, c.C, c.H + 2 * c.pad, c.W + 2 * c.pad, c.R, c.S, c.stride, d["OH"], d["OW"])
    assert full.dtype == f
    return q16(full[:, :, c.pad:c.pad + c.H, c.pad:c.pad + c.W])


def h_wgrad16(d, bn=None, order="seq", p=None, pixels=None):
    """dw before the l2 term, fp32; pixels: the rows of the reduction that take part (default: all)."""
    c = d["case"]
    p = patches(h_operand16(d, bn), c) if p is None else p
    dy, p = d["dy"].astype(f).transpose(0, 2, 3, 1).reshape(d["M"], c.K), p.reshape(d["M"], -1)
    if pixels is not None:
        dy, p = dy[pixels], p[pixels]
    return acc16(dy.T, p, order).reshape(c.K, -1, c.R, c.S)


def stored16_check(name, got, r):
    """A bf16 store against the closed form and the interval form, each logged under its own name."""
    R.check(name + " closed", got, r.ref, r.b16c)
    R.check(name, got, r.ref, r.b16)


# ---------------------------------------------------------------------------------------------------------
# the reference itself
# ---------------------------------------------------------------------------------------------------------

def _close(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("name", NAMES)
def test_reference_agrees_with_oracle(name):
    d = R.make_inputs(name)
    c = d["case"]
    w64, b64 = d["w"].astype(np.float64), d["bias"].astype(np.float64)
    for bias in (False, True):
        y, cache = oref.conv_forward(d["x"], w64, b64 if bias else None, c.stride, c.pad)
        _close(R.forward(d, bias).ref, y)
        for l2 in (0.0, R.L2):
            dx, dw, _ = oref.conv_backward(d["dy"], w64, cache, c.stride, c.pad, bias, l2)
            assert dx.shape == d["x"].shape
            _close(R.dgrad(d, "phase").ref, dx)
            _close(R.wgrad(d, l2).ref, dw)


@pytest.mark.parametrize("name", NAMES)
def test_dgrad_and_wgrad_are_the_adjoints_of_the_forward(name):
    d = R.make_inputs(name)
    c = d["case"]
    w64 = d["w"].astype(np.float64)
    lhs = float((R.conv(d["x"], w64, c.stride, c.pad) * d["dy"]).sum())
    scale = float((R.conv(np.abs(d["x"]), np.abs(w64), c.stride, c.pad) * np.abs(d["dy"])).sum())
    assert abs(lhs - float((d["x"] * R.dgrad(d, "phase").ref).sum())) <= 1e-12 * scale
    assert abs(lhs - float((w64 * R.wgrad(d).ref).sum())) <= 1e-12 * scale


@pytest.mark.parametrize("name", NAMES)
def test_inputs_keep_the_relu_masks_decided(name):
    """Precondition of every ReLU case, for both BatchNorms of the (case, seed) in SEEDS."""
    assert name in R.SEEDS
    assert R.margins(R.make_inputs(name)) > 1.0


@pytest.mark.parametrize("name", NAMES)
def test_cases_stay_small(name):
    d = R.make_inputs(name)
    for k in ("x", "dy", "w"):
        assert d[k].size <= R.MAX_ELEMENTS, (name, k, d[k].size)


def test_unreached_pixels_have_a_zero_bound():
    for name, entry in (("e6", "phase"), ("e12", "phase"), ("s6", "subpixel"), ("s7", "subpixel")):
        d = R.make_inputs(name)
        r = R.dgrad(d, entry)
        dead = R.conv_dx(np.ones_like(d["dy"]), np.ones_like(d["w"], dtype=np.float64), d["stride"], d["pad"],
                         d["H"], d["W"]) == 0
        assert dead.any() and (r.ref[dead] == 0).all() and (r.A[dead] == 0).all() and (r.A[~dead] > 0).all()


# ---------------------------------------------------------------------------------------------------------
# the bounds admit the honest implementation
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_bounds_admit_the_honest_forward(name):
    d = R.make_inputs(name)
    for narrow in ((False, True) if name in R.NARROW else (False,)):
        for bn in (None, 0, 1):
            for bias in (False, True):
                r = R.forward(d, bias, bn, narrow)
                y = h_forward(d, bias, bn)
                R.check("{} fwd y {}".format(name, "narrow" if narrow else "engine"), y, r.ref, r.A)
                R.stats_checks("{} fwd stats".format(name), h_stats(y), y, r.ref, r.A)


@pytest.mark.parametrize("name", NAMES)
def test_bounds_admit_the_honest_dgrad(name):
    d = R.make_inputs(name)
    dx = h_dgrad(d)
    entries = ["phase"] + (["gemm"] if d["stride"] == 1 else []) + (["subpixel"] if d["stride"] == 2 else [])
    for entry in entries:
        r = R.dgrad(d, entry)
        R.check("{} dgrad dx {}".format(name, entry), dx, r.ref, r.A)


@pytest.mark.parametrize("name", NAMES)
def test_bounds_admit_the_honest_wgrad(name):
    d = R.make_inputs(name)
    for bn in (None, 0, 1):
        for l2 in (0.0, R.L2):
            r = R.wgrad(d, l2, bn)
            R.check("{} wgrad dw {}".format(name, "plain" if bn is None else "bnx"),
                    h_wgrad(d, d["dy"].astype(f), l2, bn), r.ref, r.A)
    for relu in (0, 1):
        for lattice in ((1, 2) if name in R.NARROW else (1,)):
            dy, ed = R.formed_dy(d, relu, lattice)
            for bn in (None, 1):
                r = R.wgrad(d, R.L2, bn, dy, ed)
                R.check("{} wgrad dw bnbwd lat{}".format(name, lattice), h_wgrad(d, h_dy(d, relu, lattice), R.L2, bn),
                        r.ref, r.A)


@pytest.mark.parametrize("name", NAMES)
def test_bf16_bounds_admit_the_honest_forward(name):
    d = R.make_inputs(name)
    for bn in (None, 0, 1):
        for order in ORDERS16:
            acc = h_forward16(d, bn, order)
            for bias in (False, True):
                r = R.forward(d, bias, bn, bf16=True)
                y = h_store16(d, acc, bias)
                stored16_check("{} bf16 fwd y".format(name), y, r)
                R.stats_checks("{} bf16 fwd stats".format(name), h_stats(y), y, r.ref, r.b16)


@pytest.mark.parametrize("name", NAMES)
def test_bf16_bounds_admit_the_honest_dgrad(name):
    d = R.make_inputs(name)
    for order in ORDERS16:
        dx = h_dgrad16(d, order)
        for entry in ["phase"] + (["gemm"] if d["stride"] == 1 else []):
            stored16_check("{} bf16 dgrad dx {}".format(name, entry), dx, R.dgrad(d, entry, bf16=True))


@pytest.mark.parametrize("name", NAMES)
def test_bf16_bounds_admit_the_honest_wgrad(name):
    d = R.make_inputs(name)
    for bn in (None, 0, 1):
        for order in ORDERS16:
            dw = h_wgrad16(d, bn, order)
            for l2 in (0.0, R.L2):
                r = R.wgrad(d, l2, bn, bf16=True)
                R.check("{} bf16 wgrad dw {}".format(name, "plain" if bn is None else "bnx"),
                        dw + f(l2) * d["w"] if l2 else dw, r.ref, r.A)


def test_bf16_unreached_pixels_have_a_zero_bound():
    for name in ("e6", "e12"):
        d = R.make_inputs(name)
        r = R.dgrad(d, "phase", bf16=True)
        dead = R.taps_map(d["case"])[None, None] * np.ones_like(r.ref) == 0
        dead |= R.conv_dx(np.ones_like(d["dy"]), np.ones_like(d["w"], dtype=np.float64), d["stride"], d["pad"],
                          d["H"], d["W"]) == 0
        assert dead.any() and (r.ref[dead] == 0).all() and (r.b16[dead] == 0).all() and (r.b16c[dead] == 0).all()
        assert (r.b16[~dead] > 0).all()


# ---------------------------------------------------------------------------------------------------------
# the bounds reject the defects
# ---------------------------------------------------------------------------------------------------------

def defect(k):
    """(name, got, ref, bound): a mutation of the honest implementation and the bound that must reject it."""
    if k == "tap":          # the centre tap (inside the image) dropped at the corner pixel of image 0
        d = R.make_inputs("e1")
        r, y = R.forward(d), h_forward(d).copy()
        y[0, :, 0, 0] -= d["w"][:, :, 1, 1] @ d["x"][0, :, 0, 0].astype(f)
        return "one tap dropped at one border pixel", y, r.ref, r.A
    if k == "padding":      # the BatchNorm applied to the zero padding: bn(0) where 0 belongs
        d = R.make_inputs("e1")
        c = d["case"]
        r = R.forward(d, False, 0)
        a = bn_operand_f32(oref.pad_input(d["x"], c.pad), R.pi_of(d, 0))
        return "padding normalised", h_forward(d, p=patches(a, c._replace(pad=0, H=c.H + 2, W=c.W + 2))), r.ref, r.A
    if k in ("ring", "ring-multirow"):
        # the newest window row (r = R - 1) of an image's first output row taken from the image before it: the
        # weight gradient's ring not restaged when a block crosses into the next image
        d = R.make_inputs("n4" if k == "ring" else "nm1")
        c = d["case"]
        p = patches(d["x"].astype(f), c).copy()
        for n in (range(1, c.N) if k == "ring-multirow" else (1,)):
            p[n, 0, :, :, c.R - 1, :] = patches(d["x"][n - 1:n].astype(f), c)[0, 0, :, :, c.R - 1, :]
        r = R.wgrad(d)
        return "input row from the neighbouring image", h_wgrad(d, d["dy"].astype(f), p=p), r.ref, r.A
    if k == "column":       # one (c, r, s) column of dw misses one output row's contribution
        d = R.make_inputs("n4")
        p = patches(d["x"].astype(f), d["case"]).copy()
        p[1, 2, :, 1, 1, 1] = 0
        r = R.wgrad(d)
        return "dw column misses one output row", h_wgrad(d, d["dy"].astype(f), p=p), r.ref, r.A
    if k == "leak":         # the padded channel's column (bn(0) of the zero channel, not zero) added into channel C - 1
        d = R.make_inputs("e4")
        c = d["case"]
        r = R.wgrad(d, 0.0, 0)
        m, i, ga, be = (v[c.C:].astype(f) for v in d["pi"])
        a = np.concatenate([h_operand(d, 0), np.broadcast_to((ga * ((f(0) - m) * i) + be)[None, :, None, None],
                                                             (c.N, c.Cp - c.C, c.H, c.W))], axis=1)
        dwp = d["dy"].astype(f).transpose(0, 2, 3, 1).reshape(d["M"], c.K).T @ patches(a, c).reshape(d["M"], -1)
        dwp = dwp.reshape(c.K, c.Cp, c.R, c.S)
        dw = dwp[:, :c.C].copy()
        dw[:, c.C - 1] += dwp[:, c.C]
        return "padded channel leaks into dw", dw, r.ref, r.A
    # the bf16 mode: mutations of the honest bf16 implementation
    if k == "trunc16":      # the store truncates instead of rounding to nearest even: the interval form
        d = R.make_inputs("e1")
        r = R.forward(d, bf16=True)
        return "bf16 store truncating", h_store16(d, h_forward16(d), store=trunc16), r.ref, r.b16
    if k == "tap16":        # "tap" in bf16
        d = R.make_inputs("e1")
        r, acc = R.forward(d, bf16=True), h_forward16(d).copy()
        acc[0, :, 0, 0] -= q16(d["w"])[:, :, 1, 1] @ d["x"][0, :, 0, 0].astype(f)
        return "bf16: one tap dropped at one border pixel", q16(acc), r.ref, r.b16
    if k == "padding16":    # "padding" in bf16: rne_bf16(bn(0)) where 0 belongs
        d = R.make_inputs("e1")
        c = d["case"]
        r = R.forward(d, False, 0, bf16=True)
        a = q16(bn_operand_f32(oref.pad_input(d["x"], c.pad), R.pi_of(d, 0)))
        acc = h_forward16(d, p=patches(a, c._replace(pad=0, H=c.H + 2, W=c.W + 2)))
        return "bf16: padding normalised", q16(acc), r.ref, r.b16
    if k == "slab16":       # dw without one split's slab: e1 in bf16 runs 9 splits of 32 pixels; the first is missing
        d = R.make_inputs("e1")
        r = R.wgrad(d, bf16=True)
        return "bf16: dw misses one split's slab", h_wgrad16(d, pixels=np.arange(32, d["M"])), r.ref, r.A
    if k == "leak16":       # "leak" in bf16, under the looser bound of a rounded operand
        d = R.make_inputs("e4")
        c = d["case"]
        r = R.wgrad(d, 0.0, 0, bf16=True)
        m, i, ga, be = (v[c.C:].astype(f) for v in d["pi"])
        a = np.concatenate([h_operand(d, 0), np.broadcast_to((ga * ((f(0) - m) * i) + be)[None, :, None, None],
                                                             (c.N, c.Cp - c.C, c.H, c.W))], axis=1)
        dwp = h_wgrad16(d, p=patches(q16(a), c))
        dw = dwp[:, :c.C].copy()
        dw[:, c.C - 1] += dwp[:, c.C]
        return "bf16: padded channel leaks into dw", dw, r.ref, r.A
    raise KeyError(k)


@pytest.mark.parametrize("k", ["tap", "padding", "ring", "ring-multirow", "column", "leak",
                               "trunc16", "tap16", "padding16", "slab16", "leak16"])
def test_bounds_reject_defects(k):
    name, got, ref, bound = defect(k)
    ratio, at = R.worst(got, ref, bound)
    print("defect {} ({}): worst err/bound {:.3g} at {}".format(k, name, ratio, at))
    assert ratio > 1.0, (name, ratio)


def test_bounds_reject_statistics_defects():
    """A row of y missing from the statistics, or counted twice: the sums-of-the-stored-outputs check."""
    d = R.make_inputs("e1")
    r = R.forward(d)
    y = h_forward(d)
    R.stats_checks("honest", h_stats(y), y, r.ref, r.A)
    row = R.P.rows(y.astype(np.float64))[-1]
    for sign in (-1.0, 1.0):
        bad = h_stats(y) + sign * np.stack([row, row * row])[None]
        with pytest.raises(AssertionError, match="stored"):
            R.stats_checks("row {}".format("twice" if sign > 0 else "missing"), bad, y, r.ref, r.A)


def test_bf16_bounds_reject_statistics_defects():
    """Statistics taken from the fp32 accumulator instead of the rounded stored value, a row of y missing from them
    or counted twice: each through check (1), the sums of what the same call stored.  Check (2), against the
    reference, admits the first: the accumulator is within the per-element bounds it sums."""
    d = R.make_inputs("e1")
    r = R.forward(d, bf16=True)
    acc = h_forward16(d)
    y = q16(acc)
    R.stats_checks("honest", h_stats(y), y, r.ref, r.b16)
    with pytest.raises(AssertionError, match="stored"):
        R.stats_checks("unrounded", h_stats(acc), y, r.ref, r.b16)
    s, s32 = R.P.rows(y.astype(np.float64)), R.P.rows(acc.astype(np.float64))
    lim = R.P.EPS * (s.shape[0] + 3)
    print("statistics of the accumulator: err/bound {:.3g} (sum), {:.3g} (squares) of the stored-sums bound".format(
        R.worst(s32.sum(0), s.sum(0), lim * np.abs(s).sum(0))[0],
        R.worst((s32 * s32).sum(0), (s * s).sum(0), lim * (s * s).sum(0))[0]))
    for name in ("sum|ref", "sq|ref"):
        i = int(name == "sq|ref")
        ref = R.P.rows(r.ref)
        b = R.P.rows(r.b16)
        bound = b.sum(0) if i == 0 else (b * (2 * np.abs(ref) + b)).sum(0)
        assert R.worst(h_stats(acc)[0, i], (ref if i == 0 else ref * ref).sum(0), bound)[0] <= 1.0
    row = s[-1]
    for sign in (-1.0, 1.0):
        bad = h_stats(y) + sign * np.stack([row, row * row])[None]
        with pytest.raises(AssertionError, match="stored"):
            R.stats_checks("row {}".format("twice" if sign > 0 else "missing"), bad, y, r.ref, r.b16)


def test_mutations_the_bf16_bounds_cannot_reject():
    """Facts about the derived bounds, each asserted so that it is noticed if it stops holding:
      * a truncating store against the closed form alone stays within a factor of 2 (one ulp against a half): the
        interval form exists for it (defect "trunc16");
      * a bn(x) operand rounded to bf16 by truncation instead of to nearest even stays within the bound of y (1.000
        of the interval form at e1: the operand's own slack 2^-8 (|v| + e) summed over 72 terms covers it);
      * the weights rounded by truncation are rejected where x is raw bf16 (2.7e4: the reference's wq is exact),
        but behind a BatchNorm on load the same operand slack all but hides them (1.19 at e1; printed, not
        asserted, as a margin that small is a property of the seed);
      * no bound on dw sees the weights' rounding at all (w enters dw only as the fp32 l2 term)."""
    d = R.make_inputs("e1")
    r = R.forward(d, bf16=True)
    closed = R.worst(h_store16(d, h_forward16(d), store=trunc16), r.ref, r.b16c)[0]
    rb = R.forward(d, False, 1, bf16=True)
    c = d["case"]
    operand = R.worst(q16(h_forward16(d, p=patches(h_operand16(d, 1, trunc16), c))), rb.ref, rb.b16)[0]
    wt = trunc16(d["w"])
    raw = R.worst(q16(h_forward16(d, w=wt)), r.ref, r.b16)[0]
    behind = R.worst(q16(h_forward16(d, 1, w=wt)), rb.ref, rb.b16)[0]
    print("truncating store | closed form {:.3g}; truncated bn operand {:.3g}; truncated weights: raw x {:.3g}, behind "
          "BN on load {:.3g}".format(closed, operand, raw, behind))
    assert 1.0 < closed < 2.0
    assert raw > 1.0
    assert operand <= 1.0
