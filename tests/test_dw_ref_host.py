"""tests/_dw_ref.py on the CPU: the fp64 reference agrees with the oracle, its per-element bounds admit a
correct fp32 implementation (torch-CPU conv2d(groups=C) and its autograd; rounded once through bf16 for the
bf16-storage bounds) on every geometry with nothing excluded, and they reject eight wrong kernels -- each a
mutation of that implementation of the kind a depthwise kernel can have -- by a factor of ten or more
(measured 3.6e3 .. 1.1e7).

What the old normwise checks saw of each mutant is computed too (normwise error of the mutated tensor):
  * no mutant of 1-7 can stay below the old 1e-4 at these sizes, and the test asserts that rather than
    pretend otherwise: one wrong element among M is about 1 / sqrt(R S M) of the norm, 2e-2 at M = 2160, so a
    normwise 1e-4 passes it only on a tensor of M (norm / 1e-4)^2 elements -- printed per mutant; for the
    single dropped tap that is 9e7 elements, the first depthwise layer of config 5 at its batch size
    (512 x 56 x 56 x 64 = 1.03e8), where the per-element bound still fails by the same factor of 1e6.
    Mutants 4-7 are wrong in a whole column, filter, phase or segment and are far above 1e-4 at any size: the
    normwise tests catch them wherever the geometry runs at all, and the gap closed for them is the geometry
    (stride-1 padding 0 and R - 1, odd strided shapes), not the bound;
  * mutant 8 (bf16 store truncating) is 3.4e-3 normwise: below the old bf16 bound 1e-2 (asserted)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref as oref
from tests import _dw_ref as D

L2 = float(np.float32(1e-3))
GIDS = sorted(D.GEOMS)


def f32_impl(d, bn=None, bias=False, res=False, l2=0.0, a32=None):
    """y, dx, dw of a correct fp32 implementation (numpy fp32 arrays)."""
    a = torch.tensor(D.bn_operand_f32(d["x"], bn) if a32 is None else a32, requires_grad=True)
    w = torch.tensor(d["w"][:, None], requires_grad=True)
    y = F.conv2d(a, w, torch.tensor(d["bias"]) if bias else None, d["stride"], d["pad"], groups=d["C"])
    y.backward(torch.tensor(d["dy"].astype(np.float32)))
    dx = a.grad.numpy()
    if res:
        dx = dx + d["res"].astype(np.float32)
    dw = w.grad.numpy()[:, 0]
    if l2:
        dw = dw + np.float32(l2) * d["w"]
    return y.detach().numpy(), dx, dw


def through_bf16(a):
    return torch.tensor(a).to(torch.bfloat16).float().numpy()


def ref_of(d, bn=None, bias=False, res=False, l2=0.0):
    return D.reference(d["x"], d["w"], d["stride"], d["pad"], d["bias"] if bias else None, bn, d["dy"],
                       d["res"] if res else None, l2)


@pytest.mark.parametrize("gid", GIDS)
def test_reference_agrees_with_oracle(gid):
    d = D.make_inputs(gid)
    w64 = d["w"].astype(np.float64)
    for bias in (False, True):
        for l2 in (0.0, L2):
            r = ref_of(d, None, bias, False, l2)
            y, cache = oref.depthwise_forward(d["x"], w64, d["bias"].astype(np.float64) if bias else None,
                                              d["stride"], d["pad"])
            dx, dw, _ = oref.depthwise_backward(d["dy"], w64, cache, d["stride"], d["pad"], bias, l2)
            for got, want in ((r.y, y), (r.dx, dx), (r.dw, dw)):
                assert got.shape == want.shape
                assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_absolute_twins_and_zero_bounds():
    """Where no tap reaches an element the bound is exactly 0: stride-2 1x1 phases, and the last input row of
    geometry 9 (H = 10: the four output rows reach rows 0..8; W = 11 is reached to its last column)."""
    r = ref_of(D.make_inputs(15))
    assert (r.bx[:, :, 1::2, :] == 0).all() and (r.bx[:, :, :, 1::2] == 0).all() and (r.bx[:, :, ::2, ::2] > 0).all()
    r = ref_of(D.make_inputs(9))
    assert (r.bx[:, :, -1, :] == 0).all() and (r.dx[:, :, -1, :] == 0).all() and (r.bx[:, :, :-1, :] > 0).all()


@pytest.mark.parametrize("bn", [None, 0, 1], ids=["plain", "bn", "bnrelu"])
@pytest.mark.parametrize("gid", GIDS)
def test_bounds_admit_a_correct_fp32_implementation(gid, bn):
    d = D.make_inputs(gid)
    bnp = None if bn is None else (*d["bn"], bn)
    for bias, res, l2 in ((False, False, 0.0), (True, True, L2)):
        r = ref_of(d, bnp, bias, res, l2)
        y, dx, dw = f32_impl(d, bnp, bias, res, l2)
        tag = "g{}".format(gid)
        D.check(tag + " y f32", y, r.y, r.by)
        D.check(tag + " dx f32", dx, r.dx, r.bx)
        D.check(tag + " dw", dw, r.dw, r.bw)
        D.check(tag + " y bf16", through_bf16(y), r.y, r.by16)
        D.check(tag + " dx bf16", through_bf16(dx), r.dx, r.bx16)


def test_worst_counts_nan_and_zero_bound():
    ref, b = np.zeros((2, 2)), np.array([[0.0, 1.0], [1.0, 1.0]])
    assert D.worst(np.zeros((2, 2)), ref, b)[0] == 0.0
    assert D.worst(np.array([[1e-30, 0], [0, 0]]), ref, b) == (np.inf, (0, 0))
    assert D.worst(np.array([[0, 0], [np.nan, 0]]), ref, b) == (np.inf, (1, 0))


def _rel(a, b):
    return float(np.linalg.norm((np.asarray(a, np.float64) - b).ravel()) / np.linalg.norm(b.ravel()))


def _truncate_bf16(a):
    return (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def mutant(k):
    """(name, got, ref, bound, old normwise tolerance, whether the mutant stays below it)."""
    if k == 1:    # one tap dropped at one corner output pixel
        d = D.make_inputs(1)
        r, (y, _, _) = ref_of(d), f32_impl(d)
        y = y.copy()
        y[0, 0, 0, 0] -= d["w"][0, 1, 1] * np.float32(d["x"][0, 0, 0, 0])
        return "dropped tap", y, r.y, r.by, 1e-4, False
    if k == 2:    # the last row of the first 14-row segment (10 rows at OH = 30) taken from the row above
        d = D.make_inputs(4)
        r, (y, _, _) = ref_of(d), f32_impl(d)
        y = y.copy()
        y[0, 0:4, 9, 0:4] = y[0, 0:4, 8, 0:4]
        return "segment's last row", y, r.y, r.by, 1e-4, False
    if k == 3:    # the last column of a ragged 4-wide chunk (W = 9: column 8) left at its fill value, 0
        d = D.make_inputs(1)
        r, (y, _, _) = ref_of(d), f32_impl(d)
        y = y.copy()
        y[0, 0:4, 0:8, 8] = 0
        return "ragged column unwritten", y, r.y, r.by, 1e-4, False
    if k == 4:    # padding off by one on the left edge only: output column 0 reads one column further left
        d = D.make_inputs(2)
        r, (y, _, _) = ref_of(d), f32_impl(d)
        x = d["x"].astype(np.float32)
        shifted = np.zeros_like(x)
        shifted[..., 1:] = x[..., :-1]
        y = y.copy()
        y[..., 0] = f32_impl(d, a32=shifted)[0][..., 0]
        return "left padding", y, r.y, r.by, 1e-4, False
    if k == 5:    # the dgrad filter not flipped
        d = D.make_inputs(3)
        r = ref_of(d)
        dx = D.dgrad(d["dy"], d["w"][:, ::-1, ::-1].astype(np.float64), 1, d["pad"], d["H"], d["W"])
        return "unflipped dgrad filter", dx.astype(np.float32), r.dx, r.bx, 1e-4, False
    if k == 6:    # one sub-pixel phase of a stride-2 dgrad shifted by one quad
        d = D.make_inputs(7)
        r, (_, dx, _) = ref_of(d), f32_impl(d)
        dx = dx.copy()
        dx[:, :, 1::2, 1::2] = np.roll(dx[:, :, 1::2, 1::2], 1, axis=3)
        return "phase shifted", dx, r.dx, r.bx, 1e-4, False
    if k == 7:    # dw missing the last 8-row weight-gradient segment (rows 24..29 of 30) of one image
        d = D.make_inputs(4)
        r = ref_of(d, l2=L2)
        dy = d["dy"].copy()
        dy[0, :, 24:, :] = 0
        dw = D.wgrad(dy, d["x"], 3, 3, 1, 1) + L2 * d["w"]
        return "wgrad segment", dw.astype(np.float32), r.dw, r.bw, 1e-4, False
    if k == 8:    # the bf16 store truncating instead of rounding to nearest even
        d = D.make_inputs(1)
        r, (y, _, _) = ref_of(d), f32_impl(d)
        return "bf16 truncation", _truncate_bf16(y), r.y, r.by16, 1e-2, True
    raise KeyError(k)


@pytest.mark.parametrize("k", range(1, 9))
def test_bounds_reject_mutants(k):
    """Every mutant must exceed its bound on at least one element by a factor of 10 or more.

    Measured worst err / bound: 1 dropped tap 9.4e5; 2 segment row 3.9e6; 3 unwritten column 1.4e6;
    4 left padding 2.0e6; 5 unflipped filter 2.9e6; 6 shifted phase 1.1e7; 7 wgrad segment 5.4e3;
    8 bf16 truncation 3.6e3.
    Mutant 8 is what the interval form of the bf16 bound is for (_dw_ref.bf16_bound): against the closed
    form 2^-8 (|ref| + A) + A a truncating store, off by less than one ulp where a correct one is off by at
    most a half, never exceeds a factor of 2 (1.90 here); against rne(ref - A) .. rne(ref + A) it is off by
    nearly a whole ulp where the reference lies just below a bf16 value and only ref's distance to that
    value is allowed."""
    name, got, ref, bound, old, below = mutant(k)
    ratio, at = D.worst(got, ref, bound)
    norm = _rel(got, ref)
    print("mutant {} ({}): worst err/bound {:.3g} at {}, normwise {:.3g}".format(k, name, ratio, at, norm))
    print("  a normwise {:g} passes it from {:.2g} elements (here {})".format(old, ref.size * (norm / old) ** 2, ref.size))
    if below:
        assert norm < old
    else:       # cannot stay below the old tolerance on a tensor this small (module docstring)
        assert norm > old
    assert ratio >= 10, (name, ratio)


def test_bf16_bound_is_never_wider_than_its_closed_form():
    """The interval form of the bf16 store bound against the closed form 2^-8 (|ref| + A) + A on every
    geometry: never wider, and the closed form alone passes a truncating store within a factor of 2 --
    below the factor of ten asked of a bound that is to tell it from a rounding one."""
    for gid in GIDS:
        r = ref_of(D.make_inputs(gid), bias=True, res=True)
        for ref, A, b16 in ((r.y, r.by, r.by16), (r.dx, r.bx, r.bx16)):
            assert (b16 <= D.UB * (np.abs(ref) + A) + A).all() and (b16 >= 0).all()
    _, got, ref, _, _, _ = mutant(8)
    A = ref_of(D.make_inputs(1)).by
    assert 1.0 < D.worst(got, ref, D.UB * (np.abs(ref) + A) + A)[0] < 2.0


def test_rne_bf16_is_torch_rounding():
    rng = np.random.RandomState(0)
    v = (rng.randn(100000) * np.exp(3 * rng.randn(100000))).astype(np.float32)
    v[:4] = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 0.0]    # ties go to even
    assert (D.rne_bf16(v.astype(np.float64)) == through_bf16(v).astype(np.float64)).all()


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("fid", sorted(D.FUSED))
def test_fused_inputs_keep_the_relu_mask_decided(fid, relu):
    """Precondition of the fused-backward tests: no element of bn(x1) lies within 8 u (|gamma x_hat| + |beta|)
    of zero, so fp32 and fp64 decide the ReLU mask alike for the fixed seeds."""
    d = D.make_fused_inputs(fid, relu)
    assert D.mask_margin(d["x1"], d["po"]) > 1.0


@pytest.mark.parametrize("bn_in", [False, True])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("fid", sorted(D.FUSED))
def test_fused_bounds_admit_a_correct_fp32_implementation(fid, relu, bn_in):
    """The fused backward's bounds (dy's error scale ed entering dx and dw) admit dy formed in fp32 in
    bn_bwd_elem's operation order followed by the fp32 convolution gradients."""
    d = D.make_fused_inputs(fid, relu)
    f = np.float32
    m, i, ga, b = (np.asarray(v, dtype=f)[None, :, None, None] for v in d["po"][:4])
    C = d["C"]
    k1, k2 = d["k12"][:C][None, :, None, None], d["k12"][C:][None, :, None, None]
    x1, g = d["x1"].astype(f), d["g"].astype(f)
    xh = (x1 - m) * i
    if relu:
        g = np.where(ga * xh + b > 0, g, f(0))
    dy32 = (ga * i) * ((g - k1) - xh * k2)
    pi = (*d["pi"], 1) if bn_in else None
    dy, ed, _ = D.bn_bwd_dy(d["g"], d["x1"], d["po"], d["k12"])
    assert D.worst(dy32, dy, ed)[0] <= 1.0
    r = D.reference(d["x"], d["w"], 1, 1, None, pi, dy, d["res"], L2, dy_err=ed)
    dd = dict(d, dy=dy32.astype(np.float64))
    _, dx, dw = f32_impl(dd, pi, False, True, L2)
    D.check("fused dx", dx, r.dx, r.bx)
    D.check("fused dx bf16", through_bf16(dx), r.dx, r.bx16)
    D.check("fused dw", dw, r.dw, r.bw)
