"""tests/_bn_ref.py on the CPU: the fp64 reference agrees with the oracle, its per-element bounds admit an honest
implementation -- a numpy transcription of every kernel of batchnorm.hip in the kernel's own operation order (fp32
where the kernel is fp32, fp64 sums, bf16 stores rounded to nearest even), the partial sums taken over two groupings
of the rows (the kernel's blocks, lanes and strides; chunks of seven rows summed pairwise) and folded in two orders
(bn_fold_kernel's lanes, block_sum2's tree) -- on every case, and they reject defective ones, each a mutation of that
transcription of a kind a BatchNorm kernel can have.

Worst err / bound of the honest implementation over the 13 cases and both groupings (results, not tolerances; ReLU off /
on where two figures stand; a bf16 store attains the interval form's end by construction, so its 1.000 is "at the
bound", the closed form's figure in brackets):

    statistics sums               0.000 (sums of bf16 values and their squares are exact in fp64 at these sizes)
    mean, run_mean (first)        0.964       std, run_std (first)     0.821       invstd        0.693
    run_mean (blend)              0.943       run_std (blend)          0.849
    apply y, fp32                 0.800 / 0.794            bf16   1.000 (0.995)    mask bytes: equal
    backward sums                 0.794 / 0.779            behind a join's mask    0.723 / 0.756
    dgamma                        0.632 / 0.674            dbeta  0.930 / 0.826    k12           0.975
    backward apply dx, fp32       0.535 / 0.557            bf16   1.000 (0.995)
    one-shot dx, fp32             0.494 / 0.506            bf16   1.000
The figures near 1 are single fp32 roundings held to their half ulp, u |v|: mean, dbeta, k12 are (float) of an
fp64 value and attain up to 1 wherever |v| lies just above a power of two (a half ulp is then u |v| nearly); the
backward sums at P = 1 (case 4) are one product whose x_hat carries two fp32 roundings against XH = 2 u.

Defects (case 2: P = 3219, C = 24), the check that must fail, worst err / bound and (normwise error of that tensor):

    the last row of block 0's range dropped       sums             3.4e9   (3.2e-4)
    that row counted twice                        sums             3.4e9   (3.2e-4)
    sample variance, n / (n - 1)                  std              1.3e3   (1.6e-4);  case 1, P = 8193: 512 (6.1e-5)
    sqrt(var) + eps                               std              1.1e7   (8.4e-4);  (3.2e-6) on the layer test's data
    first flag ignored                            run_mean         inf     (9.4e-1)   (the all-zero channel's bound is 0)
    momentum on the new value                     run_mean         8.5e7   (9.1)
    truncating bf16 store                         apply y, bf16    6.0e3   (2.4e-3)
    ReLU mask from x_hat > 0                      mask bytes       inf     (9.3e-1)
    k1 missing from dx                            dx               2.8e6   (8.4e-2)
    k2 not divided by count                       k12              2.5e9   (3.2e3)
    x_hat formed with std in place of invstd      dx               6.2e6   (3.7e-1)
    last channel group never written              apply y          inf     (4.1e-2)   (NaN left in the output)

What the suite's normwise 1e-4 (tests/test_gpu_layers.py) lets through, asserted below.  At case 2 each defect is
above 1e-4, the first four by a factor of 1.6 to 8 only and through this module's inputs, not by construction:
  * the sample variance is a relative 1 / (2 (P - 1)) on every std: within 1e-4 from P = 5002 on (case 1: 6.1e-5,
    512 times its bound here);
  * sqrt(var) + eps is eps off in absolute terms: 8.4e-4 here through the constant channel alone (std = sqrt(eps)),
    3.2e-6 on test_batchnorm_layer's own data (3 + 2.5 randn), 1.1e7 times its bound here;
  * a dropped or doubled row is 1 / P of one sum: within 1e-4 from some 10^4 rows on -- and the layer test's shapes
    never had a second block whose range could be cut wrongly;
  * the truncating store, the mask and the bf16 entries had no reference at all: the layer tests are fp32, and
    every bf16 test compares with an fp32 twin of the same kernel.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import ref as oref
from tests import _bn_ref as B
from tests._convert import rel_err

f = np.float32
CIDS = sorted(B.CASES)
GROUPINGS = (("kernel", "fold"), ("chunks", "tree"))
OLD_TOL = 1e-4


@functools.lru_cache(maxsize=None)
def inputs(cid):
    return B.make_inputs(cid)


# ---------------------------------------------------------------------------------------------------------
# the honest implementation (defect: one of the mutations below)
# ---------------------------------------------------------------------------------------------------------

def q16(a):
    """fp32 -> bf16 (nearest even) -> fp32."""
    return torch.tensor(np.ascontiguousarray(a, dtype=f)).to(torch.bfloat16).float().numpy()


def trunc16(a):
    return (np.ascontiguousarray(a, dtype=f).view(np.uint32) & np.uint32(0xFFFF0000)).view(f)


def h_store(v, bf16, defect=None, V=1):
    out = (trunc16(v) if defect == "trunc_store" else q16(v)) if bf16 else np.array(v, dtype=f)
    if defect == "last_group":
        out[:, -V:] = np.nan
    return out


def seq(a):
    """Sequential fp64 sum over axis 0 (0 for no rows)."""
    return np.cumsum(a, axis=0)[-1] if a.shape[0] else np.zeros(a.shape[1:])


def h_partials(ts, tq, grouping, defect=None):
    """part[nblk][2][C] of the fp64 terms ts, tq [P][C] (bn_stats_partial_kernel / bn_bwd_partial_kernel)."""
    P, C = ts.shape
    nblk = B.bn_blocks(P, C)
    ppb = B.cdiv(P, nblk)
    PL = B.row_geom(C, 4 if C % 4 == 0 else 1)[2]
    part = np.zeros((nblk, 2, C))
    for b in range(nblk):
        p0, p1 = b * ppb, min(P, (b + 1) * ppb)
        if defect == "drop_row" and b == 0:
            p1 -= 1
        for w, t in enumerate((ts, tq)):
            if grouping == "kernel":
                acc = np.zeros(C)
                for lane in [seq(t[p0 + pl:p1:PL]) for pl in range(PL)]:
                    acc = acc + lane
            else:
                acc = np.zeros(C)
                for r in range(p0, p1, 7):
                    acc = acc + t[r:min(r + 7, p1)][::-1].sum(axis=0)
            if defect == "double_row" and b == 0:
                acc = acc + t[p1 - 1]
            part[b, w] = acc
    return part


def fold256(rows):
    """One bn_fold_kernel block: 16 lanes of up to 16 rows each, the lanes added in order."""
    acc = np.zeros(rows.shape[1:])
    for rl in range(16):
        acc = acc + seq(rows[rl::16])
    return acc


def h_fold(part, how):
    """[2][C] column sums of part[nblk][2][C]."""
    if how == "fold":
        while part.shape[0] > 256:
            part = np.stack([fold256(part[i:i + 256]) for i in range(0, part.shape[0], 256)])
        return fold256(part)
    r = np.stack([seq(part[t::256]) for t in range(256)])       # block_sum2
    o = 128
    while o:
        r[:o] += r[o:2 * o]
        o >>= 1
    return r[0]


def h_stats2(S, Q, count, first, rm0, rs0, defect=None):
    """bn_finalize_channel, mode 0."""
    eps, mom = B.BN_EPS, B.MOMENTUM
    om = f(1.0) - mom
    mean = S / count
    var = np.maximum(Q / count - mean * mean, 0.0)
    if defect == "sample_var":
        var = var * count / (count - 1)
    meanf = mean.astype(f)
    stdf = (np.sqrt(var.astype(f)) + eps) if defect == "eps_outside" else np.sqrt(var.astype(f) + eps)
    o = dict(mean=meanf, std=stdf, invstd=f(1.0) / stdf)
    if first and defect != "first_ignored":
        o["run_mean"], o["run_std"] = meanf, stdf
    else:
        a, b = (om, mom) if defect == "momentum_swapped" else (mom, om)
        o["run_mean"] = a * rm0 + b * meanf
        o["run_std"] = a * rs0 + b * stdf
    assert all(v.dtype == f for v in o.values())
    return o


def h_xhat(x, bn, defect=None):
    m, i = bn[0][None, :], bn[1][None, :]
    return (x.astype(f) - m) * ((f(1.0) / i) if defect == "std_for_invstd" else i)


def h_apply(x, bn, relu, bf16, defect=None):
    """bn_apply_kernel: (y as stored, mask)."""
    ga, be = bn[2][None, :], bn[3][None, :]
    xh = h_xhat(x, bn)
    r = ga * xh + be
    pos = (xh > 0) if defect == "mask_xhat" else (r > 0)
    if relu:
        r = np.where(pos, r, f(0))
    V = 4 if x.shape[1] % 4 == 0 else 1
    return h_store(r, bf16, defect, V), (pos if relu else np.zeros_like(pos)).astype(np.uint8)


def h_bwd_terms(x, g, bn, relu, mask8=None, defect=None):
    """bn_bwd_partial_kernel's terms: (g_e, g_e x_hat) in fp64 from the fp32 x_hat, and g_e as stored."""
    ga, be = bn[2][None, :], bn[3][None, :]
    xh = h_xhat(x, bn, defect)
    ge = g.astype(f) if mask8 is None else np.where(mask8 != 0, g.astype(f), f(0))
    gout = ge
    if relu:
        ge = np.where(ga * xh + be > 0, ge, f(0))
    return ge.astype(np.float64), ge.astype(np.float64) * xh.astype(np.float64), gout


def h_bwd2(S, Q, count, defect=None):
    """bn_finalize_channel, mode 1."""
    k2 = Q if defect == "k2_undivided" else Q / count
    return dict(dgamma=Q.astype(f), dbeta=S.astype(f), k12=np.concatenate([(S / count).astype(f), k2.astype(f)]))


def h_dx(x, g, bn, relu, k12, bf16, defect=None):
    """bn_bwd_apply_kernel / bn_bwd_elem."""
    C = x.shape[1]
    i, ga, be = bn[1][None, :], bn[2][None, :], bn[3][None, :]
    k1, k2 = k12[:C][None, :], k12[C:][None, :]
    xh = h_xhat(x, bn, defect)
    ge = g.astype(f)
    if relu:
        ge = np.where(ga * h_xhat(x, bn) + be > 0, ge, f(0))
    t = ge if defect == "k1_missing" else ge - k1
    fma = ((-xh).astype(np.float64) * k2.astype(np.float64) + t.astype(np.float64)).astype(f)
    return h_store((ga * i) * fma, bf16, defect, 4 if C % 4 == 0 else 1)


# ---------------------------------------------------------------------------------------------------------
# every check of one case: [(name, got, ref, bound)]
# ---------------------------------------------------------------------------------------------------------

def checks(cid, grouping=GROUPINGS[0], defect=None):
    d = inputs(cid)
    x, g, bn, P, C = d["x"], d["g"], d["bn"], d["P"], d["C"]
    rows_how, fold_how = grouping
    nblk = B.bn_blocks(P, C)
    out = []
    # statistics
    part = h_partials(x, x * x, rows_how, defect)
    got = h_fold(part, fold_how)
    sm = B.stats_sums(x, nblk, 1)
    out.append(("stats sums", got, sm.ref, sm.bound))
    for first in (1, 0):
        r = B.stats_stage2(sm, float(P), first, d["run_mean0"], d["run_std0"])
        h = h_stats2(got[0], got[1], float(P), first, d["run_mean0"], d["run_std0"], defect)
        for k in B.STATS_FIELDS:
            out.append(("stats first{} {}".format(first, k), h[k], getattr(r, k), getattr(r, "e_" + k)))
    # apply, backward reduce and apply
    for relu in (0, 1):
        for bf16 in (False, True):
            if bf16 and C % 4:
                continue
            nm = "relu{} {}".format(relu, "bf16" if bf16 else "f32")
            r = B.apply_ref(x, bn, relu)
            y, mask = h_apply(x, bn, relu, bf16, defect)
            out.append(("apply y " + nm, y, r.ref, r.bound(bf16)))
            if bf16:
                out.append(("apply y closed " + nm, y, r.ref, r.b16c))
            out.append(("apply mask " + nm, mask, r.mask.astype(np.float64), np.zeros(mask.shape)))
            rd = B.bwd_apply_ref(x, g, bn, relu, d["k12"])
            dx = h_dx(x, g, bn, relu, d["k12"], bf16, defect)
            out.append(("bwd_apply dx " + nm, dx, rd.ref, rd.bound(bf16)))
            if bf16:
                out.append(("bwd_apply dx closed " + nm, dx, rd.ref, rd.b16c))
        for mask8 in (None, d["mask8"]):
            ts, tq, gout = h_bwd_terms(x, g, bn, relu, mask8, defect)
            got = h_fold(h_partials(ts, tq, rows_how, defect), fold_how)
            sb = B.bwd_sums(x, g, bn, relu, nblk, 1, mask8)
            out.append(("bwd sums relu{}{}".format(relu, "" if mask8 is None else " masked"), got, sb.ref, sb.bound))
            if mask8 is not None:
                continue
            r2 = B.bwd_stage2(sb, float(P))
            h2 = h_bwd2(got[0], got[1], float(P), defect)
            for k in ("dgamma", "dbeta", "k12"):
                out.append(("bwd stage2 relu{} {}".format(relu, k), h2[k], getattr(r2, k), getattr(r2, "e_" + k)))
            for bf16 in (False, True):
                if bf16 and C % 4:
                    continue
                ro = B.bwd_apply_ref(x, g, bn, relu, r2.k12, r2.e_k12)
                dx = h_dx(x, g, bn, relu, h2["k12"], bf16, defect)
                out.append(("bwd oneshot dx relu{} {}".format(relu, "bf16" if bf16 else "f32"), dx, ro.ref,
                            ro.bound(bf16)))
    return out


def ratios(cid, grouping=GROUPINGS[0], defect=None):
    return {name: B.worst(got, ref, bound)[0] for name, got, ref, bound in checks(cid, grouping, defect)}


# ---------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------

def test_case_geometry():
    """The edge stated beside each case, recomputed."""
    g = {c: (B.row_geom(Cc, 4 if Cc % 4 == 0 else 1), B.bn_blocks(Pp, Cc)) for c, (Pp, Cc) in B.CASES.items()}
    assert g[1] == ((1, 1, 256), 2) and B.cdiv(8193, 2) == 4097 and B.bn_apply_blocks(8193, 4, 4) == 3
    assert g[2] == ((6, 6, 42), 3) and 256 - 6 * 42 == 4
    assert g[3] == ((16, 16, 16), 1)
    assert g[4][0][2] > 1 and g[5][0][2] > 3 and g[4][1] == g[5][1] == 1
    assert g[6] == ((128, 128, 2), 2) and B.cdiv(128, B.row_geom(512, 4, 32)[1]) == 4
    assert g[7] == ((256, 256, 1), 2) and B.cdiv(33, 2) == 17
    assert g[8] == ((257, 256, 1), 2)
    assert g[9] == ((3, 3, 85), 2) and 256 - 3 * 85 == 1
    assert g[10] == ((1, 1, 256), 2)
    assert g[11] == ((257, 256, 1), 2)
    assert g[12] == ((6, 6, 42), 1)
    assert B.row_geom(8, 1) == (8, 8, 32)       # case 13 on the scalar route
    # launch variants 4-7 of dk_bn_bwd_apply_f32 (8 rows per lane): several blocks on the multi-block cases
    assert B.bn_apply_blocks(8193, 4, 4, 8) == 5 and B.bn_apply_blocks(3219, 24, 4, 8) == 10
    assert B.fold_levels(256) == 1 and B.fold_levels(257) == 2 and B.fold_levels(65536) == 2
    assert B.fold_levels(65537) == 3 and B.fold_rows(65537) == 257 + 2 and B.fold_rows(513) == 3


@pytest.mark.parametrize("cid", CIDS)
def test_preconditions(cid):
    d = inputs(cid)
    assert d["P"] * d["C"] <= B.ELEMENT_CAP
    assert B.margin(d) > 1.0, "case {}: choose another seed".format(cid)
    assert (d["bn"][2] < 0).any() or d["C"] < 2
    for k in ("x", "dy", "g"):
        assert np.array_equal(d[k], B.bf16_values(d[k]))
    if d["C"] >= 4:
        assert (d["x"][:, 0] == 1.5).all() and (d["x"][:, 1] == 0).all() and d["m"][2] / d["s"][2] == 256.0


@pytest.mark.parametrize("cid", CIDS)
def test_reference_matches_oracle(cid):
    """Statistics, apply and backward chained in fp64 against oracle.ref's batch norm."""
    d = inputs(cid)
    x, g, P, C = d["x"], d["g"], d["P"], d["C"]
    gamma, beta = d["bn"][2].astype(np.float64), d["bn"][3].astype(np.float64)
    X, G = B.nchw(x), B.nchw(g)
    eps = float(B.BN_EPS)
    p4 = (lambda v: v[None, :, None, None])
    Y, cache, rm, rs = oref.bn_forward_train(X, p4(gamma), p4(beta), None, None, eps, float(B.MOMENTUM))
    s2 = B.stats_stage2(B.stats_sums(x, 1, 1), float(P), 1)
    tol = dict(rtol=1e-9, atol=1e-9)
    assert np.allclose(s2.mean, rm.ravel(), **tol) and np.allclose(s2.std, rs.ravel(), **tol)
    bn64 = (s2.mean, s2.invstd, gamma, beta)
    assert np.allclose(B.apply_ref(x, bn64, 0).ref, B.rows_(Y), **tol)
    s0 = B.stats_stage2(B.stats_sums(x, 1, 1), float(P), 0, d["run_mean0"], d["run_std0"])
    _, _, rm2, rs2 = oref.bn_forward_train(X, p4(gamma), p4(beta), p4(d["run_mean0"].astype(np.float64)),
                                           p4(d["run_std0"].astype(np.float64)), eps, float(B.MOMENTUM))
    om = float(f(1) - B.MOMENTUM)      # the oracle blends with 1 - momentum in fp64: |om - (1 - m)| <= 2^-25
    assert np.allclose(s0.run_mean, rm2.ravel(), rtol=1e-6, atol=1e-6) and om > 0
    assert np.allclose(s0.run_std, rs2.ravel(), rtol=1e-6, atol=1e-6)
    dX, dgamma, dbeta = oref.bn_backward(G, p4(gamma), cache)
    b2 = B.bwd_stage2(B.bwd_sums(x, g, bn64, 0, 1, 1), float(P))
    assert np.allclose(b2.dgamma, dgamma.ravel(), **tol) and np.allclose(b2.dbeta, dbeta.ravel(), **tol)
    assert np.allclose(B.bwd_apply_ref(x, g, bn64, 0, b2.k12).ref, B.rows_(dX), rtol=1e-9, atol=1e-8)


@pytest.mark.parametrize("grouping", GROUPINGS, ids=lambda gr: gr[0])
@pytest.mark.parametrize("cid", CIDS)
def test_honest_implementation_admitted(cid, grouping):
    for name, r in ratios(cid, grouping).items():
        assert r <= 1.0, (cid, name, r)


def test_fold_levels_admitted():
    """Synthetic rows through both fold orders and the three stage-2 modes at the fold-level edges."""
    for C, nblk in ((4, 1), (4, 257), (65, 513), (4, 65537)):
        part = B.synth_rows(nblk, C)
        sm = B.synth_sums(part, B.fold_levels(nblk))
        count = 7.0 * nblk
        for how in ("fold", "tree"):
            got = h_fold(part, how)
            assert B.worst(got, sm.ref, sm.bound)[0] <= 1.0
            r = B.stats_stage2(sm, count, 1)
            h = h_stats2(got[0], got[1], count, 1, None, None)
            for k in B.STATS_FIELDS:
                assert B.worst(h[k], getattr(r, k), getattr(r, "e_" + k))[0] <= 1.0, (C, nblk, how, k)
            r2, h2 = B.bwd_stage2(sm, count), h_bwd2(got[0], got[1], count)
            for k in ("dgamma", "dbeta", "k12"):
                assert B.worst(h2[k], getattr(r2, k), getattr(r2, "e_" + k))[0] <= 1.0, (C, nblk, how, k)
        raw = sm.Q / count - (sm.S / count) ** 2
        assert (raw[3::4] < 0).all() and (raw > 0).any()      # the clamp is met, and not everywhere


# defect -> (the checks it must fail, in one line what it is)
DEFECTS = {
    "drop_row": ("stats sums", "the last row of block 0's range dropped from the sums"),
    "double_row": ("stats sums", "that row counted twice"),
    "sample_var": ("stats first1 std", "sample variance, n / (n - 1)"),
    "eps_outside": ("stats first1 std", "sqrt(var) + eps"),
    "first_ignored": ("stats first1 run_mean", "first flag ignored (blend from the prefilled values)"),
    "momentum_swapped": ("stats first0 run_mean", "momentum on the new value"),
    "trunc_store": ("apply y relu0 bf16", "truncating bf16 store"),
    "mask_xhat": ("apply mask relu1 f32", "ReLU mask from x_hat > 0"),
    "k1_missing": ("bwd_apply dx relu0 f32", "k1 missing from dx"),
    "k2_undivided": ("bwd stage2 relu0 k12", "k2 not divided by count"),
    "std_for_invstd": ("bwd_apply dx relu0 f32", "x_hat formed with std in place of invstd"),
    "last_group": ("apply y relu0 f32", "last channel group never written"),
}
STD_KEY = "stats first1 std"


def std_normwise(x, defect):
    """Normwise error of a defective std against the reference on x[P][C] (what test_batchnorm_layer's "bn std" sees)."""
    P = float(x.shape[0])
    sm = B.stats_sums(x, 1, 1)
    h = h_stats2(sm.S, sm.Q, P, 1, None, None, defect)
    return rel_err(h["std"], B.stats_stage2(sm, P, 1).std)


def defect_report(cid=2):
    rep = {}
    for name, (key, _) in DEFECTS.items():
        for n, got, ref, bound in checks(cid, defect=name):
            if n == key:
                nw = rel_err(np.nan_to_num(np.asarray(got, dtype=np.float64), nan=0.0), ref)
                rep[name] = (B.worst(got, ref, bound)[0], nw)
    return rep


def test_defects_rejected():
    rep = defect_report()
    for name, (key, what) in DEFECTS.items():
        ratio, nw = rep[name]
        print("{:18s} {:40s} ratio {:10.3g}  normwise {:.2e}  {}".format(name, key, ratio, nw, what))
        assert ratio > 1.0, (name, ratio)
    # What a normwise 1e-4 lets through.  At case 2 every defect is above it, but not by construction:
    assert all(nw > OLD_TOL for _, nw in rep.values())
    # the sample variance is a relative 1 / (2 (P - 1)) on every std: within 1e-4 from P = 5002 on, so at case 1
    assert std_normwise(inputs(1)["x"], "sample_var") <= OLD_TOL < ratios(1, defect="sample_var")[STD_KEY]
    # sqrt(var) + eps differs by ~ eps in absolute terms: within 1e-4 wherever no channel's spread is near
    # sqrt(eps) -- on test_batchnorm_layer's own data (3 + 2.5 randn, P = 105, C = 16) it is 4e-6
    old = 3.0 + 2.5 * np.random.RandomState(9).randn(105, 16)
    assert std_normwise(B.bf16_values(old), "eps_outside") <= OLD_TOL


if __name__ == "__main__":      # the figures of the docstring
    tot = {}
    for c in CIDS:
        for gr in GROUPINGS:
            for n, r in ratios(c, gr).items():
                tot[n] = max(tot.get(n, 0.0), r)
    for n, r in tot.items():
        print("{:40s} {:.3f}".format(n, r))
    for name, (ratio, nw) in defect_report().items():
        print("{:18s} {:10.3g} ({:.1e})  {}".format(name, ratio, nw, DEFECTS[name][1]))
    print("sample_var at case 1: ratio {:.3g}, normwise {:.1e}".format(ratios(1, defect="sample_var")[STD_KEY],
                                                                      std_normwise(inputs(1)["x"], "sample_var")))
    old = 3.0 + 2.5 * np.random.RandomState(9).randn(105, 16)
    print("eps_outside on the layer test's data: normwise {:.1e}".format(std_normwise(B.bf16_values(old), "eps_outside")))
