"""fp64 reference of the stand-alone BatchNorm entry points (dorknet_amd/csrc/batchnorm.hip) and the per-element
error bounds they are held to (tests/test_bn_ref_host.py, tests/test_gpu_bn_elementwise.py).  Host only: numpy +
torch-CPU, nothing from dorknet_amd, no GPU call.  The pieces shared with the depthwise / pointwise references come
from tests/_dw_ref.py.

Operation (layers/batch_norm.py; oracle.ref.bn_forward_train / bn_backward), x[P][C], per channel c:
    S = sum_p x, Q = sum_p x^2;  mean = S / P;  var = max(Q / P - mean^2, 0);  std = sqrt(var + eps);
    invstd = 1 / std;  running = the value itself when `first`, else momentum * running + (1 - momentum) * value
    y  = gamma (x - mean) invstd + beta   (+ ReLU, mask = y > 0)
    S' = sum_p g_e, Q' = sum_p g_e x_hat with g_e = g (y > 0 under a fused ReLU);  dgamma = Q', dbeta = S',
    k1 = S' / P, k2 = Q' / P;  dx = gamma invstd (g_e - k1 - x_hat k2)

Bounds on |got - ref|, u = 2^-24, e = 2^-53, none fitted to an output and no element excluded.

Partial sums and their folds (batchnorm.hip:65-123 bn_stats_partial_kernel, :349-448 bn_bwd_partial_kernel, :126-146
block_sum2, :203-281 bn_fold_kernel).  Every term is widened to fp64 before it is squared or multiplied (:91-93,
:386-387): squares and products of fp32 / bf16 values are exact in fp64 (at most 48 significant bits).  The terms are
then added in fp64 only: in a thread (:88-103), over the pixel lanes (:120), over the partial rows (:130-143 or
:221-238) and over the fold levels (:779-786).  A sum of n terms in ANY grouping is within (n - 1) e sum|term| of the
exact sum to first order; with `rows` partial rows and `levels` fold launches the count used here is
    K = n + rows + levels + 2       ->       |S_got - S| <= e K sum|term|                                   (sum_bound)
(rows and levels are spare: they are already inside n - 1 additions; + 2 holds the second-order terms and, for
g x_hat, the one fp64 rounding of each product).  For sum g x_hat the factor x_hat = (x - mean) * invstd is formed in
fp32 (:384, two roundings: relative error XH = 2 u (1 + u)) and then widened: + XH sum|g x_hat|.

Statistics stage 2 (fold_tail.h:39-57 bn_finalize_channel; batchnorm.hip:161-177 bn_stats_finalize_kernel: the same
lines).  The reference takes eps, momentum and om = fl32(1 - momentum) as the fp32 values the kernel has.  With
eS, eQ the bounds on the two sums, Sa = sum|s term|, Qa = sum|q term| (= Q for squares), n = count:
    mean_d = fl64(S_got / n):      em = (eS / n) (1 + e) + e |mean|
    mean   = fl32(mean_d):         e_mean = u |mean| + (1 + u) em
    var_d  = fl64(fl64(Q_got / n) - fl64(mean_d^2)): each of the three operations rounds a value of at most
             Qa / n + mean^2 (+ errors): the cancellation enters as 3 e (Qa / n + mean^2) -- two roundings on the
             operands, one on the difference, the third e also holding the second-order terms -- plus the propagated
             (1 + 3 e) (eQ / n + 2 |mean| em + em^2).  Together ev.  The clamp max(., 0) is 1-Lipschitz and leaves
             the reference (>= 0) where it is, so ev holds after it (fold_tail.h:43).
    (float) var:                   ev1 = ev + u (var + ev)
    (float) var + eps in fp32:     ew  = ev1 + u (var + eps + ev1),  w = var + eps
    sqrtf (correctly rounded: hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt, __graft_entry__.py:21 adds no
    fast-math flag):               the argument lies in [w - ew, w + ew], sqrt is monotone, so the exact root is within
             iv = max(sqrt(w + ew) - sqrt(w), sqrt(w) - sqrt(max(w - ew, 0))) of std -- an interval, not ew / (2 std):
             a constant channel (w = eps) stays finite and tight -- and e_std = iv + u (std + iv)
    invstd = 1.0f / std (one rounding, fold_tail.h:48):  e_inv = d + u (1 / std + d),  d = e_std / (std (std - e_std))
    running, first:                a copy: the bound of mean / std
    running, blend (fold_tail.h:54-55): two products and a sum in fp32 (or a product and an fma: fewer roundings),
             e_run = |om| e_val (1 + 2 u) + 2 u (|momentum run0| + |om val|)

Apply (batchnorm.hip:286-340, bn_out dk_common.h:180-183): _dw_ref.bn_operand's ea = 4 u (|gamma x_hat| + |beta|) from
the fp32 parameters given (three roundings on gamma x_hat, one on the sum; an fma has fewer).  Under ReLU the bound
is 0 wherever the reference is not positive: those outputs must be exactly 0 (batchnorm.hip:317-318), and the mask byte
exactly the reference decision (:319, :326-328).  bf16 stores (dk_common.h:67-72, :95-100) are one round-to-nearest-
even of a value within ea: _dw_ref.bf16_bound(ref, ea), the closed form bf16_closed recorded next to it.

Backward stage 2 (fold_tail.h:58-62; batchnorm.hip:460-470): dgamma = (float) Q', dbeta = (float) S',
k1 = (float)(S' / n), k2 = (float)(Q' / n): one fp32 rounding each, plus the propagated sum bound (for k1, k2 through
the fp64 division: (eS / n)(1 + e) + e |k1|).

Backward apply (batchnorm.hip:476-533, bn_bwd_elem dk_common.h:193-197): _dw_ref.bn_bwd_dy's
ed = 6 u |gamma invstd| (|g_e| + |k1| + |x_hat k2|) with k12 as given (f = gamma * invstd, g - k1, x_hat (2), the fma,
the product: five roundings on each term at most, one spare for the second order).  The one-shot dk_bn_bwd_* computes
k12 itself: + |gamma invstd| (e_k1 + |x_hat| e_k2).  bf16: bf16_bound.

ReLU decisions: the seed of each case (SEEDS) is the first at which mask_margin > 1 for every element, so no fp32
evaluation of bn_out can decide a mask differently from fp64; tests/test_bn_ref_host.py asserts it.

Inputs (make_inputs): x, dy, g bf16-representable, so both storage types see the same values.  Channel c of x is
m_c + s_c randn; where C >= 4 channel 0 is constant (1.5), channel 1 all zero and channel 2 has |m_c| / s_c = 2^8
(64, 0.25).  mean, invstd, gamma (every third negative), beta and k12 of the apply / backward checks are arbitrary
fp32, not the statistics of x: each kernel is pinned on its own."""
import numpy as np

from tests._dw_ref import (U, UB, bf16_bound, bf16_closed, bf16_values, bn_bwd_dy, bn_operand,  # noqa: F401
                           mask_margin, rne_bf16, worst)
from tests._dw_ref import check as _check

EPS = 2.0 ** -53
XH = 2 * U * (1 + U)     # relative error of x_hat = (x - mean) * invstd formed in fp32
f32 = np.float32

BN_EPS = f32(1e-5)
MOMENTUM = f32(0.95)
ELEMENT_CAP = 80000      # no case holds more elements than this (the largest is case 2: 77,256)


def check(name, got, ref, bound):
    return _check(name, got, ref, bound, tag="bn")


def cdiv(a, b):
    return -(-a // b)


# (P rows, C channels): each the smallest shape reaching the named edge.  The figures follow from row_geom, bn_blocks
# and bn_apply_blocks below (batchnorm.hip:54-60, :543-550, :558-564) and are recomputed by tests/test_bn_ref_host.py.
CASES = {
    1: (8193, 4),      # one channel group, PL = 256; 2 reduce blocks (ppb 4097), 3 apply blocks; unrolled loop + remainder
    2: (3219, 24),     # cgt = 6, PL = 42: four idle threads; 3 reduce blocks
    3: (429, 64),      # one block, 16 lanes, unrolled loop + remainder
    4: (1, 64),        # fewer rows than lanes
    5: (3, 64),        # fewer rows than lanes
    6: (98, 512),      # res8 geometry, PL = 2; dk_relu_bwd_bn_partial_*'s 32-group cap gives 4 channel slices
    7: (33, 1024),     # PL = 1, 2 reduce blocks (17 + 16 rows: four trips + one remainder row)
    8: (33, 1028),     # second channel slice with one live group
    9: (2731, 3),      # scalar route, PL = 85 (one idle thread), 2 blocks
    10: (8193, 1),     # scalar, single channel
    11: (33, 257),     # scalar, two channel slices
    12: (5, 6),        # dense-head [rows][features]
    13: (429, 8),      # every pointer offset by one element: scalar route at C % 4 == 0 (fp32 only)
}
OFFSET_CASE = 13
BF16_CASES = [c for c in sorted(CASES) if CASES[c][1] % 4 == 0 and c != OFFSET_CASE]
SCALAR_CASES = [c for c in sorted(CASES) if CASES[c][1] % 4]

# The seed of each case: the first of 0, 1, 2, ... at which mask_margin > 1 holds (tests/test_bn_ref_host.py).
SEEDS = {}


def row_geom(C, V, cap=256):
    """(CG, cgt, PL) of the row loop (batchnorm.hip:54-60)."""
    CG = C // V
    cgt = min(CG, cap)
    return CG, cgt, 256 // cgt


def bn_blocks(P, C):
    """Partial rows of the reduce passes (batchnorm.hip:543-550)."""
    PL = row_geom(C, 4 if C % 4 == 0 else 1)[2]
    return min(max(cdiv(P, PL * 32), 1), 1024)


def bn_apply_blocks(P, C, V, rows_per_lane=16, cap=4096):
    """Blocks of the streaming passes (batchnorm.hip:558-564; :956-960 for the launch variants)."""
    PL = row_geom(C, V)[2]
    return min(max(cdiv(P, PL * rows_per_lane), 1), cap)


def fold_levels(nblk):
    """Launches fold_finalize needs without tickets (batchnorm.hip:779-786)."""
    lv = 1
    while nblk > 256:
        nblk = cdiv(nblk, 256)
        lv += 1
    return lv


def fold_rows(nblk):
    """Rows of fold workspace (dk_bn_partials_workspace_bytes, batchnorm.hip:650-655)."""
    rows, n = 0, nblk
    while n > 256:
        n = cdiv(n, 256)
        rows += n
    return max(rows, 1)


def nchw(a):
    """[P][C] -> (1, C, P, 1) for the helpers of tests/_dw_ref.py."""
    return np.asarray(a).T[None, :, :, None]


def rows_(a):
    """(1, C, P, 1) -> [P][C]."""
    return a[0, :, :, 0].T


def make_inputs(cid):
    """Fixed inputs of case cid: x, dy, g [P][C] fp64 arrays of bf16-representable values; bn = (mean, invstd, gamma,
    beta) and k12 arbitrary fp32; mask8 the uint8 mask of a preceding join; run_mean0 / run_std0 the running values a
    blend starts from."""
    P, C = CASES[cid]
    rng = np.random.RandomState(11000 + 100 * cid + SEEDS.get(cid, 0))
    m = 2.0 * rng.randn(C)
    s = 0.25 + 2.0 * rng.rand(C)
    if C >= 4:
        m[:3] = (1.5, 0.0, 64.0)
        s[:3] = (0.0, 0.0, 0.25)
    d = dict(P=P, C=C, m=m, s=s)
    d["x"] = bf16_values(m[None, :] + s[None, :] * rng.randn(P, C))
    d["dy"] = bf16_values(rng.randn(P, C))
    d["g"] = bf16_values(rng.randn(P, C))
    gamma = 1 + 0.3 * rng.randn(C)
    gamma[::3] *= -1.0
    d["bn"] = tuple(v.astype(f32) for v in (rng.randn(C) * 0.3, rng.rand(C) + 0.5, gamma, 0.2 * rng.randn(C)))
    d["k12"] = (rng.randn(2 * C) * 0.1).astype(f32)
    d["mask8"] = (rng.rand(P, C) < 0.6).astype(np.uint8)
    d["run_mean0"] = rng.randn(C).astype(f32)
    d["run_std0"] = (rng.rand(C) + 0.5).astype(f32)
    return d


def margin(d):
    return mask_margin(nchw(d["x"]), d["bn"])


def _sumx(a):
    """Column sums in extended precision."""
    return np.asarray(a, dtype=np.longdouble).sum(axis=0)


def _sum(a):
    """Column sums in extended precision, rounded once to fp64."""
    return _sumx(a).astype(np.float64)


def sum_bound(n, rows, levels, abs_sum):
    return EPS * (n + rows + levels + 2) * abs_sum


class Sums:
    """Exact column sums of the s and q terms ([n][C] each), their absolute twins and bounds."""

    def __init__(self, s_terms, q_terms, rows, levels, q_rel=0.0):
        n = s_terms.shape[0]
        self.n = n
        self.Sx, self.Qx = _sumx(s_terms), _sumx(q_terms)       # kept in extended precision for stage 2
        self.S, self.Q = self.Sx.astype(np.float64), self.Qx.astype(np.float64)
        self.Sa, self.Qa = _sum(np.abs(s_terms)), _sum(np.abs(q_terms))
        self.eS = sum_bound(n, rows, levels, self.Sa)
        self.eQ = sum_bound(n, rows, levels, self.Qa) + q_rel * self.Qa

    @property
    def ref(self):
        return np.stack([self.S, self.Q])

    @property
    def bound(self):
        return np.stack([self.eS, self.eQ])


def stats_sums(x, rows, levels):
    """sum x, sum x^2 of x[P][C]."""
    return Sums(x, x * x, rows, levels)


def bwd_terms(x, g, bn, relu, mask8=None):
    """(g_e, g_e x_hat): the backward reduce's terms, fp64 from the fp32 parameters."""
    m, i, ga, be = (np.asarray(v, dtype=np.float64)[None, :] for v in bn[:4])
    xh = (x - m) * i
    ge = g if mask8 is None else g * (mask8 != 0)
    if relu:
        ge = ge * (ga * xh + be > 0)
    return ge, ge * xh


def bwd_sums(x, g, bn, relu, rows, levels, mask8=None):
    ge, gx = bwd_terms(x, g, bn, relu, mask8)
    return Sums(ge, gx, rows, levels, q_rel=XH)


class Stage2:
    """Forward statistics from sums: mean, std, invstd, run_mean, run_std and e_<name> their bounds."""


def stats_stage2(sm, count, first, run_mean0=None, run_std0=None, eps=BN_EPS, momentum=MOMENTUM):
    eps, mom = float(f32(eps)), float(f32(momentum))
    om = float(f32(1.0) - f32(momentum))
    o = Stage2()
    mean = sm.S / count
    em = (sm.eS / count) * (1 + EPS) + EPS * np.abs(mean)
    o.mean, o.e_mean = mean, U * np.abs(mean) + (1 + U) * em
    meanx = sm.Sx / count
    var = np.maximum((sm.Qx / count - meanx * meanx).astype(np.float64), 0.0)   # the cancellation in extended precision
    ev = 3 * EPS * (sm.Qa / count + mean * mean) + (1 + 3 * EPS) * (sm.eQ / count + 2 * np.abs(mean) * em + em * em)
    ev1 = ev + U * (var + ev)
    w = var + eps
    ew = ev1 + U * (w + ev1)
    std = np.sqrt(w)
    iv = np.maximum(np.sqrt(w + ew) - std, std - np.sqrt(np.maximum(w - ew, 0.0)))
    o.var, o.std, o.e_std = var, std, iv + U * (std + iv)
    dinv = o.e_std / (std * (std - o.e_std))
    o.invstd, o.e_invstd = 1.0 / std, dinv + U * (1.0 / std + dinv)
    if first:
        o.run_mean, o.e_run_mean, o.run_std, o.e_run_std = o.mean, o.e_mean, o.std, o.e_std
    else:
        r0m, r0s = np.asarray(run_mean0, dtype=np.float64), np.asarray(run_std0, dtype=np.float64)
        o.run_mean = mom * r0m + om * mean
        o.e_run_mean = om * o.e_mean * (1 + 2 * U) + 2 * U * (np.abs(mom * r0m) + np.abs(om * mean))
        o.run_std = mom * r0s + om * std
        o.e_run_std = om * o.e_std * (1 + 2 * U) + 2 * U * (np.abs(mom * r0s) + np.abs(om * std))
    return o


STATS_FIELDS = ("mean", "std", "invstd", "run_mean", "run_std")


class BwdStage2:
    """dgamma, dbeta, k12 ([2 C]) and their bounds from the local / global sums."""


def bwd_stage2(sm_local, count, sm_global=None):
    g = sm_local if sm_global is None else sm_global
    o = BwdStage2()
    o.dgamma, o.e_dgamma = sm_local.Q, U * np.abs(sm_local.Q) + (1 + U) * sm_local.eQ
    o.dbeta, o.e_dbeta = sm_local.S, U * np.abs(sm_local.S) + (1 + U) * sm_local.eS
    k1, k2 = g.S / count, g.Q / count
    e1 = (g.eS / count) * (1 + EPS) + EPS * np.abs(k1)
    e2 = (g.eQ / count) * (1 + EPS) + EPS * np.abs(k2)
    o.k1, o.k2 = k1, k2
    o.e_k1, o.e_k2 = U * np.abs(k1) + (1 + U) * e1, U * np.abs(k2) + (1 + U) * e2
    o.k12, o.e_k12 = np.concatenate([k1, k2]), np.concatenate([o.e_k1, o.e_k2])
    return o


class Out:
    """An activation-sized result: ref, A (the fp32 bound / the bf16 store's A), b16 / b16c the bf16 bounds."""

    def __init__(self, ref, A):
        self.ref, self.A = ref, A
        self.b16, self.b16c = bf16_bound(ref, A), bf16_closed(ref, A)

    def bound(self, bf16):
        return self.b16 if bf16 else self.A


def apply_ref(x, bn, relu):
    """y of dk_bn_apply_* and the ReLU mask ([P][C])."""
    a, ea, pre = bn_operand(nchw(x), (*bn, relu))
    a, ea, pre = rows_(a), rows_(ea), rows_(pre)
    if relu:
        ea = np.where(pre > 0, ea, 0.0)
    o = Out(a, ea)
    o.mask = (pre > 0).astype(np.uint8) if relu else np.zeros(pre.shape, dtype=np.uint8)
    return o


def bwd_apply_ref(x, g, bn, relu, k12, e_k12=None):
    """dx of dk_bn_bwd_apply_* (k12 given) or of the one-shot (k12 the exact coefficients, e_k12 their bounds)."""
    dy, ed, _ = bn_bwd_dy(nchw(g), nchw(x), (*bn, relu), k12)
    dy, ed = rows_(dy), rows_(ed)
    if e_k12 is not None:
        C = x.shape[1]
        m, i, ga = (np.asarray(v, dtype=np.float64)[None, :] for v in bn[:3])
        xh = (x - m) * i
        ed = ed + np.abs(ga * i) * (e_k12[:C][None, :] + np.abs(xh) * e_k12[C:][None, :])
    return Out(dy, ed)


def synth_rows(nblk, C, seed=0):
    """part[nblk][2][C] fp64 of mixed sign and magnitude (magnitudes up to 1e3, over six decades); the q rows are
    positive four times in five, in every fourth channel negative four times in five: most channels have a positive
    variance and those meet the clamp."""
    rng = np.random.RandomState(13000 + 7 * nblk + C + seed)
    mag = 10.0 ** rng.uniform(-3, 3, size=(nblk, 2, C))
    sign = np.where(rng.rand(nblk, 2, C) < 0.5, -1.0, 1.0)
    sign[:, 1, :] = np.where(rng.rand(nblk, C) < 0.8, 1.0, -1.0)
    sign[:, 1, 3::4] *= -1.0
    return mag * sign * rng.rand(nblk, 2, C)


def synth_sums(part, levels):
    """The Sums of synthetic rows: n = the rows themselves."""
    return Sums(part[:, 0, :], part[:, 1, :], 0, levels)
