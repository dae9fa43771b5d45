"""fp64 reference of a pointwise (1x1) layer and the per-element error bounds its fp32 / bf16 kernels are
held to (tests/test_pw_ref_host.py, tests/test_gpu_pw_elementwise.py).  Host only: numpy + torch-CPU, nothing
from dorknet_amd, no GPU call.  The pieces shared with the depthwise reference come from tests/_dw_ref.py.

Operation (layers/pointwise_convolution.py; oracle.ref.pointwise_forward / _backward), rows m = pixels
(n, oh, ow), OH = ceil(H / stride):
    a  = bn(x) (+ ReLU) where an input BatchNorm is applied on load, else x, sampled at (stride oh, stride ow)
    y[m, k]  = sum_c a[m, c] w[k, c] + bias[k]
    dx[m, c] = sum_k dy[m, k] w[k, c] (+ residual); for stride > 1 widened to (stride OH, stride OW) with
               exact zeros (or exact copies of the residual) off the lattice; the lattice entry points keep
               dx compact
    dw[k, c] = sum_m dy[m, k] a[m, c] + l2 w[k, c]
    stats[rows][2][K] = (sum_m y, sum_m y^2) of the STORED y over the rows the call wrote
    part[rows][2][C]  = (sum_m g, sum_m g x_hat) of the input BatchNorm's backward
What the epilogues do for the partials (gemm_engine.h bn_bwd_contrib, EpStoreBnBwdT / EpWidenBnBwdT /
EpLatticeBnBwd; pw_stream.hip:241-248; pw_stream_bf16.hip:386-390, :608-615; pw_deep.hip:420-431, :626-630,
:829-834, :1043-1048; pw_deep_bf16.hip:378-386, :543-548; pw_bwd_fused.hip:223-231) -- every route alike:
    * g is the value the launch stores as dx: it INCLUDES the residual addend;
    * for bf16 storage it is the ROUNDED stored dx (widened back to fp32);
    * the ReLU mask is bn_out(x) > 0 recomputed in fp32 from the raw x (pw_deep.hip:427 lets the compiler
      contract gamma x_hat + beta; mask_margin's guard of 8 u covers either form);
    * x_hat = (x - mean) * invstd is formed in fp32 (two roundings: relative error XH = 2 u (1 + u)), then
      g and x_hat are widened and multiplied and accumulated in fp64.
No route differs in any of the three.

Absolute twins (the scale of the rounding error of any evaluation order):
    ya = |a| |w|^T + |bias|,  dxa = |dy| |w| + |res|,  dwa = |dy|^T |a|.

Bounds on |got - ref| per element, none excluded (u = 2^-24):
    fp32 y, dx   A = 2 u (C_red + 3) twin + E.  C_red: the reduction length; E = e |w| the operand's own error
                 scale carried through |w| (ea from bn_operand, ed from bn_bwd_dy, 0 for exact operands).
                 ASSUMPTION: one ulp (2 u) per accumulation step.  Neither the repository nor its guides
                 say how v_mfma_f32_32x32x2_f32 and v_mfma_f32_32x32x16_bf16 round inside an instruction
                 (the depthwise VALU arithmetic is held to u per step); one ulp per step is what any
                 faithful implementation satisfies in any order.  The constant has not been changed on
                 any kernel output.
    fp32 dw      2 u (M + 2) dwa + 2 u |ref| + sum |dy| ea + sum ed |a|,  M = N OH OW terms in any grouping
                 (split-K slabs, per-block partial rows and their fixed-order reduce).
    bf16 storage the operands are bf16 MFMA operands (pw_stream_bf16.hip:15-19, tests/_bf16_resblock_twin.py).
                 The reference uses wq = rne_bf16(w) EXACTLY in y and dx (the rounding of a given fp32 weight
                 is unambiguous); raw bf16 activations and a raw bf16 dy are exact; an operand formed on
                 load (the BatchNorm output; dy of the *_bnbwd_* entry points) is a bf16 rounding of an
                 fp32 value within e of the fp64 value, error scale 2^-8 (|v| + e) + e (operand_err).  A
                 is as above with the reduction in fp32; the store is held to bf16_bound(ref, A) and to
                 bf16_closed.
                 Weight gradient (gemm_bf16.hip:138-165 split-K on kMfBf16; pw_stream_bf16.hip
                 bwd_fused_kernel and pw_deep_bf16.hip pw_deep16_bwd_fused): both operands are activations
                 -- dy (raw bf16: exact; formed on load: rounded as the dgrad rounds it) and a (raw: exact;
                 BatchNorm on load: rounded) -- the weights do not enter except in l2 w, which uses the
                 fp32 w.  dw is fp32, bound as the fp32 one with the rounded operands' scales.
    dy_out       written through by *_dgrad_bnbwd_*: ed (fp32), bf16_bound(dy, ed) (bf16).  Where it is stored
                 the second check holds dx to dgrad(dy_out as stored, w or wq) with E = 0: the MFMA operand
                 is the stored value, so this pins the GEMM without the 2^-8 operand slack.
    stats, part  (1) against fp64 sums of what the same call stored: 2^-53 (M + rows + 2) sum |term| (squares
                 of fp32 / bf16 values are exact in fp64), for g x_hat plus XH sum |g x_hat|;
                 (2) against the fp64 reference sums: the summed per-element bounds (+ the same terms).

ReLU masks: the inputs are chosen (SEEDS) so that mask_margin > 1 for both BatchNorms of every case;
tests/test_pw_ref_host.py asserts it.

Inputs (make_inputs): activations, dy, g and res are bf16-representable, so the fp32 and the bf16 entry points see
the same values; w = randn(K, C) / sqrt(C) in fp32 (not bf16-representable); bias, BatchNorm vectors and k12
arbitrary fp32.  One seed per case."""
import numpy as np

from tests._dw_ref import (U, UB, bf16_bound, bf16_closed, bf16_values, bn_bwd_dy, bn_operand,  # noqa: F401
                           bn_operand_f32, bn_params, mask_margin, rne_bf16, worst)
from tests._dw_ref import check as _check

EPS = 2.0 ** -53
XH = 2 * U * (1 + U)     # relative error of x_hat = (x - mean) * invstd formed in fp32
STEP = 2 * U             # per accumulation step of an MFMA: one ulp (module docstring; not fitted)


def check(name, got, ref, bound):
    return _check(name, got, ref, bound, tag="pw")


# (K, C, stride, N, H, W): each the smallest shape reaching the named edge.  Routing under default knobs; with
# knobs 3, 9, 11, 13, 14 off every case runs the tiled engine (gemm_engine.h) and the tiled fused backward.
#   fp32 forward: streaming K = C = 64; deep where K % 128 == 0 and C in {64 .. 512}; else tiled
#   fp32 dgrad_bnbwd: streaming K = C = 64; deep where C % 128 == 0; else tiled.  dgrad_ex / lattice / wgrad: tiled
#   fp32 fused backward: streaming K = C = 64; deep K in {128, 256}; tiled fused (K, C) = (64, 128); else refused
#   bf16 forward / dgrad_bnbwd: streaming K, C in {64, 128} (stride 1); deep16 with 256+ on one side; else tiled
#   bf16 fused backward: streaming K = C = 64; deep16 K in {128, 256}; else refused
CASES = {
    1: (64, 64, 1, 3, 13, 11),      # streaming kernels; 429 pixels: ragged for 32-, 64- and 128-pixel tiles
    2: (64, 64, 1, 1, 1, 5),        # the same kernels on a single partial tile
    3: (64, 64, 2, 2, 13, 9),       # stride 2, odd H and W: the streaming forward gathers; lattice forms
    4: (128, 64, 1, 3, 13, 11),     # fp32 deep forward and fused deep backward, tiled dgrad; bf16 streaming
    5: (128, 64, 1, 1, 1, 33),      # one full 32-pixel tile plus one pixel
    6: (64, 128, 1, 3, 13, 11),     # fp32 tiled forward, deep dgrad, tiled fused backward; bf16 streaming
    7: (64, 128, 2, 2, 13, 9),      # the same at stride 2: tiled forward in both types
    8: (128, 128, 1, 3, 13, 11),    # fp32 deep everywhere (ahead of the streaming forward); bf16 streaming
    9: (128, 128, 1, 2, 8, 8),      # exactly two 64-pixel tiles, no ragged edge
    10: (256, 128, 1, 3, 13, 11),   # deep, the fused deep backward's 16 x 16 kernel (K = 256); bf16 deep16
    11: (256, 128, 1, 1, 1, 33),
    12: (256, 256, 1, 3, 13, 11),   # deep, fused deep backward
    13: (256, 256, 2, 2, 13, 9),    # the strided deep forward (a downsampling block's skip projection)
    14: (128, 512, 1, 3, 13, 11),   # deep, longest forward reduction (C = 512), one wave per SIMD
    15: (128, 512, 1, 1, 1, 5),
    16: (512, 256, 1, 3, 13, 11),   # deep, longest dgrad reduction (K = 512); no fused backward
    17: (512, 256, 1, 2, 8, 8),
    18: (24, 40, 1, 3, 13, 11),     # tiled engine, K and C no multiples of 32 (bf16: C no multiple of a k-step)
    19: (24, 40, 2, 2, 13, 9),
    20: (16, 3, 1, 3, 13, 11),      # C % 4 != 0: scalar loaders of the plain entry points; the others refuse
    21: (16, 3, 1, 1, 1, 33),
    22: (16, 3, 2, 2, 13, 9),       # the scalar loaders under the widening and the lattice epilogues
    23: (132, 6, 1, 2, 9, 9),       # ... and with a reduction past 128 (the deeper k-tile), 162 pixels
    24: (132, 6, 2, 2, 13, 9),
    25: (512, 512, 2, 2, 9, 9),     # bf16 strided forward on the tiled engine's 128 x 128, 8-wave tile; 50 pixels
}

# The seed of each case: the first of 0, 1, 2, ... at which mask_margin > 1 holds for the input BatchNorm (on x
# and xg) and the following one (on x1) -- a precondition on the inputs, asserted by tests/test_pw_ref_host.py.
SEEDS = {}


def out_hw(H, W, stride):
    return -(-H // stride), -(-W // stride)


def rows(a):
    """(N, C, H, W) -> (N H W, C)."""
    return a.transpose(0, 2, 3, 1).reshape(-1, a.shape[1])


def unrows(r, N, H, W):
    return r.reshape(N, H, W, -1).transpose(0, 3, 1, 2)


def sample(a, stride):
    return a[:, :, ::stride, ::stride]


def widen(d, stride):
    """The compact (N, C, OH, OW) gradient on the (stride OH, stride OW) grid, zeros off the lattice."""
    if stride == 1:
        return d.copy()
    N, C, OH, OW = d.shape
    wide = np.zeros((N, C, OH * stride, OW * stride))
    wide[:, :, ::stride, ::stride] = d
    return wide


def make_inputs(cid):
    """Fixed inputs of case cid (fp64 arrays of bf16-representable values; fp32 parameters):
    x (N,C,H,W) the layer input; xg the input BatchNorm's raw input on the widened gradient grid
    (N,C,stride OH,stride OW) (x itself where the shapes agree); dy, g, x1 (N,K,OH,OW) the output gradient,
    the following BatchNorm's gradient and raw input; res on the widened grid; w, bias; pi / po the input /
    following BatchNorm's (mean, invstd, gamma, beta); k12 the folded backward coefficients."""
    K, C, stride, N, H, W = CASES[cid]
    rng = np.random.RandomState(9000 + 100 * cid + SEEDS.get(cid, 0))
    OH, OW = out_hw(H, W, stride)
    d = dict(K=K, C=C, stride=stride, N=N, H=H, W=W, OH=OH, OW=OW, M=N * OH * OW)
    d["x"] = bf16_values(rng.randn(N, C, H, W))
    d["xg"] = d["x"] if (OH * stride, OW * stride) == (H, W) else bf16_values(rng.randn(N, C, OH * stride, OW * stride))
    for k in ("dy", "g", "x1"):
        d[k] = bf16_values(rng.randn(N, K, OH, OW))
    d["res"] = bf16_values(rng.randn(N, C, OH * stride, OW * stride))
    d["w"] = (rng.randn(K, C) / np.sqrt(C)).astype(np.float32)
    d["bias"] = rng.randn(K).astype(np.float32)
    d["pi"] = bn_params(C, rng)
    d["po"] = bn_params(K, rng)
    d["k12"] = (rng.randn(2 * K) * 0.1).astype(np.float32)
    return d


def margins(d):
    """The mask_margin of every ReLU decision a test of this case can make."""
    return min(mask_margin(d["x"], d["pi"]), mask_margin(d["xg"], d["pi"]), mask_margin(d["x1"], d["po"]))


def operand_err(v, e, formed16):
    """Error scale of an MFMA operand: e for fp32; for bf16 storage an operand formed on load is a bf16
    rounding of an fp32 value within e of v."""
    return UB * (np.abs(v) + e) + e if formed16 else e


def weights(w, bf16):
    """The weights as the GEMM uses them, fp64: w, or rne_bf16(w) exactly."""
    return bf16_values(w) if bf16 else np.asarray(w, dtype=np.float64)


class Ref:
    """Results and bounds of one call: ref, A (the fp32-storage bound, or the bf16 store's A), b16 / b16c the
    bf16-storage bounds (interval / closed form)."""

    def __init__(self, ref, A):
        self.ref, self.A = ref, A
        self.b16, self.b16c = bf16_bound(ref, A), bf16_closed(ref, A)

    def bound(self, bf16):
        return self.b16 if bf16 else self.A


def forward(x, w, stride, bias=None, bn=None, bf16=False):
    """y and its bounds.  bn = (mean, invstd, gamma, beta, relu) or None.  Also .a / .ea: the sampled operand
    and its error scale as the MFMA sees it."""
    a, ea, _ = bn_operand(x, bn)
    a, ea = sample(a, stride), sample(ea, stride)
    ea = operand_err(a, ea, bf16 and bn is not None)
    wq = weights(w, bf16)
    N, C, OH, OW = a.shape
    ar = rows(a)
    y, ya = ar @ wq.T, np.abs(ar) @ np.abs(wq).T
    if bias is not None:
        b64 = np.asarray(bias, dtype=np.float64)
        y, ya = y + b64, ya + np.abs(b64)
    A = STEP * (C + 3) * ya + rows(ea) @ np.abs(wq).T
    o = Ref(unrows(y, N, OH, OW), unrows(A, N, OH, OW))
    o.a, o.ea = a, ea
    return o


def dgrad(dy, w, stride, res=None, ed=None, bf16=False, formed=False, lattice=False):
    """dx and its bounds.  dy (N,K,OH,OW) fp64; ed its fp32 error scale where it is formed on load (formed:
    and, for bf16 storage, rounded to a bf16 operand); res on the widened grid; lattice: dx kept compact."""
    N, K, OH, OW = dy.shape
    wq = weights(w, bf16)
    dr = rows(dy)
    e = np.zeros_like(dr) if ed is None else rows(ed)
    e = operand_err(dr, e, bf16 and formed)
    dx = unrows(dr @ wq, N, OH, OW)
    A = unrows(STEP * (K + 3) * (np.abs(dr) @ np.abs(wq)) + e @ np.abs(wq), N, OH, OW)
    if lattice:
        assert res is None
        return Ref(dx, A)
    dx, A = widen(dx, stride), widen(A, stride)
    if res is not None:
        dx = dx + res
        on = widen(np.ones((N, 1, OH, OW)), stride)
        A = A + STEP * (K + 3) * np.abs(res) * on     # off the lattice the residual is copied: exact
    return Ref(dx, A)


def wgrad(dy, a, w, l2=0.0, ed=None, ea=None):
    """dw and its bound.  dy (N,K,OH,OW) and the sampled operand a (N,C,OH,OW) with their error scales as the
    MFMA sees them (forward().a / .ea; operand_err for dy)."""
    dr, ar = rows(dy), rows(a)
    M = dr.shape[0]
    dw = dr.T @ ar + l2 * np.asarray(w, dtype=np.float64)
    b = STEP * (M + 2) * (np.abs(dr).T @ np.abs(ar)) + STEP * np.abs(dw)
    if ea is not None:
        b = b + np.abs(dr).T @ rows(ea)
    if ed is not None:
        b = b + rows(ed).T @ np.abs(ar)
    return Ref(dw, b)


def _sum(a):
    """Column sums in extended precision, rounded once to fp64."""
    return np.asarray(a, dtype=np.longdouble).sum(axis=0).astype(np.float64)


def stats_checks(name, stats, stored, ref, bound, check=check):
    """stats[rows][2][K] against (1) the fp64 sums of the stored y and (2) the fp64 reference sums.
    stored / ref / bound: (N,K,OH,OW).  check: the family's check (its log tag; tests/_conv_ref.py passes its own)."""
    stats = np.asarray(stats, dtype=np.float64)
    assert not np.isnan(stats).any(), "{}: partial rows never written".format(name)
    got = _sum(stats)
    s, r, b = rows(np.asarray(stored, dtype=np.float64)), rows(ref), rows(bound)
    acc = EPS * (s.shape[0] + stats.shape[0] + 2)
    check(name + " sum|stored", got[0], _sum(s), acc * _sum(np.abs(s)))
    check(name + " sq|stored", got[1], _sum(s * s), acc * _sum(s * s))
    check(name + " sum|ref", got[0], _sum(r), _sum(b) + acc * _sum(np.abs(r)))
    check(name + " sq|ref", got[1], _sum(r * r), _sum(b * (2 * np.abs(r) + b)) + acc * _sum(r * r))


def part_checks(name, part, stored, xl, bn, ref, bound):
    """part[rows][2][C] against (1) the sums over the dx the call stored and (2) the fp64 reference.
    stored / ref / bound: dx on the compact lattice (N,C,OH,OW); xl: the BatchNorm's raw input at those
    points; bn = (mean, invstd, gamma, beta, relu)."""
    part = np.asarray(part, dtype=np.float64)
    assert not np.isnan(part).any(), "{}: partial rows never written".format(name)
    got = _sum(part)
    m, i, ga, be = (np.asarray(v, dtype=np.float64)[None, :, None, None] for v in bn[:4])
    stored = np.asarray(stored, dtype=np.float64)
    xh = (xl - m) * i
    mask = (ga * xh + be > 0) if bn[4] else np.ones_like(xh, dtype=bool)
    g, gr, bm, xh = rows(stored * mask), rows(ref * mask), rows(bound * mask), rows(xh)
    acc = EPS * (g.shape[0] + part.shape[0] + 2)
    check(name + " g|stored", got[0], _sum(g), acc * _sum(np.abs(g)))
    check(name + " gx|stored", got[1], _sum(g * xh), (acc + XH) * _sum(np.abs(g * xh)))
    check(name + " g|ref", got[0], _sum(gr), _sum(bm) + acc * _sum(np.abs(gr)))
    check(name + " gx|ref", got[1], _sum(gr * xh),
          (1 + XH) * _sum(bm * np.abs(xh)) + (acc + XH) * _sum(np.abs(gr * xh)))
