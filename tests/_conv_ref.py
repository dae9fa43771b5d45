"""fp64 reference of the dense convolution and the per-element error bounds its fp32 and bf16 kernels are held to
(tests/test_conv_ref_host.py, tests/test_gpu_conv_elementwise.py, tests/test_gpu_conv_bf16_elementwise.py).  Host
only: numpy + torch-CPU, nothing from dorknet_amd, no GPU call.  The pieces shared with the depthwise and pointwise
references come from tests/_dw_ref.py and tests/_pw_ref.py.

Operation (layers/convolution.py; oracle.ref.conv_forward / conv_backward), OH = (H + 2 pad - R) // stride + 1:
    a  = bn(x) (+ ReLU) where an input BatchNorm is applied on load, else x; zero padding AFTER the BatchNorm
    y[n,k,oh,ow]  = sum_{c,r,s} a[n,c,stride oh + r - pad, stride ow + s - pad] w[k,c,r,s] + bias[k]
    dx[n,c,h,w]   = sum over the (k, r, s) that reach the pixel of dy w; the forward input's H x W -- a pixel no
                    tap reaches (1x1 at stride 2; rows the forward never read, (H + 2 pad - R) % stride != 0)
                    is exactly 0
    dw[k,c,r,s]   = sum_{n,oh,ow} dy a + l2 w
    stats[rows][2][K] = (sum y, sum y^2) of the STORED y over the rows the call wrote
    *_bnbwd_*: dy = bn_bwd_elem(g, x1, out_bn, k12) (_dw_ref.bn_bwd_dy, its error scale ed and mask variable);
               g_lattice = 2: g is given compact on the even (oh, ow); the reference is the widened g with exact
               zeros off the lattice (dy is NOT zero there: -gamma invstd (k1 + x_hat k2)).
The arithmetic is torch.nn.functional.conv2d / torch.nn.grad.conv2d_input / conv2d_weight in fp64 on the CPU.

Absolute twins (the same code on absolute values; the scale of the rounding error of any evaluation order):
    ya = conv(|a|, |w|) + |bias|,  dxa = dgrad(|dy|, |w|),  dwa = wgrad(|dy|, |a|).

Bounds on |got - ref| per element, none excluded, none fitted to a kernel's output (u = 2^-24):
    y, dx from the MFMA kernels   A = STEP (n + 3) twin + E,  STEP = _pw_ref.STEP = 2 u.
        ASSUMPTION (that of tests/_pw_ref.py, kept and quoted): "one ulp (2 u) per accumulation step.  Neither
        the repository nor its guides say how v_mfma_f32_32x32x2_f32 and v_mfma_f32_32x32x16_bf16 round inside
        an instruction ...; one ulp per step is what any faithful implementation satisfies in any order."  The
        narrow kernels' v_mfma_f32_16x16x4_f32 (conv_narrow.hip:40-42) is held to the same.
        n = the padded reduction length the kernel runs:
          engine forward    R S Cp          (gemm_conv.hip:96: Ktot = R * S * C with C the stored channels)
          narrow forward    roundup4(C R S) (conv_narrow.hip:128: KK = (KRED + 3) / 4 k-steps of 4)
          dk_conv2d_dgrad   R S K           (gemm_conv.hip:131)
          phase dgrad       Rp Sp Kp of the pixel's phase (gemm_conv.hip:167; phase_taps, gemm_engine.h:1327-1330),
                            which is at most R S Kp; a phase without taps has n = 0 and twin = 0: exact zeros
        + 3: the bias add, the first-order slack of (1 + 2u)^n and one spare, as in _pw_ref.
        E = conv(ea, |w|): the operand's own error scale carried through |w| (ea from _dw_ref.bn_operand).
    dx from the sub-pixel kernel  U n dxa, n = (taps of the pixel's phase) K + 2.  Packed VALU FMAs
        (conv_subpixel.hip:107-108: one rounding per multiply-add), the k-sum split over even and odd k and joined
        by one add (:129): a chain is taps K / 2 + 1 roundings long, so u per step over taps K + 2 steps holds
        with room for the second-order terms of (1 + u)^n.  u per step is what _dw_ref holds VALU arithmetic to.
    dw   STEP (M + 2) dwa + 2 u |ref| + wgrad(|dy|, ea) + wgrad(ed, |a|),  M = N OH OW terms in any grouping
        (split-K slabs, gemm_engine.h:1289-1297; the narrow kernels' per-block partials, conv_narrow.hip:379-386;
        their fixed-order reduce); 2 u |ref| the final cast and the l2 fma.
    statistics  _pw_ref.stats_checks: (1) against fp64 sums of what the same call stored:
        2^-53 (M + rows + 2) sum |term|; (2) against the reference sums: the summed per-element bounds.
        (engine: EpStoreStats on kRowConv tiles, gemm_engine.h:1414-1418; narrow: conv_narrow.hip:193-195, :205-211.)

bf16 mode (bf16=True: dk_conv2d_{fwd_ex,dgrad,dgrad_phase,wgrad,wgrad_bnx}_bf16, gemm_bf16.hip:213-302; every GEMM on
v_mfma_f32_32x32x16_bf16, gemm_engine.h:930-943).  The rules are those of tests/_pw_ref.py, quoted:
    weights   "The reference uses wq = rne_bf16(w) EXACTLY in y and dx (the rounding of a given fp32 weight is
              unambiguous)"; "the weights do not enter [the weight gradient] except in l2 w, which uses the fp32 w".
    operands  "raw bf16 activations and a raw bf16 dy are exact; an operand formed on load (the BatchNorm output ...)
              is a bf16 rounding of an fp32 value within e of the fp64 value, error scale 2^-8 (|v| + e) + e
              (operand_err)".  ReLU commutes with the rounding (both monotone, 0 fixed).
    padding   exactly 0 AFTER the BatchNorm (gemm_bf16.hip:219-222: each 4-group takes its own tap's bounds test and
              the BatchNorm transforms in-image elements only); the zero padded channel of Cp > C is in the image, so
              it is normalised to its own bn(0) != 0 (beta != 0): it meets zero weights in y and must be dropped by
              the weight gradient's Cp -> C compaction.
    y, dx     A = STEP (n + 3) twin + E as above with the fp32 accumulation, n the padded reduction length the
              bf16 kernel runs: Ktot zero-filled (k >= Ktot loads 0, gemm_engine.h:241, :326) to whole k-tiles
              (:856) of BK / 16 MFMAs (:932); BK is 16 (row configs 6, 14) or 32 (8, 15, 16), so n = roundup32(Ktot)
              covers every route.  Zero products add no rounding; the padding is counted all the same.
                forward          Ktot = R S Cp                (gemm_bf16.hip:242)
                dk_conv2d_dgrad  Ktot = R S K                 (gemm_engine.h:1486)
                phase dgrad      Ktot = Rp Sp Kp of the phase (gemm_engine.h:1512); no taps: n = 0, twin = 0, exact 0
              The store is one RNE (rnd4<bf16_t> in EpStoreT::value4, gemm_engine.h:577-581; st4 of EpPhaseT, :797-799),
              held to bf16_bound(ref, A) -- the interval form -- and to bf16_closed(ref, A): Ref.b16 / Ref.b16c.
    dw        fp32 (split-K slabs and their reduce as for fp32): the fp32 form with the rounded operands' scales,
              STEP (M + 2) dwa + 2 u |ref| + wgrad(|dy|, operand_err(a, ea, True)); a raw bf16 dy is exact.
    statistics  stats_checks unchanged, over the bf16 values the call stored (EpStoreStatsT<bf16_t> accumulates the
              rounded value4, gemm_engine.h:606-614) and against the reference with the summed b16 bounds.
No kernel output has moved any constant above.

ReLU masks: the inputs are chosen (SEEDS) so that _dw_ref.mask_margin > 1 for the input BatchNorm (on x) and the
following one (on x1) of every case; tests/test_conv_ref_host.py asserts it, so no element is excluded for a flip.

Inputs (make_inputs): x, dy, g, x1 bf16-representable; w = randn / sqrt(C R S) in fp32 (not bf16-representable);
bias, BatchNorm vectors (Cp entries for the engine: the padded channel has its own, with beta != 0, so that bn(0) of
the zero padded channel is not zero and would show if it leaked into dw) and k12 arbitrary fp32.  One seed per case.

Tile and route rules the case tables cite, as read from the code:
    row tiles (gemm_engine.h:1216-1248, kRowConv, fp32): R S Cp <= 128 and K <= 64 -> config 14 (128 x 64 x 16);
        R S Cp <= 128 and K > 64 -> config 6 (64 x 64 x 16); R S Cp > 128 -> config 8 (64 x 64 x 32).  Both dgrads are
        kRowPlain: reduction <= 128 -> 6, else 8.
    split-K (gemm_engine.h:1266-1281): K <= 64 < R S Cp -> config 6 (64 x 128 x 32), else config 1 (64 x 64 x 32);
        splits = min(ceil(1024 / tiles), ceil(M / 32)) (:1289-1297): M <= 32 pixels is a single split.
    bf16 row tiles (gemm_engine.h:1209-1222, then the fp32 rules :1234-1237; forward and both dgrads are kRowConv,
        gemm_bf16.hip:243, :252, :264; "columns" are K for the forward and C for the dgrads, the reduction is R S Cp,
        R S K or the phase's Rp Sp Kp): reduction > 128 -> config 16 (128 x 128 x 32, 8 waves) with >= 128 columns, else
        config 15 (128 x 64 x 32); reduction <= 128 -> config 14 (128 x 64 x 16) with <= 64 columns, else config 6
        (64 x 64 x 16).  No bf16 convolution picks config 8 (64 x 64 x 32).
    bf16 split-K (gemm_engine.h:1265-1275): K >= 128 and R S Cp >= 128 -> config 4 (128 x 128 x 32); K <= 64 < R S Cp
        -> config 6 (64 x 128 x 32); else config 1 (64 x 64 x 32); the splits as for fp32.
    narrow (conv_narrow.hip:394-423): shapes (C,R,S,stride) in (3,5,5,2) (3,7,7,2) (3,3,3,1) (3,3,3,2) (1,3,3,1) (1,5,5,1);
        4 <= K <= 64, K % 4 == 0; forward T = ceil(OW / 16) in 1..8; quads(OW) buckets {4, 8, 16, 28, 32} of
        ceil(OW / 4); staged columns st (16 T - 1) + S and st (4 quads - 1) + S at most 256: at stride 2 that is
        OW <= 112 (T = 7, 28 quads), at stride 1 OW <= 128; rows per block = ceil(N OH / min(N OH, occ 256)) (:484-491).
    sub-pixel (conv_subpixel.hip:161-195): (R,S,stride,pad) in (5,5,2,2) (5,5,2,1) (3,3,2,1) (4,4,2,1) (7,7,2,3) (3,3,2,0)
        (2,2,2,0); C <= 16 in groups of CO = min(C, 4); tiles of 4 x 64 quads; K % 4 != 0 takes the scalar dy loads."""
import collections

import numpy as np
import torch

from tests import _pw_ref as P
from tests._dw_ref import U, bf16_values, bn_bwd_dy, bn_operand, bn_params, mask_margin, out_hw, worst  # noqa: F401
from tests._dw_ref import check as _check
from tests._pw_ref import STEP

L2 = float(np.float32(1e-3))
MAX_ELEMENTS = 1 << 20      # cap on the elements of any one tensor of a case (tests/test_conv_ref_host.py)

Case = collections.namedtuple("Case", "C Cp R S stride pad N H W K")

# Engine cases (gemm_conv.hip): each the smallest shape reaching the named edge.
ENGINE = {
    # 3x3 s1 p1; R S Cp = 72 <= 128, K = 24 <= 64: row config 14; M = 286 ragged for 128 (2 tiles + 30); K no multiple
    # of 16; split-K config 6 (K <= 64 < 72), 9 splits of 32 pixels, the last ragged (30); odd H != W
    # bf16: forward row config 14, dgrads config 15 (R S K = 216 > 128, C = 8 < 128), split-K config 6
    "e1": Case(8, 8, 3, 3, 1, 1, 2, 13, 11, 24),
    # 3x3 s1 p0; R S Cp = 108 <= 128, K = 72 > 64: row config 6; M = 198 = 3 x 64 + 6; ragged second column tile (72);
    # Cp = 12: 16-wide k-tiles cross tap boundaries, the last is ragged (108 = 6 x 16 + 12); split-K config 1
    # bf16: forward row config 6, stride-1 / phase dgrad config 15 (C = 12: every other dx row 8 bytes off a 16-byte
    # boundary), split-K config 1
    "e2": Case(12, 12, 3, 3, 1, 0, 2, 13, 11, 72),
    # 4x4 s2 p1; R S Cp = 128: config 14; M = 60 < one tile; (H + 2 pad - R) % 2 = 1 (the remainder is the bottom
    # padding row: every input row is still read, see e12)
    # bf16: forward config 14; phases of 2 x 2 taps, R S Kp = 96: config 14; split-K config 6
    "e3": Case(8, 8, 4, 4, 2, 1, 2, 13, 11, 24),
    # 5x5 s2 p1, C = 3 in Cp = 4 (the stem on the engine): config 14; M = 256 = exactly two 128-row tiles; scalar
    # EpPhase store (C % 4 != 0); the wgrad reduce compacts Cp -> C
    # bf16: forward config 14; phases of 4 .. 9 taps x 64: config 15, 6-byte pixels (scalar store); split-K config 6
    "e4": Case(3, 4, 5, 5, 2, 1, 4, 17, 17, 64),
    # 7x7 s2 p3, C = 3 in Cp = 4; R S Cp = 196 > 128: row config 8; M = 96 = 64 + 32 ragged; split-K config 6
    # bf16: forward config 15 (R S Cp = 196 > 128, K < 128); phases of 9 .. 16 taps x 24: config 15; split-K config 6
    "e5": Case(3, 4, 7, 7, 2, 3, 2, 15, 11, 24),
    # 1x1 s2 p0: three of the four dx phases have no taps and must be written as exact zeros
    # bf16: config 14 throughout (the empty phases run it with no k-tile); split-K config 1 (R S Cp = 8 <= 64)
    "e6": Case(8, 8, 1, 1, 2, 0, 2, 9, 7, 24),
    # 4x4 s3 p2 on 17 x 13: ragged phases (6 / 6 / 5 rows, 5 / 4 / 4 columns); (H + 2 pad - R) % 3 = 2
    # bf16: forward config 14 (R S Cp = 128); phases of 1 / 2 / 4 taps x 24: config 14; split-K config 6
    "e7": Case(8, 8, 4, 4, 3, 2, 2, 17, 13, 24),
    # 3x3 s1 pad = R - 1 = 2: the output (7 x 8) is larger than the input (5 x 6); K = 72: config 6; M = 56 < one tile
    # bf16: forward config 6, dgrads config 15, split-K config 1
    "e8": Case(8, 8, 3, 3, 1, 2, 1, 5, 6, 72),
    # 3x3 s1 p1, R S Cp = 144 > 128 with K = 72: row config 8, two column tiles; M = 128 = exactly two 64-row tiles;
    # split-K config 1 (the other branch) with 4 whole splits
    # bf16: forward config 15 (144 > 128, K = 72 < 128), dgrads config 15, split-K config 1
    "e9": Case(16, 16, 3, 3, 1, 1, 2, 8, 8, 72),
    # M = 30 <= 32 pixels: a single split-K split; one partial row tile
    # bf16: as e1 (14 / 15 / split-K config 6, one split)
    "e10": Case(8, 8, 3, 3, 1, 1, 1, 5, 6, 24),
    # K = 6 (K % 4 != 0: dy zero-padded to Kp = 8 for the phase dgrad, scalar dy loads in the weight gradient) and
    # C = 3 in Cp = 4 at stride 1
    # bf16: the forward, the stride-1 dgrad and the weight gradients refuse K % 4 != 0; the phase dgrad takes K = 6 in
    # Kp = 8 (reduction 72, config 14) and stores 6-byte pixels
    "e11": Case(3, 4, 3, 3, 1, 1, 2, 7, 5, 6),
    # 3x3 s2 p0 on 12 x 10: (H - R) % 2 = 1 > pad: the last dx row and column are never read by the forward and
    # must be written as exact zeros
    # bf16: config 14 throughout (phase reductions 96 / 48 / 48 / 24); split-K config 6
    "e12": Case(8, 8, 3, 3, 2, 0, 2, 12, 10, 24),
}

# Engine cases for what ENGINE does not reach under the bf16 rules (bf16 row configs 16 and, in a dgrad, 6; split-K
# config 4; K % 8 == 4).  Run in bf16 by tests/test_gpu_conv_bf16_elementwise.py, in both modes on the host.
ENGINE16 = {
    # 3x3 s1 p1, R S Cp = 144 > 128 with K = 128: forward row config 16 (128 x 128 x 32, 8 waves); M = 162 = 128 + 34
    # ragged: 2 statistics rows, 3 on 64-row tiles; split-K config 4 (K >= 128, R S Cp >= 128: 128 x 128 tiles, the
    # second column tile ragged, 144 = 128 + 16), 6 splits, the last ragged (162 = 5 x 32 + 2); dgrads config 15
    "h1": Case(16, 16, 3, 3, 1, 1, 2, 9, 9, 128),
    # the mirror image: C = 128 with R S K = 144 > 128: both dgrads on row config 16; the forward on config 15 with
    # its longest reduction (R S Cp = 1152: 36 k-tiles); split-K config 6 over nine 128-column tiles
    "h2": Case(128, 128, 3, 3, 1, 1, 2, 9, 9, 16),
    # K = 20 (K % 8 == 4): 40-byte y and dy rows, every other one 8 bytes off a 16-byte boundary; 3x3 s2 p1 on
    # 13 x 11: M = 84, phases of 1 / 2 / 2 / 4 taps; config 14 throughout, split-K config 6
    "h3": Case(8, 8, 3, 3, 2, 1, 2, 13, 11, 20),
    # C = 72 > 64 with R S K = 72 <= 128: both dgrads on row config 6 (64 x 64 x 16), which ENGINE reaches in the
    # forward only; a ragged second column tile (72 = 64 + 8); M = 30 < one tile; forward config 15, split-K config 6
    "h4": Case(72, 72, 3, 3, 1, 1, 1, 5, 6, 8),
}

# Narrow cases (conv_narrow.hip); T = ceil(OW / 16), q = ceil(OW / 4) -> quads bucket.
NARROW = {
    # shape (3,5,5,2): the stem's width at small height: OW = 112, T = 7, q = 28 -> 28, 227 staged columns; OH = 2
    "n1": Case(3, 3, 5, 5, 2, 1, 1, 5, 225, 64),
    # shape (3,7,7,2): OH = 5, OW = 19 odd (lattice), T = 2, q = 5 -> 8 (padded quads); K = 48: wave 3 empty
    "n2": Case(3, 3, 7, 7, 2, 3, 2, 9, 37, 48),
    # shape (3,3,3,1): OW = 17 just past a bucket edge: T = 2, q = 5 -> 8; K = 20: wave 1 ragged, waves 2, 3 empty
    "n3": Case(3, 3, 3, 3, 1, 1, 2, 5, 17, 20),
    # shape (3,3,3,2): OW = 7 no multiple of 4, T = 1, q = 2 -> 4; K = 4: a single quad of filters
    "n4": Case(3, 3, 3, 3, 2, 1, 2, 7, 13, 4),
    # shape (1,3,3,1), no padding: OW = 33 just past 32: T = 3, q = 9 -> 16
    "n5": Case(1, 1, 3, 3, 1, 0, 2, 4, 35, 64),
    # shape (1,5,5,1): OW = 115: T = 8, q = 29 -> 32 (padded quads)
    "n6": Case(1, 1, 5, 5, 1, 2, 1, 3, 115, 48),
    # OW = 61: T = 4, q = 16 -> 16 (the bucket's edge)
    "n7": Case(1, 1, 3, 3, 1, 1, 1, 3, 61, 20),
    # OW = 67: T = 5, q = 17 -> 28 (eleven padded quads)
    "n8": Case(3, 3, 3, 3, 1, 1, 1, 3, 67, 64),
    # OW = 91 at stride 2: T = 6, q = 23 -> 28
    "n9": Case(3, 3, 3, 3, 2, 1, 1, 5, 181, 48),
    # multi-row blocks: N OH = 70 x 31 = 2170 rows > 8 x 256 block slots at any occupancy (a block is 4 waves, a CU
    # holds at most 8 such blocks), OH odd so that blocks straddle images; OW = 2 keeps M = 4340 and with it the
    # M-term of the dw bound small enough to see a wrong ring slot (tests/test_conv_ref_host.py)
    "nm1": Case(3, 3, 5, 5, 2, 1, 70, 63, 6, 64),
    # the same with ST = 1 (3x3 stride 1): the ring advances one row at a time
    "nm2": Case(3, 3, 3, 3, 1, 1, 70, 31, 2, 20),
}
MULTIROW = ("nm1", "nm2")

# Sub-pixel dgrad cases (conv_subpixel.hip); QH x QW = ceil(H / 2) x ceil(W / 2) quads in 4 x 64 tiles.
SUBPIX = {
    # (5,5,2,2), CO = 3, K = 64 a multiple of 16; odd H != W; QH = 7 quad rows: no multiple of 4
    "s1": Case(3, 3, 5, 5, 2, 2, 2, 13, 11, 64),
    # (5,5,2,1), K = 24 (a multiple of 4, not of 16); W = 261: QW = 131 = two 64-quad tile columns + 3
    "s2": Case(3, 3, 5, 5, 2, 1, 1, 9, 261, 24),
    # (3,3,2,1), CO = 1, K = 6: the scalar dy path; QH = 6
    "s3": Case(1, 1, 3, 3, 2, 1, 2, 11, 7, 6),
    # (4,4,2,1), CO = 2, K = 70: scalar dy path over five 16-channel passes, the last ragged
    "s4": Case(2, 2, 4, 4, 2, 1, 2, 10, 14, 70),
    # (7,7,2,3), CO = 4 in one group; a one-pixel-high input
    "s5": Case(4, 4, 7, 7, 2, 3, 2, 1, 9, 16),
    # (3,3,2,0), C = 5: two channel groups, the second with one live channel; H = 12: the last row is never read
    "s6": Case(5, 5, 3, 3, 2, 0, 1, 12, 9, 24),
    # (2,2,2,0), C = 16: four channel groups; odd H and W: the last row and column get no tap
    "s7": Case(16, 16, 2, 2, 2, 0, 1, 7, 5, 16),
}

CASES = {**ENGINE, **NARROW, **SUBPIX, **ENGINE16}   # (ENGINE16 last: a case's inputs follow from its position)
ORDER = list(CASES)

# The seed of each case: the first of 0, 1, 2, ... at which mask_margin > 1 holds for the input BatchNorm (on x)
# and the following one (on x1) -- a precondition on the inputs, asserted by tests/test_conv_ref_host.py.
SEEDS = {name: 0 for name in ORDER}     # seed 0 holds for every case


def check(name, got, ref, bound):
    return _check(name, got, ref, bound, tag="conv")


def stats_checks(name, stats, stored, ref, bound):
    """_pw_ref.stats_checks under the "conv" tag."""
    P.stats_checks(name, stats, stored, ref, bound, check=check)


def case_hw(c):
    return out_hw(c.H, c.W, c.R, c.S, c.stride, c.pad)


def roundup4(v):
    return -(-v // 4) * 4


def make_inputs(name):
    """Fixed inputs of a case (fp64 arrays of bf16-representable values; fp32 parameters): x (N,C,H,W); dy, g, x1
    (N,K,OH,OW) the output gradient, the following BatchNorm's gradient and raw input; w (K,C,R,S), bias; pi / po
    the input (Cp entries) / following BatchNorm's (mean, invstd, gamma, beta); k12 its folded coefficients."""
    c = CASES[name]
    rng = np.random.RandomState(11000 + 100 * ORDER.index(name) + SEEDS.get(name, 0))
    OH, OW = case_hw(c)
    d = dict(c._asdict(), OH=OH, OW=OW, M=c.N * OH * OW, name=name, case=c)
    d["x"] = bf16_values(rng.randn(c.N, c.C, c.H, c.W))
    for k in ("dy", "g", "x1"):
        d[k] = bf16_values(rng.randn(c.N, c.K, OH, OW))
    d["w"] = (rng.randn(c.K, c.C, c.R, c.S) / np.sqrt(c.C * c.R * c.S)).astype(np.float32)
    d["bias"] = rng.randn(c.K).astype(np.float32)
    d["pi"] = bn_params(c.Cp, rng)
    d["po"] = bn_params(c.K, rng)
    d["k12"] = (rng.randn(2 * c.K) * 0.1).astype(np.float32)
    return d


def pi_of(d, relu):
    """The input BatchNorm of the C real channels, or None."""
    return None if relu is None else (*(v[:d["C"]] for v in d["pi"]), relu)


def margins(d):
    """The mask_margin of every ReLU decision a test of this case can make; every beta must be non-zero."""
    assert min(np.abs(d["pi"][3]).min(), np.abs(d["po"][3]).min()) > 0
    return min(mask_margin(d["x"], pi_of(d, 1)), mask_margin(d["x1"], (*d["po"], 1)))


# ---------------------------------------------------------------------------------------------------------
# the arithmetic
# ---------------------------------------------------------------------------------------------------------

def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64))


def conv(a, w, stride, pad):
    return torch.nn.functional.conv2d(_t(a), _t(w), None, stride, pad).numpy()


def conv_dx(dy, w, stride, pad, H, W):
    shape = (dy.shape[0], w.shape[1], H, W)
    return torch.nn.grad.conv2d_input(shape, _t(w), _t(dy), stride, pad).numpy()


def conv_dw(dy, a, wshape, stride, pad):
    return torch.nn.grad.conv2d_weight(_t(a), tuple(wshape), _t(dy), stride, pad).numpy()


def phase_taps(a, R, st, pad):
    """Taps of sub-pixel phase a along one axis (gemm_engine.h phase_taps)."""
    r0 = (a + pad) % st
    return (R - r0 + st - 1) // st if r0 < R else 0


def taps_map(c):
    """(H, W): the taps (r, s) of each dx pixel's phase."""
    th = np.array([phase_taps(h % c.stride, c.R, c.stride, c.pad) for h in range(c.H)])
    tw = np.array([phase_taps(w % c.stride, c.S, c.stride, c.pad) for w in range(c.W)])
    return th[:, None] * tw[None, :]


def widen_lattice(g2, OH, OW):
    """The compact even-lattice g (N,K,ceil(OH/2),ceil(OW/2)) on the OH x OW grid, zeros elsewhere."""
    g = np.zeros(g2.shape[:2] + (OH, OW))
    g[:, :, ::2, ::2] = g2
    return g


def roundup32(v):
    return -(-v // 32) * 32


class Ref:
    """Result and bound of one call: ref, A (the fp32 bound; in bf16 mode the bound on the value before the store),
    and in bf16 mode of y / dx b16 / b16c, the bf16 store's bounds (interval / closed form)."""

    def __init__(self, ref, A, stored16=False):
        self.ref, self.A = ref, A
        if stored16:
            self.b16, self.b16c = P.bf16_bound(ref, A), P.bf16_closed(ref, A)

    def bound(self, bf16):
        return self.b16 if bf16 else self.A


def forward(d, bias=False, bn=None, narrow=False, bf16=False):
    """y and its bound.  bn: None / 0 / 1 = the input BatchNorm off / without / with ReLU.  Also .a / .ea: the operand
    and its error scale as the MFMA sees it.  bf16: the engine's bf16 entry (module docstring)."""
    c = d["case"]
    assert not (narrow and bf16)
    a, ea, _ = bn_operand(d["x"], pi_of(d, bn))
    ea = P.operand_err(a, ea, bf16 and bn is not None)
    w = P.weights(d["w"], bf16)
    y, ya = conv(a, w, c.stride, c.pad), conv(np.abs(a), np.abs(w), c.stride, c.pad)
    if bias:
        b64 = d["bias"].astype(np.float64)[None, :, None, None]
        y, ya = y + b64, ya + np.abs(b64)
    n = roundup4(c.C * c.R * c.S) if narrow else c.R * c.S * c.Cp
    if bf16:
        n = roundup32(n)
    o = Ref(y, STEP * (n + 3) * ya + conv(ea, np.abs(w), c.stride, c.pad), bf16)
    o.a, o.ea = a, ea
    return o


def dgrad(d, entry, bf16=False):
    """dx (N,C,H,W) and its bound; entry: "gemm" (dk_conv2d_dgrad_f32 / _bf16), "phase", "subpixel" (fp32 only)."""
    c = d["case"]
    w = P.weights(d["w"], bf16)
    pad32 = roundup32 if bf16 else (lambda v: v)
    dx = conv_dx(d["dy"], w, c.stride, c.pad, c.H, c.W)
    dxa = conv_dx(np.abs(d["dy"]), np.abs(w), c.stride, c.pad, c.H, c.W)
    if entry == "gemm":
        assert c.stride == 1
        return Ref(dx, STEP * (pad32(c.R * c.S * c.K) + 3) * dxa, bf16)
    taps = taps_map(c)[None, None]
    if entry == "phase":
        return Ref(dx, STEP * (pad32(taps * roundup4(c.K)) + 3) * dxa, bf16)
    assert entry == "subpixel" and not bf16
    return Ref(dx, U * (taps * c.K + 2) * dxa)


def wgrad(d, l2=0.0, bn=None, dy=None, ed=None, bf16=False):
    """dw (K,C,R,S), fp32 in both modes, and its bound; dy / ed: the gradient formed on load and its error scale
    (default: d["dy"]; fp32 only).  bf16: the operand a of a BatchNorm on load is rounded to bf16."""
    c = d["case"]
    assert not (bf16 and dy is not None)
    a, ea, _ = bn_operand(d["x"], pi_of(d, bn))
    ea = P.operand_err(a, ea, bf16 and bn is not None)
    dy = d["dy"] if dy is None else dy
    shape = d["w"].shape
    dw = conv_dw(dy, a, shape, c.stride, c.pad) + l2 * d["w"].astype(np.float64)
    b = STEP * (d["M"] + 2) * conv_dw(np.abs(dy), np.abs(a), shape, c.stride, c.pad) + 2 * U * np.abs(dw)
    if bn is not None:
        b = b + conv_dw(np.abs(dy), ea, shape, c.stride, c.pad)
    if ed is not None:
        b = b + conv_dw(ed, np.abs(a), shape, c.stride, c.pad)
    return Ref(dw, b)


def formed_dy(d, relu, lattice=1):
    """(dy, ed) of the following BatchNorm's backward applied to g (dense, or the even lattice of g widened)."""
    g = d["g"] if lattice == 1 else widen_lattice(d["g"][:, :, ::2, ::2], d["OH"], d["OW"])
    return bn_bwd_dy(g, d["x1"], (*d["po"], relu), d["k12"])[:2]
