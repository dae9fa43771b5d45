"""fp64 references of the classifier head's kernels -- global average pooling, the dense layer, softmax with
cross-entropy, the bias-gradient column sums, the l2 term (dorknet_amd/csrc/elementwise.hip, gemm_dense.hip) -- with
the per-element error bounds they are held to, and bitwise references of the small exact kernels around them
(tests/test_head_ref_host.py, tests/test_gpu_head_elementwise.py).  Host only: numpy + torch-CPU, nothing from
dorknet_amd, no GPU call.  Shared pieces come from tests/_dw_ref.py (U, bf16 helpers, bn_operand, worst / check) and
tests/_pw_ref.py (STEP, EPS).

u = U = 2^-24, e = EPS = 2^-53.  No constant below was fitted to a kernel's output; no element is excluded.  Inputs are
fp32 values (bf16-representable where a bf16 entry shares the case), so reference and kernel read the same numbers.

Global average pooling, x[N][HW][C] (elementwise.hip:176-193 gap_fwd_kernel; :239-258 gap_bwd_kernel / gap_bwd4_kernel)
    forward   s = 0; s += x_k in order (:182-191: HW additions, the first exact), out = s / (float) HW (:192, one
              correctly rounded division): HW roundings, each relative to a partial sum of at most sum|x|, + 1 for the
              second order:                          |got - ref| <= u (HW + 1) sum|x| / HW.
              bf16 x is widened exactly (dk_common.h:56-58) and summed by the same lines: the same bound.
    backward  f = 1.0f / (float) HW (:246, :256: one rounding), dx = f * dy (one rounding): 2 u (1 + u) |ref|;
              exact (bound 0) when HW is a power of two.  bf16 dx: one round-to-nearest-even store of that product
              (dk_common.h:54, :66): _dw_ref.bf16_bound, and bitwise what the fp32 entry's result rounds to.
    join      dk_gap_join_fwd_f32 (:201-235): y = ReLU(bnA(a) + bnB(b)) formed per element as bn_add_kernel forms it,
              then the forward's sum.  Per element _bn_ref's apply bound ea = 4 u (|gamma x_hat| + |beta|) for each
              normalised operand (_dw_ref.bn_operand; an inner ReLU is 1-Lipschitz), u |va + vb| for the add, the
              outer ReLU 1-Lipschitz: ej.  out: u (HW + 1) sum y / HW + (1 + u HW) sum ej / HW.  The mask byte is the
              reference decision: join_margin = min |va + vb| / (2 ej) must exceed 1 (asserted on the host).

Column sums, in[M][N] (elementwise.hip: colsum_partial_kernel, colsum_final_kernel, colsum_chunks, dk_colsum_f32 /
dk_colsum_bf16): every term widened to fp64 (both loops of colsum_partial_kernel), added in fp64 within a chunk of
rpc = ceil(M / chunks) rows, chunks = min(ceil(M / 64), 512), the chunk sums added in fp64 and cast once
(colsum_final_kernel).  M + chunks additions in any grouping, one fp32 rounding:
                                                     u |ref| + (1 + u) e (M + chunks) sum|x|.
    The ill-conditioned column (column 0 of every case with M >= 7) holds large cancelling values whose sum is of the
    order of one term's last bits: there sum|x| / |ref| is above 10^6 and fp32 accumulation (u per addition) is far
    outside the bound while fp64 accumulation is inside.

l2 term (l2_loss_kernel in elementwise.hip; l2_multi_partial_kernel and l2_multi_final_kernel in multi_tensor.hip):
v * v of a widened fp32 is exact in fp64 (48 bits); n terms over 256 strided threads and a 256-leaf tree (block_sum,
dk_common.h), 0.5 * (double) strength exact, one fp64 product, one cast:
                                                     ev = u |v| + (1 + u) e (n + 258) |v|   (all terms positive).
    accumulate: out[0] + v in fp32: + u (|prior + v| + ev).
    multi: per 2048-element chunk the same sum (chunk_sum_squares), the chunk values added in fp64 over 256 strided
    threads and a tree (sum_partials) with add_to widened, one cast:
                                                     u |ref| + (1 + u) e (n_total + parts + 258) (|add_to| + sum v_t).

Softmax with cross-entropy, x[B][K] (elementwise.hip:262-375).  No max shift (losses.py:15-16), in the reference
neither.  Every term is positive, so the bounds on P are relative to p:
    e_j = expf(x_j) (:311, :353, :358)                          EXPF each, in numerator and in the sum
    s = sum e_j: K positive terms in any grouping -- per-lane sums of up to 32 (:308-313) and two quad exchanges
        (:314-315), or 64 lane sums and a six-level wave tree (:353-354) -- at most K - 1 roundings on any term's path
    inv = 1.0f / s (:316, :355), p = inv * e_j (:320, :358)     one rounding each
                                                     |P - p| <= p (2 EXPF + (K + 3) u)       (+ 2: second order)
    ASSUMPTION: one ulp (2 u) for expf and for logf.  Neither the repository nor its guides say how accurate the
    device library's expf and logf are, and the ROCm documentation installed with the toolchain states no figure; the
    library is built without fast-math (__graft_entry__.py HIPFLAGS); one ulp is what a faithful implementation of
    either satisfies.  The constants have not been changed on any kernel output.
    loss: dot_b = sum_j p_j y_j (:317-323, :335-336; :357-363): p_j as above, one rounding per product (or none, when
        contracted into the sum), at most K roundings on the sum of non-negative terms: relative rd = rp + (K + 1) u.
        l_b = -logf(dot_b) (:337, :364): -log1p(-rd) from the argument (absolute), LOGF |l_b| from logf itself.
        The row losses are widened and added in fp64 (:342-344, :364, :372), times 1 / B in fp64, one cast (:373):
                                                     sum_b el_b / B + e (B + 20) sum|l_b| / B + u |loss|.
    y = NULL with loss = NULL (test mode): P as above, the loss word untouched.
    backward (:378-383): dx = fl(1 / B) * (p - y) on the P the DEVICE stored: three roundings, 3 u (1 + 2 u) |ref|.

Dense layer (gemm_dense.hip:7-47 on gemm_engine.h), the forms of tests/_conv_ref.py with its ASSUMPTION of one ulp
(STEP = 2 u) per MFMA accumulation step:
    y = x w + bias      STEP (IN + 3) (|x| |w| + |bias|)        dx = dy w^T      STEP (OUT + 3) |dy| |w|^T
    dw = x^T dy + l2 w  STEP (B + 2) |x|^T |dy| + 2 u |ref|     (split-K slabs and their reduce, any grouping)
    Tile rules (gemm_engine.h:1206-1237 row_config, :1261-1276 splitk_config, :1284-1292 wgrad_splits): forward and
    dgrad are kRowPlain: reduction <= 128 -> config 6 (64 x 64 x 16), else 8 (64 x 64 x 32); the weight gradient has
    M = IN, N = OUT, reduction B: IN <= 64 < OUT -> config 6 (64 x 128 x 32), else 1 (64 x 64 x 32); splits =
    min(ceil(1024 / tiles), ceil(B / 32)).  vec_ok (:1366-1368): leading dimension, both extents multiples of 4 and a
    16-byte pointer, else the scalar loaders; ep_store (:1427-1430): OUT % 4 == 0, 16-byte output and bias, else the
    scalar store.

Exact kernels (elementwise.hip: relu_fwd_kernel, relu_bwd_kernel, mask_to_f32_kernel, add_kernel, the nchw_to_nhwc and
nhwc_unpad kernels, scale_kernel, the two cast kernels): bitwise references.  relu: v > 0 ? v : 0, mask v > 0
(-0.0 -> +0.0, NaN -> 0 with mask 0); add, scale: one IEEE operation in numpy fp32, subnormal operands and results
included (no build flag flushes them; on the host under tests/_optim_twin.ieee_host, since loading the oracle's
-ffast-math library leaves the thread flushing them); casts: torch-CPU round-to-nearest-even / exact widening; layout
kernels and dk_mask_to_f32: index arithmetic.  A NaN result of add, scale or a cast must be a NaN: IEEE 754 leaves the payload of a
NaN result to the implementation (torch-CPU's bf16 cast of a NaN stores all ones here, numpy keeps the first operand's
payload); every other result is compared bit for bit (same_bits, same16)."""
import collections
import struct

import numpy as np
import torch

from tests._dw_ref import U, UB, bf16_bound, bf16_values, bn_operand, bn_params, worst  # noqa: F401
from tests._dw_ref import check as _check
from tests._optim_twin import ieee_host
from tests._pw_ref import EPS, STEP

f32 = np.float32
EXPF = 2 * U        # ASSUMPTION (module docstring): one ulp; not fitted
LOGF = 2 * U        # ASSUMPTION (module docstring): one ulp; not fitted
L2 = float(f32(1e-3))               # = _conv_ref.L2
MAX_ELEMENTS = 1 << 20              # cap on the elements of any one tensor of a case, GRID_STRIDE_N alone excepted
GRID_STRIDE_N = 16384 * 1024 + 1029     # grid4's cap (elementwise.hip) is 16384 blocks x 256 threads x 4:
#                                         257 float4 chunks take a second trip, and the tail is 1029 % 4 = 1 element


def check(name, got, ref, bound):
    return _check(name, got, ref, bound, tag="head")


def cdiv(a, b):
    return -(-a // b)


def q16(a):
    """fp32 -> bf16 (nearest even) -> fp32, torch-CPU."""
    with ieee_host():
        return torch.as_tensor(np.ascontiguousarray(a, dtype=f32)).to(torch.bfloat16).float().numpy()


def bits16(a):
    """fp32 -> the bf16 bit patterns (uint16) torch-CPU's round-to-nearest-even cast stores."""
    with ieee_host():
        t = torch.as_tensor(np.ascontiguousarray(a, dtype=f32)).to(torch.bfloat16)
    return t.view(torch.int16).numpy().view(np.uint16)


def widen16(b):
    """bf16 bit patterns (uint16) -> fp32, exact."""
    return (np.ascontiguousarray(b, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(f32)


class Ref:
    """Result and bound of one call."""

    def __init__(self, ref, A):
        self.ref, self.A = ref, A


# ---------------------------------------------------------------------------------------------------------
# global average pooling
# ---------------------------------------------------------------------------------------------------------

# (N, HW, C): each the smallest shape reaching the named edge (256 threads per block, one per (n, c); eight loads
# at a time; gap_bwd4_kernel: four channels per thread when C % 4 == 0 and the pointers allow).
GAP = {
    "g1": (2, 1, 3),        # HW = 1: the remainder loop alone, one trip; C % 4 != 0: scalar backward
    "g2": (3, 7, 6),        # HW < 8: the remainder loop alone
    "g3": (2, 8, 20),       # HW = 8: one unrolled trip, no remainder; C % 4 == 0: the 4-wide backward
    "g4": (3, 9, 1),        # one trip + one remainder element; a single channel
    "g5": (2, 49, 512),     # the network's head; N C = 1024: four blocks
    "g6": (1, 64, 257),     # N C = 257: one thread in the second block; HW a power of two: the backward is exact
    "g7": (2, 81, 20),      # ten trips + one
    "g8": (3, 4, 20),       # the layer test's new (3, 20, 2 x 2) shape
}
GAP_MISALIGNED = ("g3", "g7")   # C % 4 == 0: dy, then dx, at a 4-byte offset takes the scalar backward by pointer
GAP_JOIN = ("g2", "g7")         # dk_gap_join_fwd_f32 against mean(ReLU(bnA(a) + bnB(b)))
JOIN_VARIANTS = ((0, None), (0, 1), (1, 0), (None, 0))     # (a_relu, b_relu); None: that operand is not normalised;
#   never both inner ReLUs: two clipped operands sum to an exact 0, a decision with no margin to measure
JOIN_SEEDS = {}                 # the first of 0, 1, ... at which join_margin > 1 (tests/test_head_ref_host.py): 0


def gap_inputs(name):
    N, HW, C = GAP[name]
    rng = np.random.RandomState(21000 + 100 * list(GAP).index(name) + JOIN_SEEDS.get(name, 0))
    d = dict(N=N, HW=HW, C=C, name=name)
    d["x"] = bf16_values(rng.randn(N, HW, C) + 0.25)
    d["dy"] = rng.randn(N, C).astype(f32).astype(np.float64)
    d["a"] = bf16_values(rng.randn(N, HW, C) * 1.5)
    d["b"] = bf16_values(rng.randn(N, HW, C))
    d["pa"], d["pb"] = bn_params(C, rng), bn_params(C, rng)
    return d


def gap_fwd(x):
    HW = x.shape[1]
    return Ref(x.sum(axis=1) / HW, U * (HW + 1) * np.abs(x).sum(axis=1) / HW)


def gap_bwd(dy, HW):
    """dx [N][HW][C] with its fp32 bound; .b16 the bf16 store's."""
    ref = np.repeat((dy / HW)[:, None, :], HW, axis=1)
    A = np.zeros_like(ref) if HW & (HW - 1) == 0 else 2 * U * (1 + U) * np.abs(ref)
    o = Ref(ref, A)
    o.b16 = bf16_bound(ref, A)
    return o


def _bn_nhwc(x, bn, relu):
    """bn_operand on [N][HW][C]."""
    if relu is None:
        return x, np.zeros_like(x)
    a, ea, _ = bn_operand(x.transpose(0, 2, 1)[..., None], (*bn, relu))
    return a[..., 0].transpose(0, 2, 1), ea[..., 0].transpose(0, 2, 1)


def gap_join(d, a_relu, b_relu):
    """out [N][C], its bound, .mask [N][HW][C] uint8 and .margin."""
    va, ea = _bn_nhwc(d["a"], d["pa"], a_relu)
    vb, eb = _bn_nhwc(d["b"], d["pb"], b_relu)
    pre = va + vb
    ej = ea + eb + U * np.abs(pre)
    y = np.maximum(pre, 0.0)
    HW = d["HW"]
    o = Ref(y.sum(axis=1) / HW, U * (HW + 1) * y.sum(axis=1) / HW + (1 + U * HW) * ej.sum(axis=1) / HW)
    o.mask = (pre > 0).astype(np.uint8)
    o.margin = float((np.abs(pre) / (2 * ej)).min())
    return o


# ---------------------------------------------------------------------------------------------------------
# column sums
# ---------------------------------------------------------------------------------------------------------

# (M, N): 256 columns per block; chunks = min(ceil(M / 64), 512) of rpc = ceil(M / chunks) rows, eight loads at a time
COLSUM = {
    "c1": (1, 1),           # one element
    "c2": (7, 3),           # under eight rows: the remainder loop alone
    "c3": (64, 5),          # one whole chunk: eight unrolled trips, no remainder
    "c4": (65, 4),          # two chunks of 33 and 32 rows
    "c5": (286, 24),        # the bf16 suite's case: 5 chunks of 58, the last 54
    "c6": (130, 257),       # the second column block holds one column; 3 chunks of 44, the last 42
    "c7": (33000, 3),       # ceil(M / 64) = 516 > 512: the cap; 512 chunks of rpc = 65 > 64 rows, the last 45 short
}


def colsum_chunks(M):
    return min(max(cdiv(M, 64), 1), 512)


def colsum_inputs(name):
    M, N = COLSUM[name]
    rng = np.random.RandomState(22000 + list(COLSUM).index(name))
    x = rng.randn(M, N)
    if M >= 7:      # the ill-conditioned column: +-v pairs of magnitude 2^16 .. 2^17 in random rows, which cancel
        #             exactly, and two or three small values that are no multiple of an fp32 ulp at that magnitude
        v = bf16_values(65536.0 * (1 + rng.rand(M // 2 - 1)))
        rest = np.array([97 * 2.0 ** -10, 77 * 2.0 ** -11, 113 * 2.0 ** -12])[:M - 2 * len(v)]
        x[:, 0] = np.concatenate([v, -v, rest])[rng.permutation(M)]
    return bf16_values(x)


def colsum(x):
    M = x.shape[0]
    ref = np.asarray(x, dtype=np.longdouble).sum(axis=0).astype(np.float64)
    return Ref(ref, U * np.abs(ref) + (1 + U) * EPS * (M + colsum_chunks(M)) * np.abs(x).sum(axis=0))


# ---------------------------------------------------------------------------------------------------------
# l2
# ---------------------------------------------------------------------------------------------------------

L2_N = (1, 255, 256, 257, 2049, 4800)       # under / at / past the 256 threads; several strided trips
L2_PRIOR = 3.25                             # the value accumulate = 1 adds onto
L2_CHUNK = 2048
# multi-tensor tables: (sizes, strengths).  "t1": a chunk of one element, one short of / exactly / one past a chunk,
# two whole chunks and a tail; one strength 0.  "t2": 256 * 2048 + 1 elements = 257 chunks, so that with the others
# the final kernel's strided loop (256 threads) takes a second trip.  "t3": 1025 tensors of 3 elements, one more than
# the first-block entries the owner search keeps in LDS: its linear scan over the table in memory.
L2_TABLES = {
    "t1": ((1, 2047, 2048, 2049, 5000), (1e-3, 5e-4, 0.0, 2e-3, 1e-2)),
    "t2": ((300, 256 * 2048 + 1, 2049), (1e-3, 1e-4, 5e-3)),
    "t3": ((3,) * 1025, tuple(1e-4 * (k + 1) for k in range(1025))),
}
L2_ADD_TO = 1.7


def l2_weights(n, seed):
    return (np.random.RandomState(23000 + seed).randn(n) * 0.7).astype(f32)


def l2_table_inputs(name):
    sizes, strengths = L2_TABLES[name]
    ws = [l2_weights(n, 10 * list(L2_TABLES).index(name) + k + 1) for k, n in enumerate(sizes)]
    return ws, [float(f32(s)) for s in strengths]


def l2_blocks(sizes):
    """(first_block of each tensor, total_blocks) of the table (include/dorknet_hip.h)."""
    b0, out = 0, []
    for n in sizes:
        out.append(b0)
        b0 += cdiv(n, L2_CHUNK)
    return out, b0


def l2_table_bytes(ptrs, sizes, strengths):
    """The table of include/dorknet_hip.h: 32-byte records { const float* w; int64 n; int64 first_block; float
    strength; float pad }."""
    b0, _ = l2_blocks(sizes)
    return b"".join(struct.pack("<QqqfI", p, n, b, s, 0) for p, n, b, s in zip(ptrs, sizes, b0, strengths))


def _l2_value(w, strength):
    w = np.asarray(w, dtype=np.longdouble)
    return float(0.5 * np.longdouble(strength) * (w * w).sum())


def l2(w, strength, prior=None):
    """out[0] of dk_l2_loss_f32: overwrite (prior None) or accumulate onto prior."""
    v = _l2_value(w, strength)
    ev = U * abs(v) + (1 + U) * EPS * (len(w) + 258) * abs(v)
    if prior is None:
        return Ref(np.array([v]), np.array([ev]))
    return Ref(np.array([prior + v]), np.array([ev + U * (abs(prior + v) + ev)]))


def l2_multi(ws, strengths, add_to=None):
    vs = [_l2_value(w, s) for w, s in zip(ws, strengths)]
    parts = l2_blocks([len(w) for w in ws])[1]
    base = 0.0 if add_to is None else float(add_to)
    ref = base + float(np.sum(np.asarray(vs, dtype=np.longdouble)))
    n = sum(len(w) for w in ws)
    return Ref(np.array([ref]), np.array([U * abs(ref) + (1 + U) * EPS * (n + parts + 258) * (abs(base) + sum(vs))]))


# ---------------------------------------------------------------------------------------------------------
# softmax with cross-entropy
# ---------------------------------------------------------------------------------------------------------

Soft = collections.namedtuple("Soft", "B K labels logits offset")
# labels: "onehot" / "mixup" (two entries summing to 1) / None (test mode: y = NULL, loss = NULL)
# logits: "randn" (2 randn) / "wide" (uniform in [-30, 30]);  offset: None / "x" / "y" at a 4-byte offset
SOFTMAX = {
    # the float4 path (K % 4 == 0, aligned)
    "s1": Soft(1, 4, "onehot", "randn", None),          # one row, one live lane
    "s2": Soft(6, 120, "mixup", "randn", None),         # 30 quads over 4 lanes: lanes 2, 3 hold one fewer
    "s3": Soft(256, 128, "onehot", "randn", None),      # the widest row the quad path takes; exactly one pass
    "s4": Soft(257, 8, "mixup", "randn", None),         # a second pass of one row
    "s5": Soft(513, 12, "onehot", "wide", None),        # three passes; P over 26 decades
    "s6": Soft(6, 120, None, "randn", None),            # test mode on the float4 path
    # the scalar path (K % 4 != 0)
    "s7": Soft(3, 1, "onehot", "randn", None),          # K = 1: P = 1, loss 0
    "s8": Soft(5, 3, "mixup", "randn", None),           # K < 4: lane 3 of each quad idle
    "s9": Soft(257, 10, "onehot", "randn", None),       # a second pass
    "s10": Soft(300, 127, "mixup", "randn", None),      # 31 / 32 columns per lane, two passes
    # the scalar path by pointer at K % 4 == 0
    "s11": Soft(6, 120, "mixup", "randn", "x"),
    "s12": Soft(6, 120, "onehot", "randn", "y"),
    # one wave per row (K > 128)
    "s13": Soft(3, 129, "mixup", "randn", None),        # K = 129: lane 0 alone takes a third trip
    "s14": Soft(17, 130, "onehot", "randn", None),      # 17 rows over 16 waves: wave 0 takes a second row
    "s15": Soft(2, 1000, "mixup", "randn", None),       # 16 trips per lane, the last ragged
    "s16": Soft(5, 130, None, "randn", None),           # test mode on the wave path
}


def softmax_inputs(name):
    """x [B][K] fp32 and y [B][K] fp32 (None in test mode)."""
    c = SOFTMAX[name]
    rng = np.random.RandomState(24000 + list(SOFTMAX).index(name))
    x = (rng.uniform(-30, 30, (c.B, c.K)) if c.logits == "wide" else 2.0 * rng.randn(c.B, c.K)).astype(f32)
    first = rng.randint(0, c.K, c.B)
    y = None
    if c.labels is not None:
        y = np.zeros((c.B, c.K), dtype=f32)
        if c.labels == "onehot" or c.K == 1:
            y[np.arange(c.B), first] = 1
        else:
            second = (first + 1 + rng.randint(0, c.K - 1, c.B)) % c.K
            lam = (rng.randint(1, 256, c.B) / 256.0).astype(f32)      # lam and 1 - lam exact in fp32
            y[np.arange(c.B), first] = lam
            y[np.arange(c.B), second] = f32(1) - lam
    return x, y


def softmax(x, y=None):
    """P [B][K] with its bound; with labels also .loss / .eloss (arrays of one element)."""
    x = np.asarray(x, dtype=np.float64)
    B, K = x.shape
    e = np.exp(x)
    p = e / e.sum(axis=1, keepdims=True)
    rp = 2 * EXPF + (K + 3) * U
    o = Ref(p, rp * p)
    if y is not None:
        y = np.asarray(y, dtype=np.float64)
        pick = (p * y).sum(axis=1)
        lb = -np.log(pick)
        rd = rp + (K + 1) * U
        el = -np.log1p(-rd) + LOGF * np.abs(lb)
        loss = lb.sum() / B
        o.loss = np.array([loss])
        o.eloss = np.array([el.sum() / B + EPS * (B + 20) * np.abs(lb).sum() / B + U * abs(loss)])
    return o


def softmax_bwd(p_stored, y):
    """dx from the P the device stored."""
    B = p_stored.shape[0]
    ref = (np.asarray(p_stored, dtype=np.float64) - np.asarray(y, dtype=np.float64)) / B
    return Ref(ref, 3 * U * (1 + 2 * U) * np.abs(ref))


# ---------------------------------------------------------------------------------------------------------
# dense layer
# ---------------------------------------------------------------------------------------------------------

# (B, IN, OUT): row tiles 64 x 64; see the module docstring for the rules
DENSE = {
    "d1": (1, 4, 4),        # one row, one ragged tile everywhere, a single k-tile; vector loaders
    "d2": (3, 20, 33),      # OUT % 4 != 0: scalar loaders and scalar epilogue; B <= 32: one split
    "d3": (65, 64, 132),    # ragged second row tile (1 row), third column tile of 4; wgrad config 6 (IN <= 64 < OUT):
    #                         two 128-column tiles, 3 splits of one 32-row k-tile, the last with one row
    "d4": (65, 62, 130),    # the same tiles on the scalar loaders (IN, OUT % 4 != 0)
    "d5": (70, 132, 12),    # reduction 132 > 128: row config 8 forward, config 6 dgrad over three column tiles of dx;
    #                         wgrad config 1 (IN > 64), three row tiles, 3 splits
    "d6": (33, 520, 10),    # 17 k-tiles of 32, the last holding 8; dgrad reduction 10 in one ragged k-tile
}
DENSE_OFFSET_IN = "d3"      # x, w, dy at a 4-byte offset: vec_ok false by pointer alone
DENSE_OFFSET_OUT = "d3"     # y and bias (dx, dw) at a 4-byte offset: the epilogue's scalar store


def dense_inputs(name):
    B, IN, OUT = DENSE[name]
    rng = np.random.RandomState(25000 + list(DENSE).index(name))
    d = dict(B=B, IN=IN, OUT=OUT, name=name)
    d["x"], d["dy"] = bf16_values(rng.randn(B, IN)), bf16_values(rng.randn(B, OUT))
    d["w"] = (rng.randn(IN, OUT) / np.sqrt(IN)).astype(f32)
    d["bias"] = rng.randn(OUT).astype(f32)
    return d


def dense_wgrad_config(IN, OUT):
    return 6 if IN <= 64 < OUT else 1


def dense_fwd(d, bias):
    w = d["w"].astype(np.float64)
    y, ya = d["x"] @ w, np.abs(d["x"]) @ np.abs(w)
    if bias:
        b = d["bias"].astype(np.float64)[None, :]
        y, ya = y + b, ya + np.abs(b)
    return Ref(y, STEP * (d["IN"] + 3) * ya)


def dense_dgrad(d):
    w = d["w"].astype(np.float64)
    return Ref(d["dy"] @ w.T, STEP * (d["OUT"] + 3) * (np.abs(d["dy"]) @ np.abs(w).T))


def dense_wgrad(d, l2):
    dw = d["x"].T @ d["dy"] + l2 * d["w"].astype(np.float64)
    return Ref(dw, STEP * (d["B"] + 2) * (np.abs(d["x"]).T @ np.abs(d["dy"])) + 2 * U * np.abs(dw))


# ---------------------------------------------------------------------------------------------------------
# exact kernels
# ---------------------------------------------------------------------------------------------------------

EXACT_N = (1, 3, 4, 5, 1027)        # under a float4; a whole one; one + a tail; 256 float4s + a tail of 3

_SPECIAL_BITS = (
    0x00000000, 0x80000000,                 # +0, -0
    0x00000001, 0x80000001,                 # the smallest subnormals
    0x007FFFFF, 0x807FFFFF,                 # the largest subnormals
    0x00800000, 0x80800000,                 # the smallest normals
    0x7F800000, 0xFF800000,                 # +inf, -inf
    0x7FC00001, 0xFFC00001,                 # quiet NaNs with low payload bits
    0x3F808000, 0x3F818000,                 # bf16 ties: 1 + 2^-8 (down to even), 1 + 3 * 2^-8 (up to even)
    0xBF808000, 0xBF818000,                 # the same, negative
    0x3F808001, 0x3F807FFF,                 # one bit above / below a tie
    0x7F7FFFFF, 0xFF7FFFFF,                 # the largest finite values: round to +-inf in bf16
    0x00008000, 0x00018000,                 # subnormal ties (to +0, and up to 2 * 2^-133)
    0x3F800000, 0xC0490FDB,                 # 1, -pi
)


def special_values(n=None):
    """The special-value vector as fp32 (24 entries, 4-wide route), or its first n (n = 23: the casts' whole-array
    scalar fallback, and a tail of 3 for the others)."""
    v = np.array(_SPECIAL_BITS, dtype=np.uint32).view(f32)
    return v if n is None else v[:n].copy()


def special_partner():
    """The second operand of add on the special vector: cancels to -0 + +0, rounds subnormal sums, inf - inf."""
    bits = (0x80000000, 0x80000000, 0x00000001, 0x00000001, 0x00000001, 0x00800000, 0x80000001, 0x00000003,
            0xFF800000, 0xFF800000, 0x3F800000, 0x7F800000, 0x33800000, 0x33800000, 0x3F800000, 0x3F800000,
            0x00000000, 0x80000000, 0x7F7FFFFF, 0x7F7FFFFF, 0x00008000, 0x80018000, 0xBF800000, 0x40490FDB)
    return np.array(bits, dtype=np.uint32).view(f32)


SCALES = (f32(0.5), f32(-1e-3), f32(3.0))       # 0.5: subnormal results are halved and rounded to even


def relu_fwd(x):
    """(y, mask).  v > 0 is decided on the bit pattern (a positive, non-NaN word), so that a host thread left in
    denormals-are-zero mode (tests/_optim_twin.ieee_host) decides a subnormal as IEEE does."""
    x = np.ascontiguousarray(x, dtype=f32)
    bits = x.view(np.int32)
    pos = (bits > 0) & (bits <= 0x7F800000)
    return np.where(pos, x, f32(0)), pos.astype(np.uint8)


def relu_bwd(dy, mask):
    return np.where(np.asarray(mask) != 0, np.asarray(dy, dtype=f32), f32(0))


def add(a, b, relu):
    """(y, mask); mask None without ReLU."""
    with ieee_host(), np.errstate(invalid="ignore", over="ignore"):
        v = np.asarray(a, dtype=f32) + np.asarray(b, dtype=f32)
    if not relu:
        return v, None
    return relu_fwd(v)


def scale(x, s):
    with ieee_host(), np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return f32(s) * np.asarray(x, dtype=f32)


def mask_to_f32(mask):
    return np.where(np.asarray(mask) != 0, f32(1), f32(0))


def same_bits(got, want):
    """Bitwise equality of fp32 arrays, except that a NaN in want asks for a NaN (any payload) in got."""
    got, want = np.ascontiguousarray(got, dtype=f32), np.ascontiguousarray(want, dtype=f32)
    nan = np.isnan(want)
    return bool(got.shape == want.shape and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
                and np.isnan(got[nan]).all())


def same16(got, want):
    """same_bits for bf16 bit patterns (uint16 / int16 arrays)."""
    return same_bits(widen16(np.asarray(got).view(np.uint16)), widen16(np.asarray(want).view(np.uint16)))


# dk_nchw_to_nhwc_f32: (N, C, H, W, Cp, y misaligned)
NCHW = {
    "l1": (2, 3, 5, 7, 4, False),       # the 4-wide kernel (Cp = 4, C <= 4, aligned y)
    "l2": (2, 3, 5, 7, 4, True),        # the same with y at a 4-byte offset: the general kernel
    "l3": (2, 1, 5, 7, 4, False),       # one channel, three pad lanes
    "l4": (2, 5, 5, 7, 8, False),       # C = 5 in Cp = 8: the general kernel with padding
    "l5": (2, 6, 5, 7, 6, False),       # C = Cp = 6: no padding
}
UNPAD = {"u1": (70, 4, 3), "u2": (70, 8, 5)}    # (P, Cp, C): P C = 210 / 350, the second over one block


def nchw_to_nhwc(x, Cp):
    N, C, H, W = x.shape
    y = np.zeros((N, H, W, Cp), dtype=f32)
    for n in range(N):
        for c in range(C):
            y[n, :, :, c] = x[n, c]
    return y


def nhwc_unpad(x, C):
    return np.ascontiguousarray(x[:, :C])


def layout_input(shape, seed):
    return np.random.RandomState(26000 + seed).randn(*shape).astype(f32)


def case_tensor_sizes():
    """{case: the largest tensor's element count} over every table (the cap of tests/test_head_ref_host.py)."""
    out = {}
    for k, (N, HW, C) in GAP.items():
        out[k] = N * HW * C
    for k, (M, N) in COLSUM.items():
        out[k] = M * N
    for n in L2_N:
        out["l2-%d" % n] = n
    for k, (sizes, _) in L2_TABLES.items():
        out[k] = max(sizes)
    for k, c in SOFTMAX.items():
        out[k] = c.B * c.K
    for k, (B, IN, OUT) in DENSE.items():
        out[k] = max(B * IN, B * OUT, IN * OUT)
    for n in EXACT_N:
        out["exact-%d" % n] = n
    for k, (N, C, H, W, Cp, _) in NCHW.items():
        out[k] = N * H * W * max(C, Cp)
    for k, (P, Cp, C) in UNPAD.items():
        out[k] = P * Cp
    return out
