"""numpy float32 twin of the activations beyond ReLU (dorknet_amd/csrc/act_math.h, activations.hip, and
act_bwd_bn_partial_kernel in batchnorm.hip), the per-element bounds the twin itself is held to against torch CPU fp64
(tests/test_activation_host.py), and the fixed inputs of the GPU cases (tests/test_gpu_activations.py).  Host only:
numpy + torch-CPU, nothing from dorknet_amd, no GPU call.

The rules (v the layer input, g = dy * act'(v)); every fp32 operation is rounded once on its own, in this order:
    LeakyReLu  y = v > 0 ? v : alpha * v                          g = v > 0 ? dy : alpha * dy
    ReLu6      t = v < 0 ? 0 : v;  y = t > 6 ? 6 : t              g = (v > 0 and v < 6) ? dy : 0
    HardSwish  y = v <= -3 ? 0 : v >= 3 ? v : (v * (v + 3)) * SIXTH
               g = v <= -3 ? 0 : v >= 3 ? dy : dy * ((2 * v + 3) * SIXTH)          SIXTH = fl32(1 / 6)
    SiLu       z = exp_neg_abs(v);  d = 1 + z;  s = v >= 0 ? 1 / d : z / d;  y = v * s
               g = dy * (s * (1 + v * (1 - s)))
    exp_neg_abs(v) = e^-min(|v|, 80):
               a = |v|, 80 unless a <= 80;  kf = (a * LOG2E + 1.5 * 2^23) - 1.5 * 2^23  (= rint(a * LOG2E))
               r = (a - kf * C1) - kf * C2,  C1 = 0.693359375,  C2 = fl32(ln 2 - C1);  t = -r
               p = 1/5040;  p = p * t + c for c in 1/720, 1/120, 1/24, 1/6, 1/2, 1, 1   (each constant fl32)
               z = p * 2^-kf  (the power of two from the exponent field: exact, kf <= 115 so nothing is subnormal)
The kinks follow torch (F.leaky_relu, F.relu6, F.hardswish, F.silu): derivative alpha at 0; 0 at 0 and at 6;
0 at -3 and 1 at 3 (torch's hardswish backward takes (2 v + 3) / 6 on the open interval only).

Special values, as the rules give them:
    NaN          y and g are NaN, except LeakyReLu's g = alpha dy and ReLu6's g = 0 (the comparisons fail).  (The
                 payload bits of a NaN are not part of the rule: the GPU test compares where the NaNs are, not
                 their bits.)
    +0 / -0      LeakyReLu y = alpha * v; ReLu6 y = v; HardSwish y = (v * 3) * SIXTH; SiLu y = v * 0.5: a zero of
                 the input's sign (of alpha's times the input's for LeakyReLu).  g = alpha dy; 0; dy * 0.5; dy * 0.5.
    +inf         y = +inf (ReLu6: 6); g = dy (ReLu6: 0); SiLu's g is NaN (inf * (1 - 1)).
    -inf         LeakyReLu y = alpha * -inf, g = alpha dy; ReLu6 y = 0, g = 0; HardSwish y = 0, g = 0 (the v <= -3
                 branch, no -inf * 0); SiLu y = -inf, g = dy * -inf: the sigmoid is clamped at e^-80, not 0.
    |v| = 1e4    all finite: SiLu has s = 1, g = dy for +1e4 and s = e^-80, y = -1e4 e^-80, g = dy * (s * -9999)
                 for -1e4.
bf16 storage: operands widened (exact), the fp32 rule, one round-to-nearest-even per stored value (_dw_ref.rne_bf16).
Under BatchNorm on load v = bn_relu_out(x) (an fma: gamma * x_hat + beta, as dk_bn_apply_*), rounded to bf16 first
for bf16 storage.

Bounds of the twin against fp64, u = 2^-24 (none fitted; tests/test_activation_host.py asserts them and DESIGN.md
section 23 records the measured worst error / bound).  alpha is the fp32 value in both.
    Every bound on y carries TINY = 2^-149 besides: a product below 2^-126 is rounded to the subnormal grid.
    LeakyReLu  y: one product, u |y|.  g (dy = 1): exact.
    ReLu6      y and g exact.
    HardSwish  y: v + 3, the product, the product by SIXTH (itself within u / 2 relative of 1 / 6): 4 u |y|
               (v >= 3: y = v against fp64's v * 6 / 6, within the same bound; v <= -3: 0).   g: 2 v exact, + 3, * SIXTH (+ its own
               error), dy = 1: 3 u |g|.
    SiLu       z: t = a * LOG2E only picks k (|r| <= 0.35 either way).  k * C1 is exact (C1 has 9 significant bits,
               k 7) and so is a - k * C1 (Cody-Waite); k * C2 and the second subtraction round once each and C2
               carries its own representation error: |dr| <= u (0.027 + 0.35 + 0.027) < 0.5 u, a relative error
               of e^-r of 0.5 u.  Taylor remainder at |t| <= 0.35: 0.35^8 / 8! / 0.70 < 0.1 u.  Horner: seven
               (multiply, add) pairs on values of at most 1.42, each pair 2 u relative to its result, reaching p
               through at most |t|^j: 2 u 1.42 / (1 - 0.35) = 4.4 u absolute, / p >= 0.70 -> 6.3 u; the constants'
               own errors (u / 2 each, times |t|^j / j!-sized terms) fit in the same geometric sum.  The scaling is
               exact.  EZ = 7 u relative.
               d = 1 + z and the division: u each.  s = 1 / d: EZ z / (1 + z) + 2 u;  s = z / d: EZ / (1 + z) + 2 u
               (relative; ES below, per element).  The clamp substitutes e^-80 for e^-|v| beyond 80: an absolute
               error of s of at most CLAMP = 1.81e-35, carried as |v| CLAMP (y) and (1 + |v|)^2 CLAMP (g).
               y = v s: (ES + u) |y|.
               g: q = 1 - s: ES s + u |q|;  w = v q: |v| (that) + u |w|;  h = 1 + w: + u |h|;
               m = s h: s err(h) + ES s |h| + u |m|;  dy = 1.
"""
import numpy as np

from tests._dw_ref import U, rne_bf16

f32 = np.float32

LEAKY, RELU6, HARDSWISH, SILU = 0, 1, 2, 3
KINDS = {"LeakyReLu": LEAKY, "ReLu6": RELU6, "HardSwish": HARDSWISH, "SiLu": SILU}
KINKS = {LEAKY: (0.0,), RELU6: (0.0, 6.0), HARDSWISH: (-3.0, 3.0), SILU: ()}
KINK_MARGIN = 2.0 ** -10   # no |v - kink| below this in a seeded case: far above any fp32 evaluation error of v there

SIXTH = f32(1.0) / f32(6.0)
LOG2E = f32(1.4426950408889634)
C1 = f32(0.693359375)
C2 = f32(-2.12194441701285541057586669921875e-4)   # fl32(ln 2 - C1)
SHIFT = f32(12582912.0)
POLY = tuple(f32(c) for c in (1 / 5040, 1 / 720, 1 / 120, 1 / 24)) + (SIXTH, f32(0.5), f32(1.0), f32(1.0))
CLAMP = 1.81e-35   # >= e^-80
EZ = 7 * U
TINY = 2.0 ** -149


def exp_neg_abs(v):
    """e^-min(|v|, 80) in float32, the kernel's operations in their order."""
    v = np.asarray(v, dtype=f32)
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.where(v < 0, -v, v).astype(f32)
        a = np.where(a <= f32(80.0), a, f32(80.0)).astype(f32)
        kf = (a * LOG2E + SHIFT) - SHIFT
        r = (a - kf * C1) - kf * C2
        t = -r
        p = np.full(v.shape, POLY[0], dtype=f32)
        for c in POLY[1:]:
            p = p * t + c
        scale = ((127 - kf.astype(np.int64)) << 23).astype(np.uint32).view(f32)
        z = p * scale
    assert z.dtype == f32
    return z


def sigmoid(v):
    v = np.asarray(v, dtype=f32)
    z = exp_neg_abs(v)
    d = f32(1.0) + z
    return np.where(v >= 0, f32(1.0) / d, z / d).astype(f32)


def forward(kind, v, alpha=0.01):
    """y = act(v), float32 in and out."""
    v = np.asarray(v, dtype=f32)
    al = f32(alpha)
    with np.errstate(invalid="ignore", over="ignore"):
        if kind == LEAKY:
            y = np.where(v > 0, v, al * v)
        elif kind == RELU6:
            t = np.where(v < 0, f32(0.0), v)
            y = np.where(t > 6, f32(6.0), t)
        elif kind == HARDSWISH:
            y = np.where(v <= -3, f32(0.0), np.where(v >= 3, v, (v * (v + f32(3.0))) * SIXTH))
        else:
            y = v * sigmoid(v)
    return y.astype(f32)


def backward(kind, v, dy, alpha=0.01):
    """g = dy * act'(v), float32 in and out."""
    v, dy = np.asarray(v, dtype=f32), np.asarray(dy, dtype=f32)
    al = f32(alpha)
    with np.errstate(invalid="ignore", over="ignore"):
        if kind == LEAKY:
            g = np.where(v > 0, dy, al * dy)
        elif kind == RELU6:
            g = np.where((v > 0) & (v < 6), dy, f32(0.0))
        elif kind == HARDSWISH:
            g = np.where(v <= -3, f32(0.0), np.where(v >= 3, dy, dy * ((f32(2.0) * v + f32(3.0)) * SIXTH)))
        else:
            s = sigmoid(v)
            g = dy * (s * (f32(1.0) + v * (f32(1.0) - s)))
    return g.astype(f32)


def to_bf16(a):
    """float32 values rounded to bf16 (nearest even), as float32."""
    return rne_bf16(np.asarray(a, dtype=np.float64)).astype(f32)


def bf16_bits(a):
    """The uint16 storage of bf16-representable float32 values."""
    return (np.ascontiguousarray(a, dtype=f32).view(np.uint32) >> 16).astype(np.uint16)


def from_bf16_bits(b):
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(f32)


def forward_stored(kind, v, alpha, bf16):
    y = forward(kind, v, alpha)
    return to_bf16(y) if bf16 else y


def backward_stored(kind, v, dy, alpha, bf16):
    g = backward(kind, v, dy, alpha)
    return to_bf16(g) if bf16 else g


def bn_v(x, bn, relu, bf16):
    """(v, dead): the forward's v = bn_relu_out(x) from the BatchNorm's raw input x[P][C] -- gamma * x_hat + beta as one
    fma (float64 holds the product of two float32 values exactly, so one rounding of the float64 sum is the fma,
    short of a double-rounding tie no case relies on) -- rounded to bf16 for bf16 storage; dead: where a fused ReLU
    killed it."""
    m, i, ga, be = (np.asarray(p, dtype=f32)[None, :] for p in bn[:4])
    x = np.asarray(x, dtype=f32)
    xh = ((x - m) * i).astype(f32)
    r = (ga.astype(np.float64) * xh.astype(np.float64) + be.astype(np.float64)).astype(f32)
    dead = (~(r > 0)) if relu else np.zeros(r.shape, dtype=bool)
    v = np.where(dead, f32(0.0), r).astype(f32)
    return (to_bf16(v) if bf16 else v), dead, xh


def partial_sums(g, x, bn, rows):
    """(part, apart): part[rows][2][C] = (sum g, sum g x_hat) in fp64 over row r's pixel range [r ppb, (r + 1) ppb),
    ppb = ceil(P / rows), summed in extended precision and rounded once, of the stored gradient g[P][C], x_hat = (x - mean) * invstd formed in fp32 and every product
    widened to fp64 first (exact); apart the same sums of absolute values (for _bn_ref.sum_bound)."""
    m, i = (np.asarray(p, dtype=f32)[None, :] for p in bn[:2])
    xh = ((np.asarray(x, dtype=f32) - m) * i).astype(f32).astype(np.float64)
    g64 = np.asarray(g, dtype=f32).astype(np.float64)
    P, C = g64.shape
    ppb = -(-P // rows)
    part, apart = np.zeros((rows, 2, C)), np.zeros((rows, 2, C))
    gl, tl = g64.astype(np.longdouble), (g64 * xh).astype(np.longdouble)   # (the products are exact in fp64)
    for r in range(rows):
        sl = slice(r * ppb, min(P, (r + 1) * ppb))
        part[r, 0], part[r, 1] = gl[sl].sum(axis=0), tl[sl].sum(axis=0)
        apart[r, 0], apart[r, 1] = np.abs(gl[sl]).sum(axis=0), np.abs(tl[sl]).sum(axis=0)
    return part, apart


def backward_bnx(kind, x, dy, bn, relu, alpha, bf16, rows, v=None, dead=None):
    """(g, part, apart): dk_act_bwd_bnx_*'s stored gradient [P][C] (float32 values) -- dy * act'(v), +0 where a fused
    ReLU killed v -- and its partial sums.  v / dead: the forward's v and the ReLU's decisions where the caller has
    them (the GPU test takes them from dk_bn_apply_*), else bn_v's."""
    if v is None:
        v, dead, _ = bn_v(x, bn, relu, bf16)
    g = backward_stored(kind, v, dy, alpha, bf16)
    g = np.where(dead, f32(0.0), g).astype(f32)
    return (g, *partial_sums(g, x, bn, rows))


# -- the twin's own bounds against fp64 ---------------------------------------------------------------------

def reference(kind, v, alpha=0.01):
    """(y, act') by torch CPU fp64 autograd over the F.* function; alpha the fp32 value."""
    import torch
    import torch.nn.functional as F
    t = torch.tensor(np.asarray(v, dtype=np.float64), requires_grad=True)
    fn = {LEAKY: lambda a: F.leaky_relu(a, float(f32(alpha))), RELU6: F.relu6, HARDSWISH: F.hardswish,
          SILU: F.silu}[kind]
    y = fn(t)
    y.backward(torch.ones_like(y))
    return y.detach().numpy(), t.grad.numpy()


def bounds(kind, v, alpha=0.01):
    """(bound on |y - ref|, bound on |act' - ref|) per element, from the operation counts in the module docstring."""
    v = np.asarray(v, dtype=np.float64)
    y, d = reference(kind, v, alpha)
    if kind == LEAKY:
        return U * np.abs(y) + TINY, np.zeros_like(v)
    if kind == RELU6:
        return np.zeros_like(v), np.zeros_like(v)
    if kind == HARDSWISH:
        return 4 * U * np.abs(y) + TINY, 3 * U * np.abs(d)
    z = np.exp(-np.abs(v))
    s = np.where(v >= 0, 1 / (1 + z), z / (1 + z))
    ES = np.where(v >= 0, EZ * z / (1 + z), EZ / (1 + z)) + 2 * U
    av = np.abs(v)
    by = (ES + U) * np.abs(y) + av * CLAMP + TINY
    q = 1 - s
    w = v * q
    h = 1 + w
    eq = ES * s + U * np.abs(q)
    ew = av * eq + U * np.abs(w)
    eh = ew + U * np.abs(h)
    bd = s * eh + ES * s * np.abs(h) + U * np.abs(s * h) + (1 + av) ** 2 * CLAMP
    return by, bd


EDGE_VALUES = (0.0, -0.0, 6.0, -3.0, 3.0, 1e4, -1e4, 80.0, -80.0, 87.0, -87.0, 1.0, -1.0)   # finite: held to the bounds
SPECIALS = (np.inf, -np.inf, np.nan)                                                         # stated, not bounded


def grid():
    """The float32 points the twin is checked on: 2^20 evenly spaced in [-30, 30], every bf16-representable value in
    [-100, 100], and the finite edge values."""
    lin = np.linspace(-30.0, 30.0, 2 ** 20).astype(f32)
    bits = np.arange(0, 1 << 16, dtype=np.uint32)
    bf = (bits << 16).view(f32)
    bf = bf[np.isfinite(bf) & (np.abs(bf) <= 100) & ((np.abs(bf) >= 2.0 ** -126) | (bf == 0))]
    return np.concatenate([lin, bf, np.asarray(EDGE_VALUES, dtype=f32)])


# -- the GPU cases' inputs ----------------------------------------------------------------------------------------------

def kink_margin(kind, v):
    """The least |v - kink| over the finite elements (inf without a kink)."""
    v = np.asarray(v, dtype=np.float64)
    v = v[np.isfinite(v)]
    return min([float(np.abs(v - k).min()) for k in KINKS[kind]] + [np.inf]) if v.size else np.inf


def seeded(kind, make):
    """(seed, value): make(seed) at the first seed of 0, 1, 2, ... whose values keep KINK_MARGIN from every kink."""
    for seed in range(1000):
        val = make(seed)
        if kink_margin(kind, val[0] if isinstance(val, tuple) else val) >= KINK_MARGIN:
            return seed, val
    raise AssertionError("no seed below 1000 keeps the kink margin")


def entry_inputs(kind, shape, seed):
    """v and dy (float32, bf16-representable so both storage types see the same values) of an entry case: normal
    values of scale 3 about the kinks."""
    rng = np.random.RandomState(23000 + 101 * kind + seed)
    n = int(np.prod(shape))
    v = to_bf16(3.0 * rng.randn(n)).reshape(shape)
    dy = to_bf16(rng.randn(n)).reshape(shape)
    return v, dy


def with_edges(v, nan=True):
    """v with its leading elements replaced by +-0, the kink values, +-inf, +-1e4 (bf16: 9984) and NaN."""
    edge = [0.0, -0.0, 6.0, -3.0, 3.0, np.inf, -np.inf, 1e4, -1e4] + ([np.nan] if nan else [])
    out = np.array(v, dtype=f32).ravel()
    out[:len(edge)] = to_bf16(np.asarray(edge, dtype=f32))
    return out.reshape(np.shape(v))
