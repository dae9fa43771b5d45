"""fp64 reference of a depthwise layer and the per-element error bounds its fp32 / bf16 kernels are held
to (tests/test_dw_ref_host.py, tests/test_gpu_dw_elementwise.py).  Host only: numpy + torch-CPU, nothing
from dorknet_amd, no GPU call.

Operation (depthwise_convolution.py:85-121, :198-221; oracle.ref.depthwise_forward / _backward):
    a  = bn(x) (+ ReLU) where an input BatchNorm is applied on load, else x; zero padding after it
    y  = sum_{r,s} w[c,r,s] a[n,c,oh st + r - pad, ow st + s - pad] + bias[c]
    dx = sum over the taps that reach the pixel of w * dy (+ residual)
    dw = sum_{n,oh,ow} dy * a (+ l2 * w)

Every quantity comes with its "absolute twin" -- the same code on absolute values -- which is the scale
of the rounding error of any evaluation order:  ya = |w| (*) |a| + |bias|, dxa = dgrad(|dy|, |w|) + |res|,
dwa = sum |dy| |a|.

Bounds on |got - ref| per element, none excluded (u = 2^-24):
    y, dx stored in fp32   A = (n + 1) u ya + E,  n = R S + 2 roundings (R S taps, the bias or residual add,
                           one spare), the +1 the first-order slack of (1 + u)^n;  E = |w| (*) ea is the
                           operand's own error scale (0 for exact operands)
    y, dx stored in bf16   one round-to-nearest-even store of a value v within A of ref.  Rounding is monotone,
                           so the stored value lies between rne(ref - A) and rne(ref + A):
                           max(rne(ref + A) - ref, ref - rne(ref - A)), which is never more than the looser
                           closed form 2^-8 (|ref| + A) + A (a half ulp of v is at most 2^-8 |v|); bf16_bound
                           takes the smaller of the two per element.  The closed form alone cannot tell a
                           truncating store from a rounding one by more than a factor of 2 (one ulp against
                           a half); the interval can, wherever ref lies just below a bf16 value
    dw (fp32)              u (nw dwa + 2 |ref|) + sum |dy| ea,  nw = N OH OW terms in any grouping, 2 |ref|
                           the final cast and the l2 fma
BatchNorm on load: a is bn_out (dk_common.h:180-183) in fp64 from the fp32 parameters, its fp32 evaluation
error scale ea = 4 u (|gamma x_hat| + |beta|) (three roundings on gamma x_hat, one on the sum); ReLU is
1-Lipschitz, so the same scale holds after it and no element needs excluding.
The fused backward's dy = gamma invstd (g mask - k1 - x_hat k2) (bn_bwd_elem, dk_common.h:189-197) has the
error scale ed = 6 u |gamma invstd| (|g| + |k1| + |x_hat k2|); it enters as E = |w| (*) ed for dx and as
sum |a| ed for dw.

Inputs (make_inputs): activations are bf16-representable, so the fp32 and the bf16 entry points see the
same values and the reference needs no rounding emulation; filters, bias and BatchNorm vectors are
arbitrary fp32."""
import numpy as np
import torch

U = 2.0 ** -24
UB = 2.0 ** -8


def out_hw(H, W, R, S, stride, pad):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1


def bf16_values(a):
    """Round to bf16 (nearest even) and widen to fp64."""
    return torch.as_tensor(np.asarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


def _padded(a, pad):
    return np.pad(a, ((0, 0), (0, 0), (pad, pad), (pad, pad))) if pad else a


def conv(a, w, stride, pad, bias=None):
    """y of the layer, fp64.  a (N,C,H,W), w (C,R,S)."""
    C, R, S = w.shape
    OH, OW = out_hw(a.shape[2], a.shape[3], R, S, stride, pad)
    ap = _padded(a, pad)
    y = np.zeros((a.shape[0], C, OH, OW))
    for r in range(R):
        for s in range(S):
            y += w[:, r, s][None, :, None, None] * ap[:, :, r:r + stride * OH:stride, s:s + stride * OW:stride]
    if bias is not None:
        y = y + bias[None, :, None, None]
    return y


def dgrad(dy, w, stride, pad, H, W, res=None):
    """dx of the layer, fp64.  dy (N,C,OH,OW)."""
    C, R, S = w.shape
    N, _, OH, OW = dy.shape
    dxp = np.zeros((N, C, H + 2 * pad, W + 2 * pad))
    for r in range(R):
        for s in range(S):
            dxp[:, :, r:r + stride * OH:stride, s:s + stride * OW:stride] += dy * w[:, r, s][None, :, None, None]
    dx = dxp[:, :, pad:pad + H, pad:pad + W]
    return dx + res if res is not None else dx.copy()


def wgrad(dy, a, R, S, stride, pad):
    """sum_{n,oh,ow} dy * a per tap (without the l2 term), fp64."""
    N, C, OH, OW = dy.shape
    ap = _padded(a, pad)
    dw = np.zeros((C, R, S))
    for r in range(R):
        for s in range(S):
            dw[:, r, s] = (dy * ap[:, :, r:r + stride * OH:stride, s:s + stride * OW:stride]).sum(axis=(0, 2, 3))
    return dw


def bn_operand(x, bn):
    """(a, ea, pre): the BatchNorm (+ ReLU) output in fp64 from the fp32 parameters, its fp32 evaluation
    error scale, and the value before the ReLU.  bn = (mean, invstd, gamma, beta, relu) or None."""
    if bn is None:
        return x, np.zeros_like(x), x
    m, i, g, b = (np.asarray(v, dtype=np.float64)[None, :, None, None] for v in bn[:4])
    gx = g * ((x - m) * i)
    pre = gx + b
    ea = 4 * U * (np.abs(gx) + np.abs(b))
    return (np.maximum(pre, 0.0) if bn[4] else pre), ea, pre


def bn_operand_f32(x, bn):
    """bn_out's operation order in fp32 (what a correct kernel computes): ((x - mean) * invstd) * gamma + beta."""
    if bn is None:
        return np.asarray(x, dtype=np.float32)
    x = np.asarray(x, dtype=np.float32)
    m, i, g, b = (np.asarray(v, dtype=np.float32)[None, :, None, None] for v in bn[:4])
    a = g * ((x - m) * i) + b
    return np.where(a > 0, a, np.float32(0)) if bn[4] else a


def bn_bwd_dy(g, x1, out_bn, k12):
    """(dy, ed, pre): the following BatchNorm's backward apply in fp64 (bn_bwd_elem), its fp32 error scale,
    and that BatchNorm's output before the ReLU (the mask's decision variable; guard = its own fp32
    error scale 8 u (|gamma x_hat| + |beta|), see mask_margin).  out_bn = (mean, invstd, gamma, beta, relu)."""
    m, i, ga, b = (np.asarray(v, dtype=np.float64)[None, :, None, None] for v in out_bn[:4])
    C = g.shape[1]
    k1 = np.asarray(k12[:C], dtype=np.float64)[None, :, None, None]
    k2 = np.asarray(k12[C:], dtype=np.float64)[None, :, None, None]
    xh = (x1 - m) * i
    pre = ga * xh + b
    gm = g * (pre > 0) if out_bn[4] else g
    dy = ga * i * (gm - k1 - xh * k2)
    ed = 6 * U * np.abs(ga * i) * (np.abs(gm) + np.abs(k1) + np.abs(xh * k2))
    return dy, ed, pre


def mask_margin(x1, out_bn):
    """min over the elements of |bn(x1)| / (8 u (|gamma x_hat| + |beta|)): > 1 means no fp32 evaluation
    of bn(x1) can decide its ReLU mask differently from fp64."""
    m, i, ga, b = (np.asarray(v, dtype=np.float64)[None, :, None, None] for v in out_bn[:4])
    gx = ga * ((x1 - m) * i)
    return float((np.abs(gx + b) / (8 * U * (np.abs(gx) + np.abs(b)))).min())


def rne_bf16(v):
    """fp64 values rounded to the nearest bf16 (8 significant bits), ties to even, without an fp32 step
    in between (normal range)."""
    _, e = np.frexp(v)
    q = np.ldexp(1.0, e - 8)    # the bf16 ulp of v's binade: |v| / q is in [128, 256)
    return np.rint(v / q) * q


def bf16_bound(ref, A):
    """The bound on |stored - ref| for a bf16 store of a value within A of ref (module docstring)."""
    closed = UB * (np.abs(ref) + A) + A
    interval = np.maximum(rne_bf16(ref + A) - ref, ref - rne_bf16(ref - A))
    return np.minimum(closed, interval)


def bf16_closed(ref, A):
    """The closed form 2^-8 (|ref| + A) + A alone (checked and recorded next to bf16_bound, which implies it)."""
    return UB * (np.abs(ref) + A) + A


class Ref:
    """The fp64 results of one layer call and their bounds.  Fields: y, dx, dw (None where not asked for),
    by / bx / bw the fp32-storage bounds, by16 / bx16 the bf16-storage ones (by16c / bx16c: their closed form)."""


def reference(x, w, stride, pad, bias=None, bn=None, dy=None, res=None, l2=0.0, dy_err=None, want_dx=True):
    """x (N,C,H,W) and dy, res: fp64 arrays of bf16-representable values; w (C,R,S), bias: fp32 values.
    dy_err: the error scale of dy where it is itself computed in fp32 (the fused backward)."""
    w = np.asarray(w, dtype=np.float64)
    C, R, S = w.shape
    N, _, H, W = x.shape
    a, ea, _ = bn_operand(x, bn)
    wa = np.abs(w)
    n = R * S + 2
    o = Ref()
    o.a = a
    b64 = None if bias is None else np.asarray(bias, dtype=np.float64)
    o.y = conv(a, w, stride, pad, b64)
    ya = conv(np.abs(a), wa, stride, pad, None if b64 is None else np.abs(b64))
    o.by = (n + 1) * U * ya + conv(ea, wa, stride, pad)
    o.by16, o.by16c = bf16_bound(o.y, o.by), bf16_closed(o.y, o.by)
    o.dx = o.dw = None
    if dy is not None:
        ed = np.zeros_like(dy) if dy_err is None else dy_err
        if want_dx:
            o.dx = dgrad(dy, w, stride, pad, H, W, res)
            dxa = dgrad(np.abs(dy), wa, stride, pad, H, W, None if res is None else np.abs(res))
            o.bx = (n + 1) * U * dxa + dgrad(ed, wa, stride, pad, H, W)
            o.bx16, o.bx16c = bf16_bound(o.dx, o.bx), bf16_closed(o.dx, o.bx)
        o.dw = wgrad(dy, a, R, S, stride, pad) + l2 * w
        dwa = wgrad(np.abs(dy), np.abs(a), R, S, stride, pad)
        nw = dy.shape[0] * dy.shape[2] * dy.shape[3]
        o.bw = (U * (nw * dwa + 2 * np.abs(o.dw)) + wgrad(np.abs(dy), ea, R, S, stride, pad)
                + wgrad(ed, np.abs(a), R, S, stride, pad))
    return o


def worst(got, ref, bound):
    """(ratio, index): the largest |got - ref| / bound over every element; an error where the bound is 0
    (an output no tap reaches must be exactly 0) counts as infinite, as does a NaN."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    k = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[k]), tuple(int(v) for v in k)


def check(name, got, ref, bound, tag="dw"):
    """Assert every element within its bound; returns the worst ratio (logged under the family's tag)."""
    from tests._convert import log_ratio
    r, k = worst(got, ref, bound)
    log_ratio(name, r, tag)
    assert r <= 1.0, "{}: element {} got {!r} want {!r} bound {:.3e} (err / bound = {:.3g})".format(
        name, k, float(np.asarray(got)[k]), float(ref[k]), float(bound[k]), r)
    return r


# Geometries: R = S, stride, pad, N, H, W, C -- each the smallest shape reaching the named edge
# (TW = 4 outputs per thread along W (2 at stride 2), fp32 row segments of at most 14, bf16 whole columns,
# weight-gradient segments of 8 rows, 4 sub-pixel quads per thread).
GEOMS = {
    1: (3, 1, 1, 2, 15, 9, 8),      # two fp32 segments (8 + 7); ragged column chunk (9 = 4 + 4 + 1)
    2: (3, 1, 0, 2, 13, 11, 8),     # no padding; the dgrad is the forward with padding 2
    3: (3, 1, 2, 1, 5, 6, 8),       # pad = R - 1: output larger than input; dgrad padding 0
    4: (3, 1, 1, 2, 30, 5, 64),     # three segments of 10; two wgrad segments + a ragged third
    5: (3, 1, 1, 1, 1, 1, 8),       # one pixel: eight of the nine taps are padding
    6: (3, 1, 1, 1, 3, 3, 1028),    # C / 4 = 257: wgrad's second channel block; statistics unsupported
    7: (3, 2, 1, 2, 29, 7, 8),      # stride 2, odd H and W; OH = 15; partial last quad row and column
    8: (3, 2, 1, 1, 14, 18, 8),     # even H and W; nine quad columns: the last 4-quad chunk holds one
    9: (3, 2, 0, 1, 10, 11, 24),    # stride 2 without padding: gather dgrad; last row / column get nothing
    10: (5, 1, 2, 2, 11, 11, 12),   # 5x5 ring window; C / 4 = 3 does not divide 256: no statistics
    11: (5, 1, 0, 2, 9, 10, 8),     # dgrad padding 4
    12: (5, 2, 2, 2, 13, 12, 8),    # 5x5 sub-pixel dgrad
    13: (5, 2, 2, 1, 9, 9, 8),      # the same with odd H and W
    14: (1, 1, 0, 2, 6, 5, 8),      # 1x1, stride 1
    15: (1, 2, 0, 2, 9, 8, 4),      # 1x1, stride 2: phases without taps write zeros; one channel group
}


def make_inputs(gid, seed=0):
    """Fixed inputs of geometry gid: dict of x, dy, res (fp64, bf16-representable), w, bias, bn (fp32)."""
    R, stride, pad, N, H, W, C = GEOMS[gid]
    rng = np.random.RandomState(1000 * seed + gid)
    OH, OW = out_hw(H, W, R, R, stride, pad)
    d = dict(R=R, stride=stride, pad=pad, N=N, H=H, W=W, C=C, OH=OH, OW=OW)
    d["x"] = bf16_values(rng.randn(N, C, H, W))
    d["dy"] = bf16_values(rng.randn(N, C, OH, OW))
    d["res"] = bf16_values(rng.randn(N, C, H, W))
    d["w"] = (rng.randn(C, R, R) * 0.5).astype(np.float32)
    d["bias"] = rng.randn(C).astype(np.float32)
    d["bn"] = bn_params(C, rng)
    return d


def bn_params(C, rng):
    """(mean, invstd, gamma, beta) fp32 vectors of a BatchNorm with non-trivial affine parameters."""
    return tuple(v.astype(np.float32) for v in
                 (rng.randn(C) * 0.3, rng.rand(C) + 0.5, 1 + 0.3 * rng.randn(C), 0.2 * rng.randn(C)))


# The fused stride-1 backward (dk_dwconv_bwd_bnbwd_*): 3x3, stride 1, pad 1; N, H, W, C
FUSED = {
    1: (2, 15, 9, 8),       # geometry 1
    4: (2, 30, 5, 64),      # geometry 4
    20: (2, 13, 19, 64),    # W >= 12, C / 4 a multiple of 16: two columns per thread
}


def make_fused_inputs(fid, relu):
    """Fixed inputs of a fused-backward case: g, x1 (the gradient and the raw input of the following
    BatchNorm), x, res (bf16-representable fp64); po / pi the following / input BatchNorm's fp32 vectors,
    k12 its folded backward coefficients, w the filters.  The seed fixes the ReLU-mask precondition
    (mask_margin > 1, tests/test_dw_ref_host.py)."""
    N, H, W, C = FUSED[fid]
    rng = np.random.RandomState(7000 + 10 * fid + relu)
    d = dict(R=3, stride=1, pad=1, N=N, H=H, W=W, C=C, OH=H, OW=W)
    for k in ("g", "x1", "x", "res"):
        d[k] = bf16_values(rng.randn(N, C, H, W))
    d["po"] = bn_params(C, rng) + (relu,)
    d["pi"] = bn_params(C, rng)
    d["k12"] = (rng.randn(2 * C) * 0.1).astype(np.float32)
    d["w"] = (rng.randn(C, 3, 3) * 0.3).astype(np.float32)
    return d
