"""Shared helpers for the BatchNorm partial-row tests (tests/test_gpu_fold.py,
tests/test_gpu_partial_rows.py).

A producer writes fp64 partial rows part[rows][2][C] next to its output; the caller sizes that
buffer from a separate dk_*_rows() query and a fold reduces all `rows` rows.  check_stats /
check_bwd compare an armed in-launch fold with the separate fold launch; the TABLE lists every
producer with its row query, a launch closure and a plain torch fp64 reference for the [2][C]
sums (tests/test_gpu_partial_rows.py runs the checks)."""
import contextlib

import numpy as np
import torch

from dorknet_amd._hip import DK_FOLDED, lib, stream_handle

EPS, MOM = 1e-5, 0.9
F32, BF16 = torch.float32, torch.bfloat16
CL = torch.channels_last


def nhwc(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda").contiguous(
        memory_format=torch.channels_last)


def vec(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def bn_params(C, rng):
    return [vec(v) for v in (rng.randn(C) * 0.3, rng.rand(C) + 0.5, 1 + 0.3 * rng.randn(C), 0.2 * rng.randn(C))]


class Res:
    def __init__(self):
        self.t = torch.zeros(16384, dtype=torch.int32, device="cuda")
        self.sc = torch.empty(8 << 20, dtype=torch.uint8, device="cuda")

    def args(self):
        return self.t.data_ptr(), self.t.numel(), self.sc.data_ptr(), self.sc.numel()


def _close(a, b, what):
    a, b = a.double(), b.double()
    err = float((a - b).abs().max() / (b.abs().max() + 1e-30))
    assert err <= 1e-6, (what, err)


def check_stats(launch, rows, C, P, rng):
    """launch(part_ptr) -> status of a producer writing part[rows][2][C] (statistics of P pixels)."""
    res = Res()
    st = stream_handle()
    part = torch.full((rows, 2, C), float("nan"), dtype=torch.float64, device="cuda")
    rm0, rs0 = vec(rng.randn(C)), vec(rng.rand(C) + 0.5)
    got = [torch.empty(C, device="cuda") for _ in range(3)] + [rm0.clone(), rs0.clone()]
    assert lib.dk_bn_fold_arm_stats(part.data_ptr(), rows, C, float(P), EPS, MOM, 0, *(t.data_ptr() for t in got),
                                    *res.args()) == 0
    assert launch(part.data_ptr()) == DK_FOLDED
    want = [torch.empty(C, device="cuda") for _ in range(3)] + [rm0.clone(), rs0.clone()]
    nb = lib.dk_bn_partials_workspace_bytes(rows, C)
    ws = torch.empty(max(nb, 256), dtype=torch.uint8, device="cuda")
    tk = torch.zeros(256, dtype=torch.int32, device="cuda")
    assert lib.dk_bn_stats_from_partials_f32(part.data_ptr(), rows, C, float(P), EPS, MOM, 0,
                                             *(t.data_ptr() for t in want), ws.data_ptr(), nb, tk.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(part).all()
    for g, w, name in zip(got, want, ("mean", "std", "invstd", "running_mean", "running_std")):
        _close(g, w, name)
    assert int(res.t.abs().sum()) == 0, "tickets not left zero"
    # unarmed: the same launch returns 0
    assert launch(part.data_ptr()) == 0


def check_bwd(launch, rows, C, P):
    res = Res()
    st = stream_handle()
    part = torch.full((rows, 2, C), float("nan"), dtype=torch.float64, device="cuda")
    got = [torch.empty(C, device="cuda"), torch.empty(C, device="cuda"), torch.empty(2 * C, device="cuda")]
    assert lib.dk_bn_fold_arm_bwd(part.data_ptr(), rows, C, float(P), *(t.data_ptr() for t in got),
                                  *res.args()) == 0
    assert launch(part.data_ptr()) == DK_FOLDED
    want = [torch.empty(C, device="cuda"), torch.empty(C, device="cuda"), torch.empty(2 * C, device="cuda")]
    nb = lib.dk_bn_partials_workspace_bytes(rows, C)
    ws = torch.empty(max(nb, 256), dtype=torch.uint8, device="cuda")
    tk = torch.zeros(256, dtype=torch.int32, device="cuda")
    assert lib.dk_bn_bwd_from_partials_f32(part.data_ptr(), rows, C, float(P), *(t.data_ptr() for t in want),
                                           ws.data_ptr(), nb, tk.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(part).all()
    for g, w, name in zip(got, want, ("dgamma", "dbeta", "k12")):
        _close(g, w, name)
    assert int(res.t.abs().sum()) == 0, "tickets not left zero"
    assert launch(part.data_ptr()) == 0


# ---------------------------------------------------------------------------------------
# The table of partial-row producers.
# ---------------------------------------------------------------------------------------
NAN = float("nan")


@contextlib.contextmanager
def knobs(pairs):
    """dk_debug_set_gemm_config(kind, value) for every pair, the defaults back on exit."""
    try:
        for k, v in pairs:
            lib.dk_debug_set_gemm_config(k, v)
        yield
    finally:
        for k, _ in pairs:
            lib.dk_debug_set_gemm_config(k, -1)


def act(rng, shape, dtype, scale=1.0, shift=0.0):
    """An NCHW-shaped, NHWC-stored activation of `dtype` (bf16: rounded once here, so the kernel
    and the reference see the same values)."""
    t = torch.as_tensor((rng.randn(*shape) * scale + shift).astype(np.float32), device="cuda").to(dtype)
    return t.contiguous(memory_format=CL)


def nan_act(shape, dtype=F32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda").contiguous(memory_format=CL)


def ptrs(ts):
    return tuple(t.data_ptr() for t in ts)


def scratch(nbytes):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device="cuda")


def _bn64(x, p):
    """x_hat and bn(x) in fp64 from the fp32 parameters p = (mean, invstd[, gamma, beta])."""
    v = [t.double().view(1, -1, 1, 1) for t in p]
    xh = (x.double() - v[0]) * v[1]
    return xh, (v[2] * xh + v[3] if len(v) == 4 else None)


def untie(x, p):
    """The BN-backward kernels recompute the fused ReLU's mask bn(x) > 0 in fp32; the reference does
    it in fp64.  An element with bn(x) within rounding of 0 could fall on either side, and the
    whole gradient element would then count as error: move such inputs away from the edge (the
    test is about the sums, not about ties)."""
    for _ in range(8):
        tie = _bn64(x, p)[1].abs() < 1e-3
        if not bool(tie.any()):
            return x
        x = torch.where(tie, (x.float() + 0.37).to(x.dtype), x).contiguous(memory_format=CL)
    raise AssertionError("could not move the inputs off the ReLU edge")


def stats_ref(y):
    """([2][C] sums, [2][C] sums of |term|) of the stored y: sum y, sum y^2."""
    y = y.double()
    s = torch.stack([y.sum((0, 2, 3)), (y * y).sum((0, 2, 3))])
    return s, torch.stack([y.abs().sum((0, 2, 3)), (y * y).sum((0, 2, 3))])


def bwd_ref(dx, x, p, relu):
    """Stage 1 of a BatchNorm's backward over the stored dx: sum g, sum g * x_hat with g = dx
    masked by bn(x) > 0 when the BN has a fused ReLU; x_hat = (x - mean) * invstd in fp64."""
    xh, b = _bn64(x, p)
    g = dx.double()
    if relu:
        g = g * (b > 0)
    t2 = g * xh
    return (torch.stack([g.sum((0, 2, 3)), t2.sum((0, 2, 3))]),
            torch.stack([g.abs().sum((0, 2, 3)), t2.abs().sum((0, 2, 3))]))


class Case:
    """One built table entry: `rows` from the entry's query, part[rows][2][C] over P pixels,
    launch(part_ptr) -> status, `outs` the kernel's other outputs (NaN before the launch),
    ref() -> (sums, sums of |term|) in fp64."""

    def __init__(self, kind, rows, C, P, launch, outs, ref):
        self.kind, self.rows, self.C, self.P = kind, rows, C, P
        self.launch, self.outs, self.ref = launch, outs, ref

    def poison(self):
        for t in self.outs:
            t.fill_(NAN)


def _seed(*a):
    return np.random.RandomState(sum((i + 1) * int(v) for i, v in enumerate(a)) % (2 ** 31))


def _out_hw(H, W, stride):
    return (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1


# ---- depthwise ----
def dw_fwd(dtype, N, C, H, W, stride, join=False):
    rng = _seed(1, N, C, H, W, stride, join)
    st = stream_handle()
    OH, OW = _out_hw(H, W, stride)
    w = vec(rng.randn(C, 3, 3) * 0.3)
    query = lib.dk_dwconv_fwd_bf16_stats_rows if dtype is BF16 else lib.dk_dwconv_fwd_stats_rows
    rows = query(N, OH, OW, C, stride)
    y = nan_act((N, C, OH, OW), dtype)
    if join:
        a, b = act(rng, (N, C, H, W), F32), act(rng, (N, C, H, W), F32)
        pa = bn_params(C, rng)
        yj = nan_act((N, C, H, W))
        mask = torch.zeros(N * H * W * C, dtype=torch.uint8, device="cuda")

        def launch(p):
            return lib.dk_dwconv_fwd_join_f32(a.data_ptr(), *ptrs(pa), 0, b.data_ptr(), 0, 0, 0, 0, 0, yj.data_ptr(),
                                              mask.data_ptr(), N, H, W, C, w.data_ptr(), stride, 0, y.data_ptr(),
                                              OH, OW, p, st)
        keep, outs = (a, b, pa, mask), [y, yj]
    else:
        x = act(rng, (N, C, H, W), dtype)
        pi = bn_params(C, rng)
        fn = lib.dk_dwconv_fwd_ex_bf16 if dtype is BF16 else lib.dk_dwconv_fwd_ex_f32

        def launch(p):
            return fn(x.data_ptr(), N, H, W, C, w.data_ptr(), 3, 3, stride, 1, 0, y.data_ptr(), OH, OW, *ptrs(pi), 1,
                      p, st)
        keep, outs = (x, pi), [y]
    c = Case("stats", rows, C, N * OH * OW, launch, outs, lambda: stats_ref(y))
    c.keep = (keep, w)
    return c


def dw_dgrad(dtype, N, C, H, W, stride, join=False):
    rng = _seed(2, N, C, H, W, stride, join)
    st = stream_handle()
    OH, OW = _out_hw(H, W, stride)
    w = vec(rng.randn(C, 3, 3) * 0.3)
    dy = act(rng, (N, C, OH, OW), dtype)
    dx = nan_act((N, C, H, W), dtype)
    nb = lib.dk_dwconv_dgrad_workspace_bytes(C, 3, 3)
    ws = scratch(nb)
    if stride == 1:
        rows = (lib.dk_dwconv_dgrad_bf16_stats_rows if dtype is BF16 else lib.dk_dwconv_dgrad_stats_rows)(N, H, W, C, 1)
    else:
        rows = lib.dk_dwconv_dgrad_join_rows(N, H, W, C, 3, 3, stride, 1)
    if join:
        jx = act(rng, (N, C, H, W), F32)
        jp = [vec(rng.randn(C) * 0.3), vec(rng.rand(C) + 0.5)]
        mask = torch.as_tensor((rng.rand(N, H, W, C) > 0.4).astype(np.uint8), device="cuda")

        def launch(p):
            return lib.dk_dwconv_dgrad_join_f32(dy.data_ptr(), N, OH, OW, C, w.data_ptr(), 3, 3, stride, 1,
                                                dx.data_ptr(), H, W, ws.data_ptr(), nb, 0, 0, mask.data_ptr(),
                                                jx.data_ptr(), *ptrs(jp), p, st)
        # dx is stored with the join's mask applied: the sums are over it as it stands
        ref = lambda: bwd_ref(dx, jx, jp, 0)  # noqa: E731
        keep = (jx, jp, mask)
    else:
        pi = bn_params(C, rng)
        x = untie(act(rng, (N, C, H, W), dtype), pi)
        fn = lib.dk_dwconv_dgrad_ex_bf16 if dtype is BF16 else lib.dk_dwconv_dgrad_ex_f32

        def launch(p):
            return fn(dy.data_ptr(), N, OH, OW, C, w.data_ptr(), 3, 3, stride, 1, dx.data_ptr(), H, W, ws.data_ptr(),
                      nb, 0, x.data_ptr(), *ptrs(pi), 1, p, st)
        ref = lambda: bwd_ref(dx, x, pi, 1)  # noqa: E731
        keep = (x, pi)
    c = Case("bwd", rows, C, N * H * W, launch, [dx], ref)
    c.keep = (keep, w, dy, ws)
    return c


def dw_bwd(dtype, N, C, H, W, stride, join=False):
    """The fused depthwise backwards (stride 1: dw_bwd_fused_kernel; stride 2: dw_bwd_s2_kernel)."""
    rng = _seed(3, N, C, H, W, stride, join)
    st = stream_handle()
    OH, OW = _out_hw(H, W, stride)
    g, bx = act(rng, (N, C, OH, OW), dtype), act(rng, (N, C, OH, OW), dtype)
    po = bn_params(C, rng)
    k12 = vec(rng.randn(2 * C) * 0.1)
    w = vec(rng.randn(C, 3, 3) * 0.3)
    dw = torch.full((C, 3, 3), NAN, device="cuda")
    dx = nan_act((N, C, H, W), dtype)
    bf = dtype is BF16
    if stride == 1:
        rows = (lib.dk_dwconv_bwd_bnbwd_bf16_stats_rows if bf else lib.dk_dwconv_bwd_bnbwd_stats_rows)(N, H, W, C)
        nb = (lib.dk_dwconv_bwd_bnbwd_bf16_workspace_bytes if bf else lib.dk_dwconv_bwd_bnbwd_workspace_bytes)(
            N, H, W, C, 3, 3)
    else:
        rows = lib.dk_dwconv_bwd_s2_stats_rows(N, H, W, C)
        nb = lib.dk_dwconv_bwd_s2_workspace_bytes(N, H, W, C)
    ws = scratch(nb)
    head = (g.data_ptr(), bx.data_ptr(), N, H, W, C) + ((OH, OW) if stride == 2 else ()) + ptrs(po) + (1, k12.data_ptr())
    if join:
        # x is the join's output y = ReLU(.) itself: the mask is x > 0 (no stored mask is read)
        x = torch.relu(act(rng, (N, C, H, W), F32)).contiguous(memory_format=CL)
        jx = act(rng, (N, C, H, W), F32)
        jp = [vec(rng.randn(C) * 0.3), vec(rng.rand(C) + 0.5)]
        if stride == 1:
            def launch(p):
                return lib.dk_dwconv_bwd_bnbwd_join_f32(*head, x.data_ptr(), w.data_ptr(), 3, 3, 1, 0.0, dw.data_ptr(),
                                                        dx.data_ptr(), 0, 0, jx.data_ptr(), *ptrs(jp), p,
                                                        ws.data_ptr(), nb, st)
        else:
            def launch(p):
                return lib.dk_dwconv_bwd_s2_bnbwd_join_f32(*head, x.data_ptr(), w.data_ptr(), 0.0, dw.data_ptr(),
                                                           dx.data_ptr(), 0, 0, jx.data_ptr(), *ptrs(jp), p,
                                                           ws.data_ptr(), nb, st)
        ref = lambda: bwd_ref(dx, jx, jp, 0)  # noqa: E731
        keep = (x, jx, jp)
    else:
        pi = bn_params(C, rng)
        x = untie(act(rng, (N, C, H, W), dtype), pi)
        if stride == 1:
            fn = lib.dk_dwconv_bwd_bnbwd_bf16 if bf else lib.dk_dwconv_bwd_bnbwd_f32

            def launch(p):
                return fn(*head, x.data_ptr(), w.data_ptr(), 3, 3, 1, 0.0, dw.data_ptr(), dx.data_ptr(), 0, *ptrs(pi),
                          1, p, ws.data_ptr(), nb, st)
        else:
            fn = lib.dk_dwconv_bwd_s2_bnbwd_bf16 if bf else lib.dk_dwconv_bwd_s2_bnbwd_f32

            def launch(p):
                return fn(*head, x.data_ptr(), w.data_ptr(), 0.0, dw.data_ptr(), dx.data_ptr(), 0, *ptrs(pi), 1, p,
                          ws.data_ptr(), nb, st)
        ref = lambda: bwd_ref(dx, x, pi, 1)  # noqa: E731
        keep = (x, pi)
    c = Case("bwd", rows, C, N * H * W, launch, [dx, dw], ref)
    c.keep = (keep, g, bx, po, k12, w, ws)
    return c


# ---- pointwise ----
def pw_fwd(dtype, K, C, N, H, W, stride):
    rng = _seed(4, K, C, N, H, W, stride)
    st = stream_handle()
    OH, OW = -(-H // stride), -(-W // stride)
    x = act(rng, (N, C, H, W), dtype, shift=0.2)
    w = vec(rng.randn(K, C) * 0.2)
    pi = bn_params(C, rng)
    y = nan_act((N, K, OH, OW), dtype)
    bf = dtype is BF16
    if bf and stride != 1:
        rows = lib.dk_pwconv_fwd_bf16_strided_stats_rows(N, OH, OW, K, C, stride)
    else:
        rows = (lib.dk_pwconv_fwd_bf16_stats_rows if bf else lib.dk_pwconv_fwd_stats_rows)(N, OH, OW, K, C)
    fn = lib.dk_pwconv_fwd_ex_bf16 if bf else lib.dk_pwconv_fwd_ex_f32

    def launch(p):
        return fn(x.data_ptr(), N, H, W, C, w.data_ptr(), K, stride, 0, y.data_ptr(), OH, OW, *ptrs(pi), 1, p, st)
    c = Case("stats", rows, K, N * OH * OW, launch, [y], lambda: stats_ref(y))
    c.keep = (x, w, pi)
    return c


def pw_dgrad(dtype, K, C, N, OH, OW, stride, lattice=False):
    """dk_pwconv_dgrad_ex_* (stride 2: dx widened, zeros off the lattice) and the lattice form."""
    rng = _seed(5, K, C, N, OH, OW, stride, lattice)
    st = stream_handle()
    H, W = OH * stride, OW * stride
    dy = act(rng, (N, K, OH, OW), dtype)
    w = vec(rng.randn(K, C) * 0.2)
    pi = bn_params(C, rng)
    x = untie(act(rng, (N, C, H, W), dtype), pi)
    rows = lib.dk_pwconv_dgrad_stats_rows(N, OH, OW, K, C)
    if lattice:
        dx = nan_act((N, C, OH, OW))

        def launch(p):
            return lib.dk_pwconv_dgrad_lattice_f32(dy.data_ptr(), N, OH, OW, K, w.data_ptr(), C, stride, dx.data_ptr(),
                                                   x.data_ptr(), *ptrs(pi), 1, p, st)
        ref = lambda: bwd_ref(dx, x[:, :, ::stride, ::stride], pi, 1)  # noqa: E731
    else:
        dx = nan_act((N, C, H, W), dtype)
        fn = lib.dk_pwconv_dgrad_ex_bf16 if dtype is BF16 else lib.dk_pwconv_dgrad_ex_f32

        def launch(p):
            return fn(dy.data_ptr(), N, OH, OW, K, w.data_ptr(), C, stride, dx.data_ptr(), 0, x.data_ptr(), *ptrs(pi),
                      1, p, st)
        ref = lambda: bwd_ref(dx, x, pi, 1)  # noqa: E731
    c = Case("bwd", rows, C, N * H * W, launch, [dx], ref)
    c.keep = (dy, w, pi, x)
    return c


def pw_dgrad_bnbwd(dtype, K, C, N, H, W):
    rng = _seed(6, K, C, N, H, W)
    st = stream_handle()
    g, bx = act(rng, (N, K, H, W), dtype), act(rng, (N, K, H, W), dtype)
    po = bn_params(K, rng)
    k12 = vec(rng.randn(2 * K) * 0.1)
    w = vec(rng.randn(K, C) * 0.2)
    pi = bn_params(C, rng)
    x = untie(act(rng, (N, C, H, W), dtype), pi)
    dyo, dx = nan_act((N, K, H, W), dtype), nan_act((N, C, H, W), dtype)
    bf = dtype is BF16
    rows = (lib.dk_pwconv_dgrad_bnbwd_bf16_stats_rows if bf else lib.dk_pwconv_dgrad_bnbwd_stats_rows)(N, H, W, K, C)
    fn = lib.dk_pwconv_dgrad_bnbwd_bf16 if bf else lib.dk_pwconv_dgrad_bnbwd_f32

    def launch(p):
        return fn(g.data_ptr(), bx.data_ptr(), N, H, W, K, *ptrs(po), 1, k12.data_ptr(), dyo.data_ptr(), w.data_ptr(),
                  C, dx.data_ptr(), 0, x.data_ptr(), *ptrs(pi), 1, p, st)
    c = Case("bwd", rows, C, N * H * W, launch, [dx, dyo], lambda: bwd_ref(dx, x, pi, 1))
    c.keep = (g, bx, po, k12, w, pi, x)
    return c


def pw_bwd(dtype, K, C, N, H, W):
    rng = _seed(7, K, C, N, H, W)
    st = stream_handle()
    g, bx = act(rng, (N, K, H, W), dtype), act(rng, (N, K, H, W), dtype)
    po = bn_params(K, rng)
    k12 = vec(rng.randn(2 * K) * 0.1)
    w = vec(rng.randn(K, C) * 0.2)
    pi = bn_params(C, rng)
    x = untie(act(rng, (N, C, H, W), dtype), pi)
    dw = torch.full((K, C), NAN, device="cuda")
    dx = nan_act((N, C, H, W), dtype)
    bf = dtype is BF16
    rows = (lib.dk_pwconv_bwd_fused_bf16_rows if bf else lib.dk_pwconv_bwd_fused_rows)(N, H, W, K, C)
    nb = (lib.dk_pwconv_bwd_fused_bf16_workspace_bytes if bf else lib.dk_pwconv_bwd_fused_workspace_bytes)(
        N, H, W, K, C)
    ws = scratch(nb)
    fn = lib.dk_pwconv_bwd_bnbwd_bf16 if bf else lib.dk_pwconv_bwd_bnbwd_f32

    def launch(p):
        return fn(g.data_ptr(), bx.data_ptr(), N, H, W, K, *ptrs(po), 1, k12.data_ptr(), w.data_ptr(), C, 0.0,
                  dw.data_ptr(), dx.data_ptr(), 0, x.data_ptr(), *ptrs(pi), 1, p, ws.data_ptr(), nb, st)
    c = Case("bwd", rows, C, N * H * W, launch, [dx, dw], lambda: bwd_ref(dx, x, pi, 1))
    c.keep = (g, bx, po, k12, w, pi, x, ws)
    return c


# ---- the others ----
def conv_fwd(N, H, W):
    """dk_conv2d_fwd_ex_f32 at the stem's geometry (5 x 5, stride 2, 3 channels padded to 4)."""
    rng = _seed(8, N, H, W)
    st = stream_handle()
    Cp, K, R, s, pad = 4, 64, 5, 2, 2
    OH, OW = (H + 2 * pad - R) // s + 1, (W + 2 * pad - R) // s + 1
    x = nhwc(np.concatenate([rng.randn(N, 3, H, W), np.zeros((N, 1, H, W))], 1))
    w = vec(rng.randn(K, R, R, Cp) * 0.1)
    y = nan_act((N, K, OH, OW))
    rows = lib.dk_conv2d_fwd_stats_rows(N, OH, OW, K, Cp, R, R)

    def launch(p):
        return lib.dk_conv2d_fwd_ex_f32(x.data_ptr(), N, H, W, Cp, w.data_ptr(), K, R, R, s, pad, 0, y.data_ptr(), OH,
                                        OW, 0, 0, 0, 0, 0, p, st)
    c = Case("stats", rows, K, N * OH * OW, launch, [y], lambda: stats_ref(y))
    c.keep = (x, w)
    return c


def conv_narrow_fwd(N, H, W):
    rng = _seed(9, N, H, W)
    st = stream_handle()
    C, K, R, s, pad = 3, 64, 5, 2, 1
    OH, OW = (H + 2 * pad - R) // s + 1, (W + 2 * pad - R) // s + 1
    x = torch.from_numpy(rng.randn(N, C, H, W).astype(np.float32)).cuda()  # NCHW
    w = vec(rng.randn(K, C, R, R) * 0.1)
    y = nan_act((N, K, OH, OW))
    rows = lib.dk_conv2d_fwd_narrow_stats_rows(N, C, H, W, K, R, R, s, pad, OH, OW)

    def launch(p):
        return lib.dk_conv2d_fwd_narrow_f32(x.data_ptr(), N, C, H, W, w.data_ptr(), K, R, R, s, pad, 0, y.data_ptr(),
                                            OH, OW, p, st)
    c = Case("stats", rows, K, N * OH * OW, launch, [y], lambda: stats_ref(y))
    c.keep = (x, w)
    return c


def relu_bwd_partial(N, C, H, W):
    rng = _seed(10, N, C, H, W)
    st = stream_handle()
    P = N * H * W
    dy = act(rng, (N, C, H, W), F32)
    mask = torch.as_tensor((rng.rand(N, H, W, C) > 0.4).astype(np.uint8), device="cuda")
    pi = bn_params(C, rng)
    x = untie(act(rng, (N, C, H, W), F32), pi)
    dx = nan_act((N, C, H, W))
    rows = lib.dk_bn_partial_blocks(P, C)
    nb = lib.dk_bn_workspace_bytes(P, C)

    def launch(p):
        return lib.dk_relu_bwd_bn_partial_f64(dy.data_ptr(), mask.data_ptr(), x.data_ptr(), P, C, *ptrs(pi), 1,
                                              dx.data_ptr(), p, nb, st)
    # dx = mask ? dy : 0 as stored; the BN's own fused ReLU masks it once more in the sums
    c = Case("bwd", rows, C, P, launch, [dx], lambda: bwd_ref(dx, x, pi, 1))
    c.keep = (dy, mask, pi, x)
    return c


# Longest chain a kernel accumulates in fp32 before it widens to fp64, with the line it is read
# from (k = 1: every term is widened on its own).
K_DW_FWD = (1, "depthwise.hip:439-441, each stored y widened before the add")
K_DW_FWD16 = (4, "depthwise.hip:433-435 and :458-459, a thread's row of TW <= 4 stored values in fp32, then fp64")
K_DW_DGRAD = (1, "depthwise.hip:449-450, g and g * x_hat widened per element")
K_DW_SUBPIX = (1, "depthwise.hip:651-652 / :660-661")
K_DW_BWD = (1, "depthwise.hip:1219-1220")
K_DW_BWD_JOIN = (1, "depthwise.hip:1199-1200")
K_DW_BWD_S2 = (1, "depthwise.hip:1580-1581 / :1592-1593")
K_TILED_STATS = (1, "gemm_engine.h:611-613, EpStoreStatsT::put4")
K_TILED_BWD = (1, "gemm_engine.h:632-633, bn_bwd_contrib")
K_PWS_FWD = (1, "pw_stream.hip:489")
K_PWS_DGRAD = (1, "pw_stream.hip:247-248")
K_PWS_BWD = (1, "pw_stream.hip:845-846")
K_PWD_FWD = (1, "pw_deep.hip:266 / :274")
K_PWD_DGRAD = (1, "pw_deep.hip:429-430 / :629-630")
K_PWD_BWD = (1, "pw_deep.hip:833-834 / :1047-1048")
K_PWSH_FWD = (1, "pw_stream_bf16.hip:189")
K_PWSH_DGRAD = (1, "pw_stream_bf16.hip:389-390")
K_PWSH_BWD = (1, "pw_stream_bf16.hip:614-615")
K_PWD16_FWD = (1, "pw_deep_bf16.hip:225")
K_PWD16_BWD = (1, "pw_deep_bf16.hip:547-548")
K_NARROW = (1, "conv_narrow.hip:193")
K_BN_PARTIAL = (1, "batchnorm.hip:386-387")

# knob kinds (include/dorknet_hip.h, dk_debug_set_gemm_config)
ROW_CFG, STREAM, DWB_BLOCKS, DW_SEG, PWSH, DEEP, DEEP16 = 0, 3, 7, 8, 9, 11, 13

# GEMM producers: M = 2 x 9 x 11 = 198 pixels, a multiple of no tile height
G = (2, 9, 11)
DW30 = (2, 64, 30, 30)    # fp32 forward / dgrad: 3 rows, bf16: 1
DW7 = (3, 512, 7, 7)      # blocks span images; several channel slices in the fused backward
DW15 = (3, 64, 15, 15)    # stride 2, odd extents


def _e(id, entry, query, dtype, shape, k, make, force=(), other=None, knob=None):
    """force: knobs that select the variant (held for every check); other: knobs under which another
    variant takes the shape (its row count must differ: the rows written tell the two apart);
    knob: the tuning knob of the "under a knob" check."""
    return dict(id=id, entry=entry, query=query, dtype="bf16" if dtype is BF16 else "f32", shape=shape, k=k[0],
                k_src=k[1], make=make, force=tuple(force), other=other, knob=knob)


def _table():
    T = []
    seg = ((DW_SEG, 5),)
    dwb = ((DWB_BLOCKS, 3),)
    for dt, sfx, q, k in ((F32, "f32", "dk_dwconv_fwd_stats_rows", K_DW_FWD),
                          (BF16, "bf16", "dk_dwconv_fwd_bf16_stats_rows", K_DW_FWD16)):
        for shp, s in ((DW30, 1), (DW7, 1), (DW15, 2)):
            T.append(_e("dw_fwd_%s-s%d-%dx%dx%dx%d" % ((sfx, s) + shp), "dk_dwconv_fwd_ex_" + sfx, q, dt, shp, k,
                        lambda dt=dt, shp=shp, s=s: dw_fwd(dt, *shp, s), knob=seg))
    for shp, s in ((DW30, 1), (DW15, 2)):
        T.append(_e("dw_fwd_join_f32-s%d-%dx%dx%dx%d" % ((s,) + shp), "dk_dwconv_fwd_join_f32",
                    "dk_dwconv_fwd_stats_rows", F32, shp, K_DW_FWD, lambda shp=shp, s=s: dw_fwd(F32, *shp, s, True),
                    knob=seg))
    for dt, sfx in ((F32, "f32"), (BF16, "bf16")):
        q1 = "dk_dwconv_dgrad_bf16_stats_rows" if dt is BF16 else "dk_dwconv_dgrad_stats_rows"
        for shp, s in ((DW30, 1), (DW7, 1), (DW15, 2)):
            T.append(_e("dw_dgrad_%s-s%d-%dx%dx%dx%d" % ((sfx, s) + shp), "dk_dwconv_dgrad_ex_" + sfx,
                        q1 if s == 1 else "dk_dwconv_dgrad_join_rows", dt, shp, K_DW_DGRAD if s == 1 else K_DW_SUBPIX,
                        lambda dt=dt, shp=shp, s=s: dw_dgrad(dt, *shp, s), knob=seg))
    T.append(_e("dw_dgrad_join_f32-s2-%dx%dx%dx%d" % DW15, "dk_dwconv_dgrad_join_f32", "dk_dwconv_dgrad_join_rows", F32,
                DW15, K_DW_SUBPIX, lambda: dw_dgrad(F32, *DW15, 2, True), knob=seg))
    for dt, sfx in ((F32, "f32"), (BF16, "bf16")):
        q1 = "dk_dwconv_bwd_bnbwd_bf16_stats_rows" if dt is BF16 else "dk_dwconv_bwd_bnbwd_stats_rows"
        for shp, s in ((DW30, 1), (DW7, 1), (DW15, 2)):
            name = "dk_dwconv_bwd_bnbwd_" + sfx if s == 1 else "dk_dwconv_bwd_s2_bnbwd_" + sfx
            T.append(_e("dw_bwd_%s-s%d-%dx%dx%dx%d" % ((sfx, s) + shp), name,
                        q1 if s == 1 else "dk_dwconv_bwd_s2_stats_rows", dt, shp, K_DW_BWD if s == 1 else K_DW_BWD_S2,
                        lambda dt=dt, shp=shp, s=s: dw_bwd(dt, *shp, s), knob=dwb))
    for shp, s in ((DW30, 1), (DW7, 1), (DW15, 2)):
        name = "dk_dwconv_bwd_bnbwd_join_f32" if s == 1 else "dk_dwconv_bwd_s2_bnbwd_join_f32"
        T.append(_e("dw_bwd_join_f32-s%d-%dx%dx%dx%d" % ((s,) + shp), name,
                    "dk_dwconv_bwd_bnbwd_stats_rows" if s == 1 else "dk_dwconv_bwd_s2_stats_rows", F32, shp,
                    K_DW_BWD_JOIN if s == 1 else K_DW_BWD_S2, lambda shp=shp, s=s: dw_bwd(F32, *shp, s, True),
                    knob=dwb))

    def pw(id, entry, query, dt, K, C, k, make, s=1, **kw):
        # shape: N x K x C x H x W of the layer input (stride s: the output is G's 9 x 11)
        T.append(_e("%s-K%d-C%d" % (id, K, C), entry, query, dt, (G[0], K, C, s * G[1], s * G[2]), k, make, **kw))

    # pointwise forward: the streaming, deep and tiled variants
    q = "dk_pwconv_fwd_stats_rows"
    pw("pw_fwd_f32-stream", "dk_pwconv_fwd_ex_f32", q, F32, 64, 64, K_PWS_FWD, lambda: pw_fwd(F32, 64, 64, *G, 1),
       other=((STREAM, 0),))
    pw("pw_fwd_f32-tiled", "dk_pwconv_fwd_ex_f32", q, F32, 64, 64, K_TILED_STATS, lambda: pw_fwd(F32, 64, 64, *G, 1),
       force=((STREAM, 0),), other=(), knob=((ROW_CFG, 1),))
    pw("pw_fwd_f32-deep", "dk_pwconv_fwd_ex_f32", q, F32, 128, 64, K_PWD_FWD, lambda: pw_fwd(F32, 128, 64, *G, 1),
       other=((DEEP, 0),))
    q = "dk_pwconv_fwd_bf16_stats_rows"
    pw("pw_fwd_bf16-stream", "dk_pwconv_fwd_ex_bf16", q, BF16, 64, 64, K_PWSH_FWD,
       lambda: pw_fwd(BF16, 64, 64, *G, 1), other=((PWSH, 0),))
    pw("pw_fwd_bf16-tiled", "dk_pwconv_fwd_ex_bf16", q, BF16, 64, 64, K_TILED_STATS,
       lambda: pw_fwd(BF16, 64, 64, *G, 1), force=((PWSH, 0),), other=())
    pw("pw_fwd_bf16-deep", "dk_pwconv_fwd_ex_bf16", q, BF16, 256, 128, K_PWD16_FWD,
       lambda: pw_fwd(BF16, 256, 128, *G, 1), other=((DEEP16, 0),))
    # stride 2 at a streaming shape: the bf16 streaming kernels take stride 1 only, so the launch is
    # the tiled engine's and the plain query (the streaming rows) does not describe it
    pw("pw_fwd_bf16-s2", "dk_pwconv_fwd_ex_bf16", "dk_pwconv_fwd_bf16_strided_stats_rows", BF16, 64, 64, K_TILED_STATS,
       lambda: pw_fwd(BF16, 64, 64, G[0], 2 * G[1], 2 * G[2], 2), s=2)
    pw("pw_fwd_f32-s2", "dk_pwconv_fwd_ex_f32", "dk_pwconv_fwd_stats_rows", F32, 64, 64, K_PWS_FWD,
       lambda: pw_fwd(F32, 64, 64, G[0], 2 * G[1], 2 * G[2], 2), s=2)
    # pointwise dgrad (the tiled engine's epilogues)
    q = "dk_pwconv_dgrad_stats_rows"
    pw("pw_dgrad_f32-s1", "dk_pwconv_dgrad_ex_f32", q, F32, 64, 64, K_TILED_BWD,
       lambda: pw_dgrad(F32, 64, 64, *G, 1), knob=((ROW_CFG, 1),))
    pw("pw_dgrad_f32-s2", "dk_pwconv_dgrad_ex_f32", q, F32, 128, 64, K_TILED_BWD,
       lambda: pw_dgrad(F32, 128, 64, *G, 2), s=2)
    pw("pw_dgrad_bf16-s1", "dk_pwconv_dgrad_ex_bf16", q, BF16, 64, 64, K_TILED_BWD,
       lambda: pw_dgrad(BF16, 64, 64, *G, 1))
    pw("pw_dgrad_lattice_f32-s2", "dk_pwconv_dgrad_lattice_f32", q, F32, 64, 64, K_TILED_BWD,
       lambda: pw_dgrad(F32, 64, 64, *G, 2, True), s=2)
    q = "dk_pwconv_dgrad_bnbwd_stats_rows"
    pw("pw_dgrad_bnbwd_f32-stream", "dk_pwconv_dgrad_bnbwd_f32", q, F32, 64, 64, K_PWS_DGRAD,
       lambda: pw_dgrad_bnbwd(F32, 64, 64, *G), other=((STREAM, 0),))
    pw("pw_dgrad_bnbwd_f32-tiled", "dk_pwconv_dgrad_bnbwd_f32", q, F32, 64, 64, K_TILED_BWD,
       lambda: pw_dgrad_bnbwd(F32, 64, 64, *G), force=((STREAM, 0),), other=())
    pw("pw_dgrad_bnbwd_f32-deep", "dk_pwconv_dgrad_bnbwd_f32", q, F32, 256, 128, K_PWD_DGRAD,
       lambda: pw_dgrad_bnbwd(F32, 256, 128, *G), other=((DEEP, 0),))
    q = "dk_pwconv_dgrad_bnbwd_bf16_stats_rows"
    # (no `other`: the bf16 streaming dgrad and the tiled engine's 128-row tile both write one row per
    # 128 pixels at K = C = 64, so the row count cannot tell the two apart)
    pw("pw_dgrad_bnbwd_bf16-stream", "dk_pwconv_dgrad_bnbwd_bf16", q, BF16, 64, 64, K_PWSH_DGRAD,
       lambda: pw_dgrad_bnbwd(BF16, 64, 64, *G))
    pw("pw_dgrad_bnbwd_bf16-tiled", "dk_pwconv_dgrad_bnbwd_bf16", q, BF16, 64, 64, K_TILED_BWD,
       lambda: pw_dgrad_bnbwd(BF16, 64, 64, *G), force=((PWSH, 0),))
    # fused pointwise backward: K = C = 64 (streaming), K = 128 / C = 64 and a deep K (weight-stationary)
    q = "dk_pwconv_bwd_fused_rows"
    for K, C, k in ((64, 64, K_PWS_BWD), (128, 64, K_PWD_BWD), (256, 128, K_PWD_BWD)):
        pw("pw_bwd_f32", "dk_pwconv_bwd_bnbwd_f32", q, F32, K, C, k, lambda K=K, C=C: pw_bwd(F32, K, C, *G))
    q = "dk_pwconv_bwd_fused_bf16_rows"
    for K, C, k in ((64, 64, K_PWSH_BWD), (128, 64, K_PWD16_BWD), (256, 128, K_PWD16_BWD)):
        pw("pw_bwd_bf16", "dk_pwconv_bwd_bnbwd_bf16", q, BF16, K, C, k, lambda K=K, C=C: pw_bwd(BF16, K, C, *G))
    # the others
    T.append(_e("conv2d_fwd_ex_f32-2x21x19", "dk_conv2d_fwd_ex_f32", "dk_conv2d_fwd_stats_rows", F32, (2, 4, 21, 19),
                K_TILED_STATS, lambda: conv_fwd(2, 21, 19)))
    T.append(_e("conv2d_fwd_narrow_f32-2x23x21", "dk_conv2d_fwd_narrow_f32", "dk_conv2d_fwd_narrow_stats_rows", F32,
                (2, 3, 23, 21), K_NARROW, lambda: conv_narrow_fwd(2, 23, 21)))
    T.append(_e("relu_bwd_bn_partial_f64-2x64x9x11", "dk_relu_bwd_bn_partial_f64", "dk_bn_partial_blocks", F32,
                (2, 64, 9, 11), K_BN_PARTIAL, lambda: relu_bwd_partial(2, 64, 9, 11)))
    return T


TABLE = _table()
