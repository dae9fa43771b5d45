"""Every output element of the fp32 dense-convolution entry points -- the implicit-GEMM engine's forward, input
gradient (stride 1 and per sub-pixel phase) and weight gradient (plain, BatchNorm on load, the following
BatchNorm's backward on load), the narrow-input forward and weight gradients, and the sub-pixel input gradient --
and the forward's BatchNorm statistics against the fp64 reference of the same operation (tests/_conv_ref.py), each
under the bound derived there from the arithmetic, none excluded.  The cases (_conv_ref.ENGINE / NARROW / SUBPIX)
are the smallest that reach each tile choice, split-K configuration, narrow shape, quad bucket and sub-pixel
geometry; their comments say which.

The engine entry points run twice: under the default knobs and with the row and split-K tiles forced to one other
valid configuration (dk_debug_set_gemm_config 0 -> 16, 128 x 128 x 32, which no fp32 convolution picks by itself; 1
-> the one of 64 x 128 x 32 / 64 x 64 x 32 the shape does not pick; restored in a finally), so both are held to the
reference directly.

Outputs are guarded (tests/_guard.py): 16-byte-aligned slices of NaN-bit-filled buffers whose 64-element margins
must stay intact and in which no element may remain NaN.  Statistics are pre-filled with NaN, rows + 1 rows
allocated: every row the *_stats_rows() query reports must have been written and the extra one must stay NaN.

The multi-row narrow cases nm1 / nm2 (N = 70: 2170 output rows) assert from the library's own queries that a block
owns more than one output row.

Worst err / bound per family on an MI355X, default and forced tiles together (recorded with DORKNET_SLACK_LOG;
results, not tolerances; 1632 checks in all):

    family                                          checks   worst
    engine forward y (plain, bnx, ex)                  432   0.098
      statistics | stored   (sum, squares)             144   0, 0.107
      statistics | reference                           144   0.015, 0.020
    dgrad dx  stride 1 (dk_conv2d_dgrad_f32)            10   0.006
              phase                                     38   0.073
              sub-pixel                                  7   0.098
    wgrad dw  plain / bnx / bnbwd               48 / 96 / 176   0.026 / 0.042 / 0.053
    narrow forward y                                    44   0.099
      statistics | stored / reference                   22   0, 0.018 / 0.005, 0.007
    narrow wgrad dw / bnbwd (dense and lattice)    22 / 88   0.005 / 0.015

Multi-row cases: N = 70 as tabled (no enlargement was needed); both queries report 1085 blocks for the 2170 output
rows of nm1 and of nm2, two rows per block in the forward and in the weight gradient, so every other block straddles
two images.

Every fp32 output stays below a tenth of its bound (the MFMA outputs against 2 u per step, the sub-pixel VALU sums
against u per step), so the one-ulp-per-step model of the MFMA is not strained here either and the constants
stand as derived.  No kernel defect was found.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

from dorknet_amd._hip import HipError, lib, stream_handle, workspace
from tests import _conv_ref as R
from tests._convert import log_ratio
from tests._guard import Guarded

pytestmark = pytest.mark.gpu

F32 = torch.float32
L2 = R.L2
ROUTES = ("default", "forced")
ZERO5 = (0, 0, 0, 0, 0)
ENGINE, NARROW, SUBPIX = list(R.ENGINE), list(R.NARROW), list(R.SUBPIX)


@contextlib.contextmanager
def routing(route, c):
    """"forced": row tile 16 and the split-K tile the shape does not pick (gemm_engine.h splitk_config: K <= 64 <
    R S Cp -> 6, else 1) for the calls inside."""
    if route == "default":
        yield
        return
    try:
        lib.dk_debug_set_gemm_config(0, 16)
        lib.dk_debug_set_gemm_config(1, 1 if c.K <= 64 < c.R * c.S * c.Cp else 6)
        yield
    finally:
        lib.dk_debug_set_gemm_config(0, -1)
        lib.dk_debug_set_gemm_config(1, -1)


def nhwc(a, cp=None):
    """An NCHW host array on the device as fp32 NHWC, the channels zero-padded to cp."""
    a = np.asarray(a, dtype=np.float32).transpose(0, 2, 3, 1)
    if cp is not None and cp != a.shape[3]:
        a = np.concatenate([a, np.zeros(a.shape[:3] + (cp - a.shape[3],), np.float32)], axis=3)
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def vec(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def nchw(a):
    return a.transpose(0, 3, 1, 2)


def nan_rows(rows, n):
    return torch.full((rows + 1, 2, n), float("nan"), dtype=torch.float64, device="cuda")


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def inputs(name):
    d = R.make_inputs(name)
    c = d["case"]
    st = stream_handle()
    d["x_d"], d["x_nchw"] = nhwc(d["x"], c.Cp), vec(d["x"])
    d["dy_d"], d["dyp_d"] = nhwc(d["dy"]), nhwc(d["dy"], R.roundup4(c.K))
    d["g_d"], d["x1_d"], d["g2_d"] = nhwc(d["g"]), nhwc(d["x1"]), nhwc(d["g"][:, :, ::2, ::2])
    d["w_d"], d["bias_d"], d["k12_d"] = vec(d["w"]), vec(d["bias"]), vec(d["k12"])
    d["pi_d"], d["po_d"] = [vec(v) for v in d["pi"]], [vec(v) for v in d["po"]]
    d["krsc_d"] = torch.empty((c.K, c.R, c.S, c.Cp), dtype=F32, device="cuda")
    lib.dk_conv_weight_krsc_f32(d["w_d"].data_ptr(), c.K, c.C, c.R, c.S, c.Cp, d["krsc_d"].data_ptr(), st)
    d["crsk_d"] = torch.empty((c.C, c.R, c.S, c.K), dtype=F32, device="cuda")
    lib.dk_conv_weight_crsk_f32(d["w_d"].data_ptr(), c.K, c.C, c.R, c.S, d["crsk_d"].data_ptr(), st)
    torch.cuda.synchronize()
    return d


def pi_ptrs(d, relu):
    return ZERO5 if relu is None else (*(t.data_ptr() for t in d["pi_d"]), relu)


def po_ptrs(d, relu):
    return (*(t.data_ptr() for t in d["po_d"]), relu)


def refused(code, fn, *args):
    with pytest.raises(HipError, match=str(code)):
        fn(*args)


@functools.lru_cache(maxsize=None)
def fwd_ref(name, bias, bn, narrow=False):
    return R.forward(inputs(name), bias, bn, narrow)


@functools.lru_cache(maxsize=None)
def dgrad_ref(name, entry):
    return R.dgrad(inputs(name), entry)


@functools.lru_cache(maxsize=None)
def wgrad_ref(name, l2, bn, relu=None, lattice=1):
    d = inputs(name)
    if relu is None:
        return R.wgrad(d, l2, bn)
    return R.wgrad(d, l2, bn, *R.formed_dy(d, relu, lattice))


def stats_result(name, part, rows, got, r):
    s = host(part)
    assert np.isnan(s[rows]).all(), "{}: a row past the reported {} was written".format(name, rows)
    R.stats_checks(name, s[:rows], got, r.ref, r.A)


# ---------------------------------------------------------------------------------------------------------
# the engine
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", ENGINE)
def test_engine_forward(name, route):
    d = inputs(name)
    c, OH, OW, sh = d["case"], d["OH"], d["OW"], stream_handle()
    geom = (c.K, c.R, c.S, c.stride, c.pad)
    x, w = d["x_d"].data_ptr(), d["krsc_d"].data_ptr()
    with routing(route, c):
        for bias in (False, True):
            b = d["bias_d"].data_ptr() if bias else 0
            y = Guarded((c.N, OH, OW, c.K), F32)
            assert lib.dk_conv2d_fwd_f32(x, c.N, c.H, c.W, c.Cp, w, *geom, b, y.ptr, OH, OW, sh) == 0
            r = fwd_ref(name, bias, None)
            R.check("fwd {} {} plain y".format(name, route), nchw(y.result()), r.ref, r.A)
            for relu in (0, 1):
                y = Guarded((c.N, OH, OW, c.K), F32)
                assert lib.dk_conv2d_fwd_bnx_f32(x, c.N, c.H, c.W, c.Cp, w, *geom, b, y.ptr, OH, OW, *pi_ptrs(d, relu),
                                                 sh) == 0
                r = fwd_ref(name, bias, relu)
                R.check("fwd {} {} bnx y".format(name, route), nchw(y.result()), r.ref, r.A)
            for bn in (None, 0, 1):
                for stats in (False, True):
                    rows = lib.dk_conv2d_fwd_stats_rows(c.N, OH, OW, c.K, c.Cp, c.R, c.S)
                    assert rows > 0
                    part = nan_rows(rows, c.K) if stats else None
                    y = Guarded((c.N, OH, OW, c.K), F32)
                    assert lib.dk_conv2d_fwd_ex_f32(x, c.N, c.H, c.W, c.Cp, w, *geom, b, y.ptr, OH, OW, *pi_ptrs(d, bn),
                                                    part.data_ptr() if stats else 0, sh) == 0
                    r = fwd_ref(name, bias, bn)
                    got = nchw(y.result())
                    R.check("fwd {} {} ex y".format(name, route), got, r.ref, r.A)
                    if stats:
                        stats_result("fwd {} {} stats".format(name, route), part, rows, got, r)


def test_forced_route_is_another_tile():
    """e2 (M = 198): four 64-row tiles by default, two 128-row tiles under the forced row configuration."""
    c = R.ENGINE["e2"]
    OH, OW = R.case_hw(c)
    rows = {}
    for route in ROUTES:
        with routing(route, c):
            rows[route] = lib.dk_conv2d_fwd_stats_rows(c.N, OH, OW, c.K, c.Cp, c.R, c.S)
    assert rows == {"default": 4, "forced": 2}


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", ENGINE + SUBPIX)
def test_engine_dgrad(name, route):
    """dk_conv2d_dgrad_phase_f32 at every case (dy zero-padded to Kp as the layer does), dk_conv2d_dgrad_f32 at the
    stride-1 cases with K % 4 == 0."""
    d = inputs(name)
    c, OH, OW, sh = d["case"], d["OH"], d["OW"], stream_handle()
    Kp = R.roundup4(c.K)
    with routing(route, c):
        nb = lib.dk_conv2d_dgrad_phase_workspace_bytes(c.K, c.C, c.R, c.S, c.stride)
        assert nb == c.C * c.R * c.S * Kp * 4
        dx = Guarded((c.N, c.H, c.W, c.C), F32)
        assert lib.dk_conv2d_dgrad_phase_f32(d["dyp_d"].data_ptr(), c.N, OH, OW, Kp, c.K, d["w_d"].data_ptr(), c.C, c.R,
                                             c.S, c.stride, c.pad, dx.ptr, c.H, c.W, workspace.get(nb), nb, sh) == 0
        r = dgrad_ref(name, "phase")
        R.check("dgrad-phase {} {} dx".format(name, route), nchw(dx.result()), r.ref, r.A)
        if c.stride == 1 and c.K % 4 == 0:
            dx = Guarded((c.N, c.H, c.W, c.C), F32)
            assert lib.dk_conv2d_dgrad_f32(d["dy_d"].data_ptr(), c.N, OH, OW, c.K, d["crsk_d"].data_ptr(), c.C, c.R, c.S,
                                           c.pad, dx.ptr, c.H, c.W, sh) == 0
            r = dgrad_ref(name, "gemm")
            R.check("dgrad-gemm {} {} dx".format(name, route), nchw(dx.result()), r.ref, r.A)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", ENGINE)
def test_engine_wgrad(name, route):
    d = inputs(name)
    c, OH, OW, sh = d["case"], d["OH"], d["OW"], stream_handle()
    x = d["x_d"].data_ptr()
    shape = (c.N, c.H, c.W, c.Cp, c.C, c.K, c.R, c.S, c.stride, c.pad, OH, OW)
    with routing(route, c):
        nb = lib.dk_conv2d_wgrad_workspace_bytes(c.N, OH, OW, c.K, c.Cp, c.R, c.S)
        assert nb >= c.K * c.R * c.S * c.Cp * 4
        for l2 in (0.0, L2):
            tail = (d["w_d"].data_ptr() if l2 else 0, l2)
            dw = Guarded((c.K, c.C, c.R, c.S), F32)
            assert lib.dk_conv2d_wgrad_f32(d["dy_d"].data_ptr(), x, *shape, *tail, dw.ptr, workspace.get(nb), nb, sh) == 0
            r = wgrad_ref(name, l2, None)
            R.check("wgrad-plain {} {} dw".format(name, route), dw.result(), r.ref, r.A)
            for relu in (0, 1):
                dw = Guarded((c.K, c.C, c.R, c.S), F32)
                assert lib.dk_conv2d_wgrad_bnx_f32(d["dy_d"].data_ptr(), x, *shape, *tail, dw.ptr, workspace.get(nb), nb,
                                                   *pi_ptrs(d, relu), sh) == 0
                r = wgrad_ref(name, l2, relu)
                R.check("wgrad-bnx {} {} dw".format(name, route), dw.result(), r.ref, r.A)
            for relu in (0, 1):
                for bn in (None, 1):
                    dw = Guarded((c.K, c.C, c.R, c.S), F32)
                    args = (d["g_d"].data_ptr(), d["x1_d"].data_ptr(), x, *shape, *po_ptrs(d, relu), d["k12_d"].data_ptr(),
                            *tail, dw.ptr, workspace.get(nb), nb, *pi_ptrs(d, bn), sh)
                    if c.K % 4:
                        refused(10001, lib.dk_conv2d_wgrad_bnbwd_f32, *args)
                        continue
                    assert lib.dk_conv2d_wgrad_bnbwd_f32(*args) == 0
                    r = wgrad_ref(name, l2, bn, relu)
                    R.check("wgrad-bnbwd {} {} dw".format(name, route), dw.result(), r.ref, r.A)


# ---------------------------------------------------------------------------------------------------------
# the narrow-input kernels
# ---------------------------------------------------------------------------------------------------------

def narrow_geom(d):
    c = d["case"]
    return (c.N, c.C, c.H, c.W, c.K, c.R, c.S, c.stride, c.pad, d["OH"], d["OW"])


@pytest.mark.parametrize("name", NARROW)
def test_narrow_forward(name):
    d = inputs(name)
    c, OH, OW, sh = d["case"], d["OH"], d["OW"], stream_handle()
    assert lib.dk_conv2d_narrow_preferred(*narrow_geom(d)) == 1
    rows = lib.dk_conv2d_fwd_narrow_stats_rows(*narrow_geom(d))
    assert 0 < rows <= c.N * OH
    if name in R.MULTIROW:
        assert rows < c.N * OH, "one output row per block: enlarge N"
        log_ratio("nfwd {} rows per block".format(name), -(-c.N * OH // rows), "conv-info")
    for bias in (False, True):
        for stats in (False, True):
            part = nan_rows(rows, c.K) if stats else None
            y = Guarded((c.N, OH, OW, c.K), F32)
            assert lib.dk_conv2d_fwd_narrow_f32(d["x_nchw"].data_ptr(), c.N, c.C, c.H, c.W, d["w_d"].data_ptr(), c.K, c.R,
                                                c.S, c.stride, c.pad, d["bias_d"].data_ptr() if bias else 0, y.ptr, OH,
                                                OW, part.data_ptr() if stats else 0, sh) == 0
            r = fwd_ref(name, bias, None, True)
            got = nchw(y.result())
            R.check("nfwd {} y".format(name), got, r.ref, r.A)
            if stats:
                stats_result("nfwd {} stats".format(name), part, rows, got, r)


@pytest.mark.parametrize("name", NARROW)
def test_narrow_wgrad(name):
    d = inputs(name)
    c, sh = d["case"], stream_handle()
    geom = narrow_geom(d)
    nb = lib.dk_conv2d_wgrad_narrow_workspace_bytes(*geom)
    blocks = nb // (4 * c.K * c.C * c.R * c.S)
    assert 0 < blocks <= c.N * d["OH"] and nb == blocks * 4 * c.K * c.C * c.R * c.S
    if name in R.MULTIROW:
        assert blocks < c.N * d["OH"], "one output row per block: enlarge N"
        log_ratio("nwgrad {} rows per block".format(name), -(-c.N * d["OH"] // blocks), "conv-info")
    x = d["x_nchw"].data_ptr()
    for l2 in (0.0, L2):
        tail = (d["w_d"].data_ptr() if l2 else 0, l2)
        dw = Guarded((c.K, c.C, c.R, c.S), F32)
        assert lib.dk_conv2d_wgrad_narrow_f32(d["dy_d"].data_ptr(), x, *geom, *tail, dw.ptr, workspace.get(nb), nb, sh) == 0
        r = wgrad_ref(name, l2, None)
        R.check("nwgrad {} dw".format(name), dw.result(), r.ref, r.A)
        for relu in (0, 1):
            for lattice in (1, 2):
                dw = Guarded((c.K, c.C, c.R, c.S), F32)
                g = d["g_d"] if lattice == 1 else d["g2_d"]
                assert lib.dk_conv2d_wgrad_bnbwd_narrow_f32(g.data_ptr(), d["x1_d"].data_ptr(), x, *geom, *po_ptrs(d, relu),
                                                            d["k12_d"].data_ptr(), lattice, *tail, dw.ptr,
                                                            workspace.get(nb), nb, sh) == 0
                r = wgrad_ref(name, l2, None, relu, lattice)
                R.check("nbnbwd {} lat{} dw".format(name, lattice), dw.result(), r.ref, r.A)


# ---------------------------------------------------------------------------------------------------------
# the sub-pixel input gradient
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SUBPIX)
def test_subpixel_dgrad(name):
    """Held to the reference test_engine_dgrad holds the phase dgrad to at the same case (its own bound)."""
    d = inputs(name)
    c, sh = d["case"], stream_handle()
    nb = lib.dk_conv2d_dgrad_subpixel_workspace_bytes(c.K, c.C, c.R, c.S, c.stride, c.pad)
    assert nb > 0
    dx = Guarded((c.N, c.H, c.W, c.C), F32)
    assert lib.dk_conv2d_dgrad_subpixel_f32(d["dy_d"].data_ptr(), c.N, d["OH"], d["OW"], c.K, d["w_d"].data_ptr(), c.C,
                                            c.R, c.S, c.stride, c.pad, dx.ptr, c.H, c.W, workspace.get(nb), nb, sh) == 0
    r = dgrad_ref(name, "subpixel")
    assert np.array_equal(r.ref, dgrad_ref(name, "phase").ref)
    R.check("dgrad-subpixel {} dx".format(name), nchw(dx.result()), r.ref, r.A)


# ---------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------

def untouched(*bufs):
    torch.cuda.synchronize()
    for b in bufs:
        ints = b.buf.view(b.itype)
        assert bool((ints == b.bits).all()), "a refused call wrote its output"


def test_narrow_refusals():
    """Status 10001 / 10002 exactly, nothing launched, and the next call on the stream works."""
    sh = stream_handle()
    # (C, R, S, stride, pad, N, H, W, K): one past the supported width at stride 2 (OW = 113) and stride 1 (OW = 129),
    # K = 68 > 64, K = 6 (K % 4), shapes not instantiated
    bad = [(3, 5, 5, 2, 1, 1, 5, 227, 64), (3, 3, 3, 1, 1, 1, 3, 129, 64), (3, 5, 5, 2, 1, 1, 7, 13, 68),
           (3, 5, 5, 2, 1, 1, 7, 13, 6), (2, 3, 3, 1, 1, 1, 5, 9, 16), (3, 5, 5, 1, 2, 1, 5, 9, 16)]
    for C, Rr, S, st, pad, N, H, W, K in bad:
        OH, OW = R.out_hw(H, W, Rr, S, st, pad)
        geom = (N, C, H, W, K, Rr, S, st, pad, OH, OW)
        assert lib.dk_conv2d_narrow_preferred(*geom) == 0
        assert lib.dk_conv2d_fwd_narrow_stats_rows(*geom) == 0
        assert lib.dk_conv2d_wgrad_narrow_workspace_bytes(*geom) == 0
        x = torch.zeros((N, C, H, W), device="cuda")
        w = torch.zeros((K, C, Rr, S), device="cuda")
        t = torch.zeros((N, OH, OW, roundup16(K)), device="cuda")
        bn = [torch.zeros(roundup16(K), device="cuda") for _ in range(4)]
        k12 = torch.zeros(2 * roundup16(K), device="cuda")
        y, dw = Guarded((N, OH, OW, K), F32), Guarded((K, C, Rr, S), F32)
        nb = 1 << 20
        refused(10001, lib.dk_conv2d_fwd_narrow_f32, x.data_ptr(), N, C, H, W, w.data_ptr(), K, Rr, S, st, pad, 0, y.ptr,
                OH, OW, 0, sh)
        refused(10001, lib.dk_conv2d_wgrad_narrow_f32, t.data_ptr(), x.data_ptr(), *geom, 0, 0.0, dw.ptr,
                workspace.get(nb), nb, sh)
        refused(10001, lib.dk_conv2d_wgrad_bnbwd_narrow_f32, t.data_ptr(), t.data_ptr(), x.data_ptr(), *geom,
                *(v.data_ptr() for v in bn), 1, k12.data_ptr(), 1, 0, 0.0, dw.ptr, workspace.get(nb), nb, sh)
        untouched(y, dw)
    # a supported shape: g_lattice = 3, and a workspace one byte short
    d = inputs("n4")
    c, geom = d["case"], narrow_geom(d)
    nb = lib.dk_conv2d_wgrad_narrow_workspace_bytes(*geom)
    dw = Guarded((c.K, c.C, c.R, c.S), F32)
    refused(10001, lib.dk_conv2d_wgrad_bnbwd_narrow_f32, d["g_d"].data_ptr(), d["x1_d"].data_ptr(), d["x_nchw"].data_ptr(),
            *geom, *po_ptrs(d, 1), d["k12_d"].data_ptr(), 3, 0, 0.0, dw.ptr, workspace.get(nb), nb, sh)
    refused(10002, lib.dk_conv2d_wgrad_narrow_f32, d["dy_d"].data_ptr(), d["x_nchw"].data_ptr(), *geom, 0, 0.0, dw.ptr,
            workspace.get(nb), nb - 1, sh)
    refused(10002, lib.dk_conv2d_wgrad_bnbwd_narrow_f32, d["g_d"].data_ptr(), d["x1_d"].data_ptr(), d["x_nchw"].data_ptr(),
            *geom, *po_ptrs(d, 1), d["k12_d"].data_ptr(), 1, 0, 0.0, dw.ptr, workspace.get(nb), nb - 1, sh)
    untouched(dw)
    assert lib.dk_conv2d_wgrad_narrow_f32(d["dy_d"].data_ptr(), d["x_nchw"].data_ptr(), *geom, 0, 0.0, dw.ptr,
                                          workspace.get(nb), nb, sh) == 0
    r = wgrad_ref("n4", 0.0, None)
    R.check("nwgrad n4 after refusals dw", dw.result(), r.ref, r.A)


def roundup16(v):
    return -(-v // 16) * 16


def test_dgrad_refusals():
    sh = stream_handle()
    d = inputs("s1")
    c, OH, OW = d["case"], d["OH"], d["OW"]
    dy, w = d["dy_d"].data_ptr(), d["w_d"].data_ptr()
    dx = Guarded((c.N, c.H, c.W, 17), F32)      # large enough for every call below
    big = 1 << 20
    # sub-pixel: C = 17, a geometry that is not instantiated, a short workspace
    assert lib.dk_conv2d_dgrad_subpixel_workspace_bytes(c.K, 17, c.R, c.S, 2, c.pad) == 0
    assert lib.dk_conv2d_dgrad_subpixel_workspace_bytes(c.K, c.C, 3, 3, 2, 2) == 0
    w17 = torch.zeros((c.K, 17, c.R, c.S), device="cuda")
    refused(10001, lib.dk_conv2d_dgrad_subpixel_f32, dy, c.N, OH, OW, c.K, w17.data_ptr(), 17, c.R, c.S, 2, c.pad, dx.ptr,
            c.H, c.W, workspace.get(big), big, sh)
    refused(10001, lib.dk_conv2d_dgrad_subpixel_f32, dy, c.N, OH, OW, c.K, w, c.C, 3, 3, 2, 2, dx.ptr, c.H, c.W,
            workspace.get(big), big, sh)
    nb = lib.dk_conv2d_dgrad_subpixel_workspace_bytes(c.K, c.C, c.R, c.S, c.stride, c.pad)
    refused(10002, lib.dk_conv2d_dgrad_subpixel_f32, dy, c.N, OH, OW, c.K, w, c.C, c.R, c.S, c.stride, c.pad, dx.ptr, c.H,
            c.W, workspace.get(big), nb - 1, sh)
    # phase: Kp != roundup4(K), a short workspace
    nbp = lib.dk_conv2d_dgrad_phase_workspace_bytes(c.K, c.C, c.R, c.S, c.stride)
    refused(10002, lib.dk_conv2d_dgrad_phase_f32, dy, c.N, OH, OW, c.K + 4, c.K, w, c.C, c.R, c.S, c.stride, c.pad, dx.ptr,
            c.H, c.W, workspace.get(big), big, sh)
    refused(10002, lib.dk_conv2d_dgrad_phase_f32, dy, c.N, OH, OW, c.K, c.K, w, c.C, c.R, c.S, c.stride, c.pad, dx.ptr,
            c.H, c.W, workspace.get(big), nbp - 1, sh)
    untouched(dx)
    dx = Guarded((c.N, c.H, c.W, c.C), F32)
    assert lib.dk_conv2d_dgrad_subpixel_f32(dy, c.N, OH, OW, c.K, w, c.C, c.R, c.S, c.stride, c.pad, dx.ptr, c.H, c.W,
                                            workspace.get(big), nb, sh) == 0
    r = dgrad_ref("s1", "subpixel")
    R.check("dgrad-subpixel s1 after refusals dx", nchw(dx.result()), r.ref, r.A)


def test_engine_forward_refusals():
    """C % 4 != 0 and a misaligned x, on all three forward entry points."""
    sh = stream_handle()
    d = inputs("e1")
    c, OH, OW = d["case"], d["OH"], d["OW"]
    geom = (c.K, c.R, c.S, c.stride, c.pad)
    x, w = d["x_d"].data_ptr(), d["krsc_d"].data_ptr()
    y = Guarded((c.N, OH, OW, c.K), F32)
    for xp, C in ((x, 3), (x, 6), (x + 4, c.Cp)):
        refused(10001, lib.dk_conv2d_fwd_f32, xp, c.N, c.H, c.W, C, w, *geom, 0, y.ptr, OH, OW, sh)
        refused(10001, lib.dk_conv2d_fwd_bnx_f32, xp, c.N, c.H, c.W, C, w, *geom, 0, y.ptr, OH, OW, *pi_ptrs(d, 1), sh)
        refused(10001, lib.dk_conv2d_fwd_ex_f32, xp, c.N, c.H, c.W, C, w, *geom, 0, y.ptr, OH, OW, *pi_ptrs(d, 1), 0, sh)
    untouched(y)
    assert lib.dk_conv2d_fwd_f32(x, c.N, c.H, c.W, c.Cp, w, *geom, 0, y.ptr, OH, OW, sh) == 0
    r = fwd_ref("e1", False, None)
    R.check("fwd e1 after refusals y", nchw(y.result()), r.ref, r.A)
