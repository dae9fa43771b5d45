"""Every output element of the bf16 dense-convolution entry points -- dk_conv2d_fwd_ex_bf16, dk_conv2d_dgrad_bf16,
dk_conv2d_dgrad_phase_bf16, dk_conv2d_wgrad_bf16 and dk_conv2d_wgrad_bnx_bf16 (gemm_bf16.hip) -- and the forward's
BatchNorm statistics against the fp64 reference of the same operation in its bf16 mode (tests/_conv_ref.py), each
under the bound derived there from the arithmetic, none excluded.  The twin of tests/test_gpu_conv_elementwise.py.

Cases: every _conv_ref.ENGINE case (their comments name the bf16 tile and split each reaches) and ENGINE16, the four
that reach what ENGINE does not under the bf16 rules: forward row config 16 with split-K config 4 (h1), both dgrads
on row config 16 (h2) and on config 6 (h4), and K % 8 == 4 (h3: 40-byte rows).  The phase dgrad also runs the SUBPIX
geometries.  Where an entry refuses a case (K = 6: the forward, the stride-1 dgrad and both weight gradients) the
refusal is asserted in the case's place.

Every entry runs twice: under the default knobs and with the row tile forced to config 8 (dk_debug_set_gemm_config
0 -> 8: 64 x 64 x 32, which the bf16 convolution rule never returns and which is instantiated for the bf16 MFMA mode
like every row configuration, gemm_engine.h igemm_rows) and the split-K tile forced to a configuration the shape does
not pick (1 -> config 1 where it picks 6 or 4, else 6); both restored in a finally.  The row and workspace queries are
called inside the same routing: they read the knobs.

Outputs are guarded (tests/_guard.py): 16-byte-aligned slices of NaN-bit-filled buffers whose 64-element margins must
stay intact and in which no element may remain NaN.  Statistics are pre-filled with NaN, rows + 1 rows allocated:
every row dk_conv2d_fwd_bf16_stats_rows() reports must have been written and the extra one must stay NaN.

What the library's queries confirm about the routes, and what they cannot: dk_conv2d_fwd_bf16_stats_rows gives the row
tile's height (every case: ceil(M / 128) under configs 14 / 15 / 16, ceil(M / 64) under 6 and under the forced 8;
test_forced_route_is_another_tile); it cannot tell config 16 from 15, which differ in columns -- those follow from
row_config as read (_conv_ref's rules paragraph).  dk_conv2d_wgrad_bf16_workspace_bytes equals splits x K x R S Cp x 4
of the picked split-K configuration at every case, but at these sizes the splits are capped by the ceil(M / 32) k-tiles
all three configurations share, so the forced configuration asks for the same bytes.  The dgrads have no query.

Worst err / bound per family on an MI355X, default and forced tiles together (recorded with DORKNET_SLACK_LOG;
results, not tolerances; 1753 logged checks in all, the refusal tests' follow-up calls included).  A bf16 store attains
the interval form's end by construction -- 1.000 is at the bound, never past it -- the closed form's figure in
brackets:

    family                                          checks        worst
    forward y (interval and closed)                  2 x 361      1.000 (0.983)
      statistics | stored   (sum, squares)           2 x 181      0, 0.011
      statistics | reference                         2 x 181      0.676, 0.856
    dgrad dx  stride 1 (dk_conv2d_dgrad_bf16)        2 x 16       1.000 (0.967)
              phase                                  2 x 47       1.000 (0.975)
    wgrad dw  plain / bnx                           60 / 121      0.026 / 0.729

The fp32 quantities: dw of raw operands stays below 3 % of its bound and the statistics agree with the fp64 sums of
the stored y to 1.1 % of the 2^-53-scale bound (the sums exactly), so neither the one-ulp-per-step model of
v_mfma_f32_32x32x16_bf16 nor the fp64 accumulation is strained.  The two larger figures are not fp32 arithmetic: dw
behind a BatchNorm on load (0.729 at h4, M = 30) and the statistics against the reference (0.856 at e10, M = 30) are
measured against sums of the 2^-8 bf16 roundings of the operand / of the stored y, which 30 terms cancel little; the
honest host implementation of tests/test_conv_ref_host.py reaches 0.816 and 0.999 of the same bounds.  No kernel
defect was found, no entry accepted arguments it could not serve, and no constant of _conv_ref.py was moved.

What the file catches, tried once on a build with rnd4<bf16_t> (dk_common.h) truncating instead of rounding to nearest
even: 47 of the 114 tests fail -- every forward and every stride-1 dgrad test and the refusal test's follow-up
forward, each already at the closed form, which is checked first (1.05 to 1.96 of it: a whole ulp against a half).
The phase dgrad passes on that build, rightly: EpPhaseT converts in st4 and never calls rnd4.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

from dorknet_amd._hip import lib, stream_handle, workspace
from tests import _conv_ref as R
from tests._guard import Guarded
from tests.test_gpu_conv_elementwise import host, nan_rows, nchw, refused, untouched, vec

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
L2 = R.L2
ROUTES = ("default", "forced")
ZERO5 = (0, 0, 0, 0, 0)
NAMES = list(R.ENGINE) + list(R.ENGINE16)
DGRAD_NAMES = NAMES + list(R.SUBPIX)
DEAD = ("e6", "e12")      # cases with dx pixels no tap reaches


def split_pick(c):
    """The split-K configuration the bf16 rule picks (gemm_engine.h splitk_config, M = K filters, N = R S Cp)."""
    n = c.R * c.S * c.Cp
    return 4 if c.K >= 128 and n >= 128 else (6 if c.K <= 64 < n else 1)


@contextlib.contextmanager
def routing(route, c):
    if route == "default":
        yield
        return
    try:
        lib.dk_debug_set_gemm_config(0, 8)
        lib.dk_debug_set_gemm_config(1, 1 if split_pick(c) in (6, 4) else 6)
        yield
    finally:
        lib.dk_debug_set_gemm_config(0, -1)
        lib.dk_debug_set_gemm_config(1, -1)


def nhwc16(a, cp=None):
    """An NCHW host array of bf16-representable values on the device as bf16 NHWC, the channels zero-padded to cp."""
    a = np.asarray(a, dtype=np.float32).transpose(0, 2, 3, 1)
    if cp is not None and cp != a.shape[3]:
        a = np.concatenate([a, np.zeros(a.shape[:3] + (cp - a.shape[3],), np.float32)], axis=3)
    t = torch.as_tensor(np.ascontiguousarray(a))
    assert torch.equal(t.to(BF16).float(), t)
    return t.to(BF16).cuda()


@functools.lru_cache(maxsize=None)
def inputs(name):
    d = R.make_inputs(name)
    c = d["case"]
    st = stream_handle()
    d["x_d"] = nhwc16(d["x"], c.Cp)
    d["dy_d"], d["dyp_d"] = nhwc16(d["dy"]), nhwc16(d["dy"], R.roundup4(c.K))
    d["w_d"], d["bias_d"] = vec(d["w"]), vec(d["bias"])
    d["pi_d"] = [vec(v) for v in d["pi"]]
    d["krsc_d"] = torch.empty((c.K, c.R, c.S, c.Cp), dtype=F32, device="cuda")
    lib.dk_conv_weight_krsc_f32(d["w_d"].data_ptr(), c.K, c.C, c.R, c.S, c.Cp, d["krsc_d"].data_ptr(), st)
    d["crsk_d"] = torch.empty((c.C, c.R, c.S, c.K), dtype=F32, device="cuda")
    lib.dk_conv_weight_crsk_f32(d["w_d"].data_ptr(), c.K, c.C, c.R, c.S, d["crsk_d"].data_ptr(), st)
    torch.cuda.synchronize()
    return d


def pi_ptrs(d, relu):
    return ZERO5 if relu is None else (*(t.data_ptr() for t in d["pi_d"]), relu)


@functools.lru_cache(maxsize=None)
def fwd_ref(name, bias, bn):
    return R.forward(inputs(name), bias, bn, bf16=True)


@functools.lru_cache(maxsize=None)
def dgrad_ref(name, entry):
    return R.dgrad(inputs(name), entry, bf16=True)


@functools.lru_cache(maxsize=None)
def wgrad_ref(name, l2, bn):
    return R.wgrad(inputs(name), l2, bn, bf16=True)


def stored16(name, got, r):
    """A bf16 store against the closed form of one rounding store and the interval form that implies it, each
    logged under its own name."""
    R.check(name + " closed", got, r.ref, r.b16c)
    R.check(name, got, r.ref, r.b16)


def fwd_args(d, bias, bn, y, part):
    c = d["case"]
    return (d["x_d"].data_ptr(), c.N, c.H, c.W, c.Cp, d["krsc_d"].data_ptr(), c.K, c.R, c.S, c.stride, c.pad,
            d["bias_d"].data_ptr() if bias else 0, y, d["OH"], d["OW"], *pi_ptrs(d, bn), part, stream_handle())


def phase_args(d, dx, ws, nb):
    c = d["case"]
    return (d["dyp_d"].data_ptr(), c.N, d["OH"], d["OW"], R.roundup4(c.K), c.K, d["w_d"].data_ptr(), c.C, c.R, c.S,
            c.stride, c.pad, dx, c.H, c.W, ws, nb, stream_handle())


def gemm_args(d, dx):
    c = d["case"]
    return (d["dy_d"].data_ptr(), c.N, d["OH"], d["OW"], c.K, d["crsk_d"].data_ptr(), c.C, c.R, c.S, c.pad, dx, c.H,
            c.W, stream_handle())


def wgrad_args(d, l2, dw, ws, nb):
    c = d["case"]
    return (d["dy_d"].data_ptr(), d["x_d"].data_ptr(), c.N, c.H, c.W, c.Cp, c.C, c.K, c.R, c.S, c.stride, c.pad,
            d["OH"], d["OW"], d["w_d"].data_ptr() if l2 else 0, l2, dw, ws, nb)


# ---------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", NAMES)
def test_forward(name, route):
    """Bias off / on x BatchNorm none / on load / with ReLU x statistics off / on."""
    d = inputs(name)
    c, OH, OW = d["case"], d["OH"], d["OW"]
    with routing(route, c):
        if c.K % 4:
            y = Guarded((c.N, OH, OW, c.K), BF16)
            refused(10001, lib.dk_conv2d_fwd_ex_bf16, *fwd_args(d, False, None, y.ptr, 0))
            untouched(y)
            return
        rows = lib.dk_conv2d_fwd_bf16_stats_rows(c.N, OH, OW, c.K, c.Cp, c.R, c.S)
        assert rows > 0
        for bias in (False, True):
            for bn in (None, 0, 1):
                r = fwd_ref(name, bias, bn)
                for stats in (False, True):
                    part = nan_rows(rows, c.K) if stats else None
                    y = Guarded((c.N, OH, OW, c.K), BF16)
                    assert lib.dk_conv2d_fwd_ex_bf16(*fwd_args(d, bias, bn, y.ptr, part.data_ptr() if stats else 0)) == 0
                    got = nchw(y.result())
                    stored16("bf16 fwd {} {} y".format(name, route), got, r)
                    if stats:
                        s = host(part)
                        assert np.isnan(s[rows]).all(), "{}: a row past the reported {} was written".format(name, rows)
                        R.stats_checks("bf16 fwd {} {} stats".format(name, route), s[:rows], got, r.ref, r.b16)


def test_forced_route_is_another_tile():
    """h1 (M = 162): two 128-row tiles by default (row config 16), three 64-row tiles under the forced config 8."""
    c = R.ENGINE16["h1"]
    OH, OW = R.case_hw(c)
    rows = {}
    for route in ROUTES:
        with routing(route, c):
            rows[route] = lib.dk_conv2d_fwd_bf16_stats_rows(c.N, OH, OW, c.K, c.Cp, c.R, c.S)
    assert rows == {"default": 2, "forced": 3}


# ---------------------------------------------------------------------------------------------------------
# input gradient
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", DGRAD_NAMES)
def test_dgrad(name, route):
    """dk_conv2d_dgrad_phase_bf16 at every case (dy zero-padded to Kp as the layer does; K = 6 in Kp = 8 at e11 and
    s3), dk_conv2d_dgrad_bf16 at the stride-1 cases with K % 4 == 0, refused (10001) at the others of stride 1."""
    d = inputs(name)
    c = d["case"]
    with routing(route, c):
        nb = lib.dk_conv2d_dgrad_phase_workspace_bytes(c.K, c.C, c.R, c.S, c.stride)
        assert nb == c.C * c.R * c.S * R.roundup4(c.K) * 4
        dx = Guarded((c.N, c.H, c.W, c.C), BF16)
        assert lib.dk_conv2d_dgrad_phase_bf16(*phase_args(d, dx.ptr, workspace.get(nb), nb)) == 0
        r = dgrad_ref(name, "phase")
        got = nchw(dx.result())
        stored16("bf16 dgrad-phase {} {} dx".format(name, route), got, r)
        if name in DEAD:    # the phases / rows no tap reaches: written, and exact zeros
            dead = R.conv_dx(np.ones_like(d["dy"]), np.ones(d["w"].shape), c.stride, c.pad, c.H, c.W) == 0
            assert dead.any() and (got[dead] == 0).all() and (r.b16[dead] == 0).all()
        if c.stride != 1:
            return
        dx = Guarded((c.N, c.H, c.W, c.C), BF16)
        if c.K % 4:
            refused(10001, lib.dk_conv2d_dgrad_bf16, *gemm_args(d, dx.ptr))
            untouched(dx)
            return
        assert lib.dk_conv2d_dgrad_bf16(*gemm_args(d, dx.ptr)) == 0
        stored16("bf16 dgrad-gemm {} {} dx".format(name, route), nchw(dx.result()), dgrad_ref(name, "gemm"))


# ---------------------------------------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", NAMES)
def test_wgrad(name, route):
    """l2 = 0 / L2 x plain / BatchNorm on load without / with ReLU.  e4, e5 (C = 3 in Cp = 4): the reduce compacts
    Cp -> C and bn(0) != 0 of the padded channel must not reach dw."""
    d = inputs(name)
    c, sh = d["case"], stream_handle()
    with routing(route, c):
        nb = lib.dk_conv2d_wgrad_bf16_workspace_bytes(c.N, d["OH"], d["OW"], c.K, c.Cp, c.R, c.S)
        assert nb >= c.K * c.R * c.S * c.Cp * 4
        if c.K % 4:
            dw = Guarded((c.K, c.C, c.R, c.S), F32)
            refused(10001, lib.dk_conv2d_wgrad_bf16, *wgrad_args(d, 0.0, dw.ptr, workspace.get(nb), nb), sh)
            refused(10001, lib.dk_conv2d_wgrad_bnx_bf16, *wgrad_args(d, 0.0, dw.ptr, workspace.get(nb), nb),
                    *pi_ptrs(d, 1), sh)
            untouched(dw)
            return
        for l2 in (0.0, L2):
            dw = Guarded((c.K, c.C, c.R, c.S), F32)
            assert lib.dk_conv2d_wgrad_bf16(*wgrad_args(d, l2, dw.ptr, workspace.get(nb), nb), sh) == 0
            r = wgrad_ref(name, l2, None)
            R.check("bf16 wgrad-plain {} {} dw".format(name, route), dw.result(), r.ref, r.A)
            for relu in (0, 1):
                dw = Guarded((c.K, c.C, c.R, c.S), F32)
                assert lib.dk_conv2d_wgrad_bnx_bf16(*wgrad_args(d, l2, dw.ptr, workspace.get(nb), nb), *pi_ptrs(d, relu),
                                                    sh) == 0
                r = wgrad_ref(name, l2, relu)
                R.check("bf16 wgrad-bnx {} {} dw".format(name, route), dw.result(), r.ref, r.A)


# ---------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------

def test_forward_refusals():
    """Exact status, y and the statistics bitwise untouched, and the next call on the stream within its bound."""
    d, d11 = inputs("e1"), inputs("e11")
    c = d["case"]
    y = Guarded((c.N, d["OH"], d["OW"], c.K), BF16)
    rows = lib.dk_conv2d_fwd_bf16_stats_rows(c.N, d["OH"], d["OW"], c.K, c.Cp, c.R, c.S)
    part = nan_rows(rows, c.K)
    good = fwd_args(d, True, 1, y.ptr, part.data_ptr())

    def swap(i, v):
        return good[:i] + (v,) + good[i + 1:]
    refused(10001, lib.dk_conv2d_fwd_ex_bf16, *fwd_args(d11, False, None, y.ptr, 0))     # K = 6
    for C in (3, 6):                                                                       # C % 4 != 0
        refused(10001, lib.dk_conv2d_fwd_ex_bf16, *swap(4, C))
    refused(10001, lib.dk_conv2d_fwd_ex_bf16, *swap(0, good[0] + 4))                       # x 4 bytes off
    refused(10001, lib.dk_conv2d_fwd_ex_bf16, *swap(12, y.ptr + 4))                        # y 4 bytes off
    refused(10001, lib.dk_conv2d_fwd_ex_bf16, *swap(11, good[11] + 4))                     # a misaligned bias
    untouched(y)
    assert bool(torch.isnan(part).all()), "a refused call wrote its statistics"
    assert lib.dk_conv2d_fwd_ex_bf16(*good) == 0
    r = fwd_ref("e1", True, 1)
    got = nchw(y.result())
    stored16("bf16 fwd e1 after refusals y", got, r)
    s = host(part)
    assert np.isnan(s[rows]).all()
    R.stats_checks("bf16 fwd e1 after refusals stats", s[:rows], got, r.ref, r.b16)


def test_dgrad_refusals():
    d = inputs("e1")
    c, sh = d["case"], stream_handle()
    K = c.K
    nb = lib.dk_conv2d_dgrad_phase_workspace_bytes(K, c.C, c.R, c.S, c.stride)
    dx = Guarded((c.N, c.H, c.W, c.C), BF16)
    good = phase_args(d, dx.ptr, workspace.get(nb), nb)
    wide = torch.zeros((c.N, d["OH"], d["OW"], K + 4), dtype=BF16, device="cuda")     # room for every Kp below
    for Kp in (K - 4, K + 2):                                                          # Kp < K, Kp % 4 != 0
        refused(10001, lib.dk_conv2d_dgrad_phase_bf16, wide.data_ptr(), *good[1:4], Kp, *good[5:])
    refused(10002, lib.dk_conv2d_dgrad_phase_bf16, *good[:-2], nb - 1, sh)             # a workspace one byte short
    d11 = inputs("e11")
    refused(10001, lib.dk_conv2d_dgrad_bf16, *gemm_args(d11, dx.ptr))                  # K = 6 (dx is large enough)
    untouched(dx)
    assert lib.dk_conv2d_dgrad_phase_bf16(*good) == 0
    stored16("bf16 dgrad-phase e1 after refusals dx", nchw(dx.result()), dgrad_ref("e1", "phase"))


def test_wgrad_refusals():
    d, d11 = inputs("e1"), inputs("e11")
    c, sh = d["case"], stream_handle()
    nb = lib.dk_conv2d_wgrad_bf16_workspace_bytes(c.N, d["OH"], d["OW"], c.K, c.Cp, c.R, c.S)
    dw = Guarded((c.K, c.C, c.R, c.S), F32)
    ws = workspace.get(nb)
    good = wgrad_args(d, L2, dw.ptr, ws, nb)
    bn = pi_ptrs(d, 1)
    for fn, tail in ((lib.dk_conv2d_wgrad_bf16, (sh,)), (lib.dk_conv2d_wgrad_bnx_bf16, (*bn, sh))):
        refused(10001, fn, *wgrad_args(d11, 0.0, dw.ptr, ws, nb), *tail)               # K = 6 (dw is large enough)
        refused(10001, fn, *good[:5], 6, 6, *good[7:], *tail)                          # Cp % 4 != 0
        refused(10001, fn, good[0], good[1] + 4, *good[2:], *tail)                     # x 4 bytes off
        refused(10002, fn, *good[:-1], nb - 1, *tail)                                  # a workspace one byte short
    untouched(dw)
    assert lib.dk_conv2d_wgrad_bnx_bf16(*good, *bn, sh) == 0
    r = wgrad_ref("e1", L2, 1)
    R.check("bf16 wgrad-bnx e1 after refusals dw", dw.result(), r.ref, r.A)
