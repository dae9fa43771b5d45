"""Every output element of the pointwise entry points -- forward, input gradient (plain, widened, lattice,
BatchNorm-backward on load), weight gradient and the fused backward, fp32 and bf16 storage -- and their
BatchNorm statistics / backward partials against the fp64 reference of the same operation (tests/_pw_ref.py),
each under the bound derived there from the arithmetic, none excluded.  The cases (_pw_ref.CASES) are the smallest
that reach each kernel family (streaming, deep, tiled engine, scalar loaders) and each tile edge: a single
partial tile, a full tile plus one pixel, two whole tiles, 429 pixels (ragged for 32, 64 and 128) and stride 2
on odd H and W.

Every entry point runs twice: under the default knobs (the specialised kernels) and with the streaming / deep /
fused-deep kernels off (dk_debug_set_gemm_config 3, 9, 11, 13, 14 = 0, restored in a finally), so that every
route is held to the reference directly and not through another kernel.

Outputs are guarded (tests/_guard.py): 16-byte-aligned slices of NaN-bit-filled buffers whose 64-element margins
must stay intact and in which no element may remain NaN; statistics and partial rows are pre-filled with NaN,
so every row the *_rows() query reports must have been written.

Refusals asserted (status 10001, nothing else):
  * C % 4 != 0 (cases 20 to 24): dk_pwconv_fwd_ex_f32, dk_pwconv_wgrad_f32 / _bnx_f32, dk_pwconv_dgrad_bnbwd_f32,
    dk_pwconv_bwd_bnbwd_f32 and every bf16 entry point (the plain dk_pwconv_fwd_f32 and dk_pwconv_dgrad_ex_f32
    take them on scalar loaders);
  * partials together with a residual at stride > 1 (dk_pwconv_dgrad_ex_f32 / _bf16);
  * dk_pwconv_dgrad_lattice_f32 at stride 1;
  * the fused backward where dk_pwconv_bwd_fused_rows / _bf16_rows is 0 (K = 512, K or C = 24 / 40 / 16 / 3;
    bf16 K = 64 with C = 128; every bf16 shape with the specialised kernels off), and at the deep kernel's
    shapes an input BatchNorm without its partials;
  * dk_pwconv_bwd_bnbwd_lattice_f32 unless K = C = 64 on the streaming kernel.

Worst err / bound per family on an MI355X, default and tiled routes together (recorded with DORKNET_SLACK_LOG;
results, not tolerances; bf16 stores attain the interval form's end by construction -- 1.000 is at the bound,
never past it -- the closed form's figure in brackets):

    family                              checks   fp32          checks   bf16
    forward y                              456   0.041            456   1.000 (0.990)
      plain entry (stride 2, C % 4)         24   0.177
      statistics | stored                  228   0, 0.248         228   0, 0.015     (sum, squares)
      statistics | reference               228   0.005, 0.008     228   1.000, 1.000
    dgrad dx (widened zeros exact)         236   0.069            212   1.000 (0.994)
      partials | stored                    152   0, 0.755         136   0, 0.755     (g, g x_hat)
      partials | reference                 152   0.009, 0.010     136   1.000, 1.000
    lattice dgrad dx / partials              8   0.050 / 0.300
    dgrad_bnbwd dx                         480   0.131            480   1.000 (0.741)
      dy_out                               240   0.624            240   1.000 (0.996)
      dx against stored dy_out             240   0.123            240   1.000 (0.991)
      partials | stored / reference        240   0.755 / 0.014    240   0.755 / 1.000
    wgrad dw                               152   0.190            152   0.950
    fused backward dx / dw                 152   0.044 / 0.182     88   1.000 (0.661) / 0.900
      partials | stored / reference         76   0.755 / 0.014     44   0.755 / 1.000
    fused lattice backward dx / dw           4   0.028 / 0.031

The fp32 GEMM outputs stay below a fifth of the 2 u-per-step bound on every route, so the one-ulp model of
the MFMA (tests/_pw_ref.py) is not strained and the constant stands as derived.  No kernel defect was found.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

from dorknet_amd._hip import HipError, lib, stream_handle, workspace
from tests import _pw_ref as P
from tests._guard import Guarded

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
F32 = torch.float32
L2 = float(np.float32(1e-3))
CIDS = sorted(P.CASES)
S1 = [c for c in CIDS if P.CASES[c][2] == 1]
KNOBS = (3, 9, 11, 13, 14)
ROUTES = ("default", "tiled")
ZERO5 = (0, 0, 0, 0, 0)


@contextlib.contextmanager
def routing(route):
    """"tiled": the streaming, deep and fused-deep kernels off for the calls inside."""
    if route == "default":
        yield
        return
    try:
        for k in KNOBS:
            lib.dk_debug_set_gemm_config(k, 0)
        yield
    finally:
        for k in KNOBS:
            lib.dk_debug_set_gemm_config(k, -1)


def nchw(a):
    return a.transpose(0, 3, 1, 2)


def dev(a, dtype):
    """An NCHW host array on the device as NHWC of the storage type (the values are bf16-representable)."""
    t = torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float32).transpose(0, 2, 3, 1)))
    return t.to(dtype).cuda()


def vec(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def nan_rows(rows, n):
    return torch.full((rows, 2, n), float("nan"), dtype=torch.float64, device="cuda")


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def inputs(cid):
    d = P.make_inputs(cid)
    d["dev"] = {(k, dt): dev(d[k], dt) for k in ("x", "xg", "dy", "g", "x1", "res") for dt in (F32, BF16)}
    d["w_d"], d["bias_d"], d["k12_d"] = vec(d["w"]), vec(d["bias"]), vec(d["k12"])
    d["pi_d"] = [vec(v) for v in d["pi"]]
    d["po_d"] = [vec(v) for v in d["po"]]
    return d


def dims(d):
    return tuple(d[k] for k in ("N", "H", "W", "C", "K", "stride", "OH", "OW"))


def p_(d, key, dt):
    return d["dev"][key, dt].data_ptr()


def pi_ptrs(d, relu):
    return (*(t.data_ptr() for t in d["pi_d"]), relu)


def po_ptrs(d, relu):
    return (*(t.data_ptr() for t in d["po_d"]), relu)


def nm(dt):
    return "bf16" if dt == BF16 else "f32"


def stored_check(name, got, r, dt):
    """A stored activation against its bound: fp32 the arithmetic's; bf16 the closed form of one rounding store
    and the interval form that implies it, each logged under its own name."""
    if dt == BF16:
        P.check(name + " closed", got, r.ref, r.b16c)
    P.check(name, got, r.ref, r.bound(dt == BF16))


def refused(fn, *args):
    with pytest.raises(HipError, match="10001"):
        fn(*args)


@functools.lru_cache(maxsize=None)
def fwd_ref(cid, bias, bn, bf16):
    d = inputs(cid)
    return P.forward(d["x"], d["w"], d["stride"], d["bias"] if bias else None,
                     None if bn is None else (*d["pi"], bn), bf16)


@functools.lru_cache(maxsize=None)
def dgrad_ref(cid, res, bf16, lattice=False):
    d = inputs(cid)
    return P.dgrad(d["dy"], d["w"], d["stride"], d["res"] if res else None, bf16=bf16, lattice=lattice)


@functools.lru_cache(maxsize=None)
def dy_ref(cid, relu):
    d = inputs(cid)
    return P.bn_bwd_dy(d["g"], d["x1"], (*d["po"], relu), d["k12"])[:2]


@functools.lru_cache(maxsize=None)
def bnbwd_dx_ref(cid, relu, res, bf16, lattice=False):
    d = inputs(cid)
    dy, ed = dy_ref(cid, relu)
    return P.dgrad(dy, d["w"], 1, d["res"] if res else None, ed, bf16, True, lattice)


@functools.lru_cache(maxsize=None)
def fused_dw_ref(cid, relu, bn, bf16):
    d = inputs(cid)
    dy, ed = dy_ref(cid, relu)
    fw = fwd_ref(cid, False, bn, bf16)
    return P.wgrad(dy, fw.a, d["w"], L2, P.operand_err(dy, ed, bf16), fw.ea)


# ---------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("cid", CIDS)
def test_forward(cid, route):
    d = inputs(cid)
    N, H, W, C, K, st, OH, OW = dims(d)
    with routing(route):
        for dt in (F32, BF16):
            bf = dt == BF16
            fn = lib.dk_pwconv_fwd_ex_bf16 if bf else lib.dk_pwconv_fwd_ex_f32
            for bias in (False, True):
                for bn in (None, 0, 1):
                    for stats in (False, True):
                        y = Guarded((N, OH, OW, K), dt)
                        bnp = ZERO5 if bn is None else pi_ptrs(d, bn)
                        if C % 4:
                            refused(fn, p_(d, "x", dt), N, H, W, C, d["w_d"].data_ptr(), K, st, 0, y.ptr, OH, OW, *bnp, 0,
                                    stream_handle())
                            continue
                        rows = (lib.dk_pwconv_fwd_bf16_strided_stats_rows(N, OH, OW, K, C, st) if bf
                                else lib.dk_pwconv_fwd_stats_rows(N, OH, OW, K, C))
                        assert rows > 0
                        part = nan_rows(rows, K) if stats else None
                        rc = fn(p_(d, "x", dt), N, H, W, C, d["w_d"].data_ptr(), K, st,
                                d["bias_d"].data_ptr() if bias else 0, y.ptr, OH, OW, *bnp,
                                part.data_ptr() if stats else 0, stream_handle())
                        assert rc == 0
                        r = fwd_ref(cid, bias, bn, bf)
                        got = nchw(y.result())
                        name = "fwd {} c{} {}".format(nm(dt), cid, route)
                        stored_check(name + " y", got, r, dt)
                        if stats:
                            P.stats_checks(name + " stats", host(part), got, r.ref, r.bound(bf))
        if st > 1 or C % 4:
            # the entry point without the optional operands: the strided skip projections; scalar loaders
            for bias in (False, True):
                y = Guarded((N, OH, OW, K), F32)
                args = (p_(d, "x", F32), N, H, W, C, d["w_d"].data_ptr(), K, st, d["bias_d"].data_ptr() if bias else 0,
                        y.ptr, OH, OW, stream_handle())
                if st > 1 and C % 4:  # the scalar loaders read plain rows: stride 1 only
                    refused(lib.dk_pwconv_fwd_f32, *args)
                    continue
                assert lib.dk_pwconv_fwd_f32(*args) == 0
                r = fwd_ref(cid, bias, None, False)
                P.check("fwd f32 c{} {} plain y".format(cid, route), nchw(y.result()), r.ref, r.A)


# ---------------------------------------------------------------------------------------------------------
# input gradient
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("cid", CIDS)
def test_dgrad(cid, route):
    d = inputs(cid)
    N, H, W, C, K, st, OH, OW = dims(d)
    with routing(route):
        for dt in (F32, BF16):
            bf = dt == BF16
            fn = lib.dk_pwconv_dgrad_ex_bf16 if bf else lib.dk_pwconv_dgrad_ex_f32
            for res in (False, True):
                for relu in (None, 0, 1):       # None: without the input BatchNorm's partials
                    dx = Guarded((N, OH * st, OW * st, C), dt)
                    rows = (lib.dk_pwconv_dgrad_bf16_stats_rows(N, OH, OW, K, C, st) if bf
                            else lib.dk_pwconv_dgrad_stats_rows(N, OH, OW, K, C))
                    part = nan_rows(max(rows, 1), C) if relu is not None else None
                    args = (p_(d, "dy", dt), N, OH, OW, K, d["w_d"].data_ptr(), C, st, dx.ptr,
                            p_(d, "res", dt) if res else 0,
                            *((p_(d, "xg", dt), *pi_ptrs(d, relu), part.data_ptr()) if part is not None
                              else (0, 0, 0, 0, 0, 0, 0)), stream_handle())
                    if (bf and C % 4) or (part is not None and res and st != 1):
                        refused(fn, *args)
                        continue
                    assert rows > 0
                    assert fn(*args) == 0
                    r = dgrad_ref(cid, res, bf)
                    got = nchw(dx.result())
                    name = "dgrad {} c{} {}".format(nm(dt), cid, route)
                    stored_check(name + " dx", got, r, dt)      # (the widened zeros: bound 0, exactly 0)
                    if part is not None:
                        P.part_checks(name + " part", host(part), P.sample(got, st), P.sample(d["xg"], st),
                                      (*d["pi"], relu), P.sample(r.ref, st), P.sample(r.bound(bf), st))
        # the compact lattice form (fp32, stride > 1)
        rows = lib.dk_pwconv_dgrad_stats_rows(N, OH, OW, K, C)
        dx, part = Guarded((N, OH, OW, C), F32), nan_rows(rows, C)
        args = (p_(d, "dy", F32), N, OH, OW, K, d["w_d"].data_ptr(), C, st, dx.ptr, p_(d, "xg", F32), *pi_ptrs(d, 1),
                part.data_ptr(), stream_handle())
        if st == 1:
            refused(lib.dk_pwconv_dgrad_lattice_f32, *args)
        else:
            assert lib.dk_pwconv_dgrad_lattice_f32(*args) == 0
            r = dgrad_ref(cid, False, False, True)
            got = nchw(dx.result())
            name = "lattice f32 c{} {}".format(cid, route)
            P.check(name + " dx", got, r.ref, r.A)
            P.part_checks(name + " part", host(part), got, P.sample(d["xg"], st), (*d["pi"], 1), r.ref, r.A)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("cid", S1)
def test_dgrad_bnbwd(cid, route):
    """dy = the following BatchNorm's backward formed on load, written through to dy_out; dx (+ residual) and the
    input BatchNorm's partials.  Where dy_out is stored, dx is also held to dgrad(dy_out as stored) with E = 0."""
    d = inputs(cid)
    N, H, W, C, K, st, OH, OW = dims(d)
    with routing(route):
        for dt in (F32, BF16):
            bf = dt == BF16
            fn = lib.dk_pwconv_dgrad_bnbwd_bf16 if bf else lib.dk_pwconv_dgrad_bnbwd_f32
            rows = (lib.dk_pwconv_dgrad_bnbwd_bf16_stats_rows if bf else lib.dk_pwconv_dgrad_bnbwd_stats_rows)(
                N, OH, OW, K, C)
            for relu in (0, 1):
                for store_dy in (False, True):
                    for bn_in in (False, True):
                        for res in (False, True):
                            dx, dyo = Guarded((N, OH, OW, C), dt), Guarded((N, OH, OW, K), dt)
                            part = nan_rows(max(rows, 1), C) if bn_in else None
                            args = (p_(d, "g", dt), p_(d, "x1", dt), N, OH, OW, K, *po_ptrs(d, relu),
                                    d["k12_d"].data_ptr(), dyo.ptr if store_dy else 0, d["w_d"].data_ptr(), C, dx.ptr,
                                    p_(d, "res", dt) if res else 0,
                                    *((p_(d, "x", dt), *pi_ptrs(d, 1), part.data_ptr()) if bn_in
                                      else (0, 0, 0, 0, 0, 0, 0)), stream_handle())
                            if C % 4:
                                refused(fn, *args)
                                continue
                            assert rows > 0
                            assert fn(*args) == 0
                            r = bnbwd_dx_ref(cid, relu, res, bf)
                            got = nchw(dx.result())
                            name = "bnbwd {} c{} {}".format(nm(dt), cid, route)
                            stored_check(name + " dx", got, r, dt)
                            if bn_in:
                                P.part_checks(name + " part", host(part), got, d["x"], (*d["pi"], 1), r.ref, r.bound(bf))
                            if store_dy:
                                dy, ed = dy_ref(cid, relu)
                                dys = nchw(dyo.result())
                                if bf:
                                    P.check(name + " dy_out closed", dys, dy, P.bf16_closed(dy, ed))
                                P.check(name + " dy_out", dys, dy, P.bf16_bound(dy, ed) if bf else ed)
                                stored_check(name + " dx|dy_out", got,
                                             P.dgrad(dys, d["w"], 1, d["res"] if res else None, bf16=bf), dt)


# ---------------------------------------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("cid", CIDS)
def test_wgrad(cid, route):
    d = inputs(cid)
    N, H, W, C, K, st, OH, OW = dims(d)
    nb = lib.dk_pwconv_wgrad_workspace_bytes(N, OH, OW, K, C)
    with routing(route):
        for dt in (F32, BF16):
            bf = dt == BF16
            for l2 in (0.0, L2):
                for bn in (None, 1):
                    dw = Guarded((K, C), F32)
                    args = (p_(d, "dy", dt), p_(d, "x", dt), N, H, W, C, K, st, OH, OW, d["w_d"].data_ptr(), l2, dw.ptr,
                            workspace.get(nb), nb)
                    if bf:
                        fn, args = lib.dk_pwconv_wgrad_bnx_bf16, args + (ZERO5 if bn is None else pi_ptrs(d, bn))
                    elif bn is None:
                        fn = lib.dk_pwconv_wgrad_f32
                    else:
                        fn, args = lib.dk_pwconv_wgrad_bnx_f32, args + pi_ptrs(d, bn)
                    if C % 4:
                        refused(fn, *args, stream_handle())
                        continue
                    assert fn(*args, stream_handle()) == 0
                    fw = fwd_ref(cid, False, bn, bf)
                    r = P.wgrad(d["dy"], fw.a, d["w"], l2, None, fw.ea)
                    P.check("wgrad {} c{} {} dw".format(nm(dt), cid, route), dw.result(), r.ref, r.A)


# ---------------------------------------------------------------------------------------------------------
# fused backward
# ---------------------------------------------------------------------------------------------------------

# the stride-1 cases for which dk_pwconv_bwd_fused_rows / _bf16_rows is positive
FUSED = {
    ("default", F32): [1, 2, 4, 5, 6, 8, 9, 10, 11, 12, 14, 15],    # K, C in {64, 128}; K in {128, 256}, C % 128 == 0
    ("tiled", F32): [1, 2, 4, 5, 6, 8, 9],                          # the tiled fused kernel: K, C in {64, 128}
    ("default", BF16): [1, 2, 4, 5, 8, 9, 10, 11, 12, 14, 15],      # K = C = 64; K in {128, 256} (not K = 64, C = 128)
    ("tiled", BF16): [],
}


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("cid", S1)
def test_fused_backward(cid, route):
    d = inputs(cid)
    N, H, W, C, K, st, OH, OW = dims(d)
    with routing(route):
        for dt in (F32, BF16):
            bf = dt == BF16
            fn = lib.dk_pwconv_bwd_bnbwd_bf16 if bf else lib.dk_pwconv_bwd_bnbwd_f32
            rows = (lib.dk_pwconv_bwd_fused_bf16_rows if bf else lib.dk_pwconv_bwd_fused_rows)(N, OH, OW, K, C)
            nb = (lib.dk_pwconv_bwd_fused_bf16_workspace_bytes if bf else lib.dk_pwconv_bwd_fused_workspace_bytes)(
                N, OH, OW, K, C)
            assert (rows > 0) == (cid in FUSED[route, dt]), (cid, route, nm(dt), rows)
            assert nb == rows * K * C * 4

            def call(relu, bn_in, with_part, res):
                dx, dw = Guarded((N, OH, OW, C), dt), Guarded((K, C), F32)
                part = nan_rows(max(rows, 1), C) if with_part else None
                args = (p_(d, "g", dt), p_(d, "x1", dt), N, OH, OW, K, *po_ptrs(d, relu), d["k12_d"].data_ptr(),
                        d["w_d"].data_ptr(), C, L2, dw.ptr, dx.ptr, p_(d, "res", dt) if res else 0, p_(d, "x", dt),
                        *(pi_ptrs(d, 1) if bn_in else ZERO5), part.data_ptr() if with_part else 0, workspace.get(nb), nb,
                        stream_handle())
                return dx, dw, part, args

            if rows <= 0:
                refused(fn, *call(1, True, True, False)[3])
                continue
            if route == "default" and K in (128, 256):
                # the deep kernel takes an input BatchNorm only with its partials
                refused(fn, *call(1, True, False, False)[3])
            for relu in (0, 1):
                for bn_in in (False, True):
                    for res in (False, True):
                        dx, dw, part, args = call(relu, bn_in, bn_in, res)
                        assert fn(*args) == 0
                        r = bnbwd_dx_ref(cid, relu, res, bf)
                        got = nchw(dx.result())
                        name = "fused {} c{} {}".format(nm(dt), cid, route)
                        stored_check(name + " dx", got, r, dt)
                        rw = fused_dw_ref(cid, relu, 1 if bn_in else None, bf)
                        P.check(name + " dw", dw.result(), rw.ref, rw.A)
                        if bn_in:
                            P.part_checks(name + " part", host(part), got, d["x"], (*d["pi"], 1), r.ref, r.bound(bf))


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("cid", [c for c in CIDS if P.CASES[c][2] > 1])
def test_fused_lattice_backward(cid, route):
    """dk_pwconv_bwd_bnbwd_lattice_f32: x read at the stride-s lattice of the H x W input with its BatchNorm on
    load, dx compact.  K = C = 64 on the streaming kernel only; refused otherwise."""
    d = inputs(cid)
    N, H, W, C, K, st, OH, OW = dims(d)
    with routing(route):
        rows = lib.dk_pwconv_bwd_fused_rows(N, OH, OW, K, C)
        nb = max(lib.dk_pwconv_bwd_fused_workspace_bytes(N, OH, OW, K, C), 256)
        for relu in (0, 1):
            for with_part in (False, True):
                dx, dw = Guarded((N, OH, OW, C), F32), Guarded((K, C), F32)
                part = nan_rows(max(rows, 1), C) if with_part else None
                args = (p_(d, "g", F32), p_(d, "x1", F32), N, OH, OW, K, *po_ptrs(d, relu), d["k12_d"].data_ptr(),
                        d["w_d"].data_ptr(), C, L2, dw.ptr, dx.ptr, p_(d, "x", F32), H, W, st, *pi_ptrs(d, 1),
                        part.data_ptr() if with_part else 0, workspace.get(nb), nb, stream_handle())
                if (K, C) != (64, 64) or route == "tiled":
                    refused(lib.dk_pwconv_bwd_bnbwd_lattice_f32, *args)
                    continue
                assert rows > 0
                assert lib.dk_pwconv_bwd_bnbwd_lattice_f32(*args) == 0
                r = bnbwd_dx_ref(cid, relu, False, False, True)
                got = nchw(dx.result())
                name = "fusedlat f32 c{} {}".format(cid, route)
                P.check(name + " dx", got, r.ref, r.A)
                rw = fused_dw_ref(cid, relu, 1, False)
                P.check(name + " dw", dw.result(), rw.ref, rw.A)
                if with_part:
                    P.part_checks(name + " part", host(part), got, P.sample(d["x"], st), (*d["pi"], 1), r.ref, r.A)
