"""Every output element of the unfused depthwise entry points -- forward, input gradient, weight gradient,
fp32 and bf16 storage -- and of the fused stride-1 backward against the fp64 reference of the same operation
(tests/_dw_ref.py), each under the bound derived there from the arithmetic, none excluded.  The geometries
(_dw_ref.GEOMS) are the smallest that reach each tile, segment and padding edge of depthwise.hip: two and
three fp32 row segments, ragged 4-wide column chunks, stride-1 padding 0 and R - 1 (the stride-1 dgrad is
the forward kernel at padding R - 1 - pad, so padding 2 / 4 "full" correlation), one pixel, C = 1028 (the
weight gradient's second channel block), odd and even strided shapes for the sub-pixel dgrads, the gather
dgrad, 5x5 and 1x1.  The other depthwise kernels (fused stride-2 backward, join forms, two columns per
thread) are tied bitwise to these entry points by their own tests.

Every call also runs with its output as a 16-byte-aligned slice of a larger allocation pre-filled with a
NaN bit pattern: the 64-element margins before and after must be bitwise untouched (a 16-byte store past a
ragged row) and no output element may remain NaN (an element never written).

Refusals asserted (status 10001, nothing else): a residual addend on the gather dgrad (geometry 9), bf16
storage on the gather dgrad.

Worst err / bound per family on an MI355X (recorded with DORKNET_SLACK_LOG; results, not tolerances):

    family                      checks   worst err / bound
    forward  fp32                  162     0.28   (geometry 14, 1x1)
    forward  bf16                  162     0.995 closed form (geometry 4);  1.000 interval form
    dgrad    fp32                   44     0.35   (geometry 14)
    dgrad    bf16                   28     0.995 closed form (geometry 4);  1.000 interval form
    wgrad    fp32                   60     0.37   (geometry 5, one pixel)
    wgrad    bf16                   60     0.37   (geometry 5)
    fused backward fp32  dx / dw    24     0.23 / 0.007
    fused backward bf16  dx / dw    24     0.995 closed form, 1.000 interval form / 0.007

bf16 stores are held to two bounds (_dw_ref.bf16_bound): the closed form 2^-8 (|ref| + A) + A, and the
interval rne(ref - A) .. rne(ref + A) that implies it.  A correct store attains the interval's end exactly
wherever the reference rounds the long way, so its recorded ratio is 1.000 by construction -- at the bound,
never past it -- while anything further (a truncating store) is a whole ulp outside.
"""
import functools

import numpy as np
import pytest
import torch

from dorknet_amd._hip import HipError, lib, stream_handle, workspace
from tests import _dw_ref as D
from tests._guard import Guarded

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
F32 = torch.float32
L2 = float(np.float32(1e-3))
GIDS = sorted(D.GEOMS)


def nchw(a):
    return a.transpose(0, 3, 1, 2)


def dev(a, dtype=F32):
    """An NCHW host array on the device as NHWC of the storage type (the values are bf16-representable)."""
    t = torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float32).transpose(0, 2, 3, 1)))
    return t.to(dtype).cuda()


def vec(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()


@functools.lru_cache(maxsize=None)
def inputs(gid):
    d = D.make_inputs(gid)
    d["dev"] = {(k, dt): dev(d[k], dt) for k in ("x", "dy", "res") for dt in (F32, BF16)}
    d["w_d"], d["bias_d"] = vec(d["w"]), vec(d["bias"])
    d["bn_d"] = [vec(v) for v in d["bn"]]
    return d


@functools.lru_cache(maxsize=None)
def fwd_ref(gid, bias, bn):
    d = inputs(gid)
    return D.reference(d["x"], d["w"], d["stride"], d["pad"], d["bias"] if bias else None,
                       None if bn is None else (*d["bn"], bn))


@functools.lru_cache(maxsize=None)
def bwd_ref(gid, res, l2, bn):
    d = inputs(gid)
    return D.reference(d["x"], d["w"], d["stride"], d["pad"], None, None if bn is None else (*d["bn"], bn),
                       d["dy"], d["res"] if res else None, l2)


def bn_ptrs(d, bn):
    return (0, 0, 0, 0, 0) if bn is None else (*(t.data_ptr() for t in d["bn_d"]), bn)


def name_of(dt):
    return "bf16" if dt == BF16 else "f32"


def check_stored(name, got, ref, dt, b32, b16, b16c):
    """A stored activation against its bound: fp32 the arithmetic's; bf16 the closed form of one rounding
    store and the interval form that implies it (_dw_ref.bf16_bound), each logged under its own name."""
    if dt == BF16:
        D.check(name + " closed", got, ref, b16c)
        D.check(name, got, ref, b16)
    else:
        D.check(name, got, ref, b32)


@pytest.mark.parametrize("bn", [None, 0, 1], ids=["plain", "bn", "bnrelu"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("gid", GIDS)
def test_forward(gid, bias, bn):
    d, r = inputs(gid), fwd_ref(gid, bias, bn)
    N, H, W, C, R, st, pad, OH, OW = (d[k] for k in ("N", "H", "W", "C", "R", "stride", "pad", "OH", "OW"))
    for dt in (F32, BF16):
        fn = lib.dk_dwconv_fwd_ex_bf16 if dt == BF16 else lib.dk_dwconv_fwd_ex_f32
        rows = (lib.dk_dwconv_fwd_bf16_stats_rows if dt == BF16 else lib.dk_dwconv_fwd_stats_rows)(N, OH, OW, C, st)
        for stats in (False, True):
            if stats and rows <= 0:
                continue
            part = torch.zeros((rows, 2, C), dtype=torch.float64, device="cuda") if stats else None
            y = Guarded((N, OH, OW, C), dt)
            rc = fn(d["dev"]["x", dt].data_ptr(), N, H, W, C, d["w_d"].data_ptr(), R, R, st, pad,
                    d["bias_d"].data_ptr() if bias else 0, y.ptr, OH, OW, *bn_ptrs(d, bn),
                    part.data_ptr() if stats else 0, stream_handle())
            assert rc in (0, 10100), rc
            check_stored("fwd {} g{}{}".format(name_of(dt), gid, " stats" if stats else ""), nchw(y.result()), r.y,
                         dt, r.by, r.by16, r.by16c)


def test_statistics_rows_where_a_block_covers_every_channel():
    """Statistics rows exist where C / 4 divides 256: not for geometries 6 (C / 4 = 257), 9 (6) and 10 (3)."""
    for gid in GIDS:
        d = inputs(gid)
        for q in (lib.dk_dwconv_fwd_stats_rows, lib.dk_dwconv_fwd_bf16_stats_rows):
            assert (q(d["N"], d["OH"], d["OW"], d["C"], d["stride"]) > 0) == (gid not in (6, 9, 10)), gid


def gather_path(d):
    """The geometries without a stride-1 or sub-pixel dgrad (depthwise.hip, dw_dgrad)."""
    return d["stride"] != 1 and (d["R"], d["pad"]) not in ((3, 1), (5, 2), (1, 0))


@pytest.mark.parametrize("res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("gid", GIDS)
def test_dgrad(gid, res):
    d, r = inputs(gid), bwd_ref(gid, res, 0.0, None)
    N, H, W, C, R, st, pad, OH, OW = (d[k] for k in ("N", "H", "W", "C", "R", "stride", "pad", "OH", "OW"))
    nb = lib.dk_dwconv_dgrad_workspace_bytes(C, R, R)
    for dt in (F32, BF16):
        fn = lib.dk_dwconv_dgrad_ex_bf16 if dt == BF16 else lib.dk_dwconv_dgrad_ex_f32
        dx = Guarded((N, H, W, C), dt)
        args = (d["dev"]["dy", dt].data_ptr(), N, OH, OW, C, d["w_d"].data_ptr(), R, R, st, pad, dx.ptr, H, W,
                workspace.get(nb), nb, d["dev"]["res", dt].data_ptr() if res else 0, 0, 0, 0, 0, 0, 0, 0,
                stream_handle())
        if gather_path(d) and (res or dt == BF16):
            # refused by design: no residual and no bf16 storage on the generic gather dgrad
            with pytest.raises(HipError, match="10001"):
                fn(*args)
            continue
        assert fn(*args) in (0, 10100)
        check_stored("dgrad {} g{}".format(name_of(dt), gid), nchw(dx.result()), r.dx, dt, r.bx, r.bx16, r.bx16c)
    if not res:
        # the entry point without the optional operands
        dx = Guarded((N, H, W, C), F32)
        assert lib.dk_dwconv_dgrad_f32(d["dev"]["dy", F32].data_ptr(), N, OH, OW, C, d["w_d"].data_ptr(), R, R, st,
                                       pad, dx.ptr, H, W, workspace.get(nb), nb, stream_handle()) == 0
        D.check("dgrad f32 g{} plain".format(gid), nchw(dx.result()), r.dx, r.bx)


def test_only_geometry_9_takes_the_gather_dgrad():
    assert [gid for gid in GIDS if gather_path(inputs(gid))] == [9]


@pytest.mark.parametrize("bn", [None, 1], ids=["plain", "bnrelu"])
@pytest.mark.parametrize("l2", [0.0, L2], ids=["nol2", "l2"])
@pytest.mark.parametrize("gid", GIDS)
def test_wgrad(gid, l2, bn):
    d, r = inputs(gid), bwd_ref(gid, False, l2, bn)
    N, H, W, C, R, st, pad, OH, OW = (d[k] for k in ("N", "H", "W", "C", "R", "stride", "pad", "OH", "OW"))
    nb = lib.dk_dwconv_wgrad_workspace_bytes(N, OH, OW, C, R, R)
    for dt in (F32, BF16):
        dw = Guarded((C, R, R), F32)
        args = (d["dev"]["dy", dt].data_ptr(), d["dev"]["x", dt].data_ptr(), N, H, W, C, R, R, st, pad, OH, OW,
                d["w_d"].data_ptr(), l2, dw.ptr, workspace.get(nb), nb)
        if dt == BF16:
            rc = lib.dk_dwconv_wgrad_bnx_bf16(*args, *bn_ptrs(d, bn), stream_handle())
        elif bn is None:
            rc = lib.dk_dwconv_wgrad_f32(*args, stream_handle())
        else:
            rc = lib.dk_dwconv_wgrad_bnx_f32(*args, *bn_ptrs(d, bn), stream_handle())
        assert rc == 0
        D.check("wgrad {} g{}".format(name_of(dt), gid), dw.result(), r.dw, r.bw)


# ---------------------------------------------------------------------------------------------------------
# The fused stride-1 backward (dk_dwconv_bwd_bnbwd_f32 / _bf16): dy = the following BatchNorm's backward
# apply, formed in fp32 and never stored, so the bf16 entry is not bit-comparable with the unfused bf16
# sequence.  dx (storage type) and dw (fp32) per element against fp64, dy's fp32 error scale ed entering the
# bounds as |w| (*) ed and sum |xb| ed (tests/_dw_ref.py).
# ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def fused_inputs(fid, relu):
    d = D.make_fused_inputs(fid, relu)
    d["dev"] = {(k, dt): dev(d[k], dt) for k in ("g", "x1", "x", "res") for dt in (F32, BF16)}
    d["w_d"], d["k12_d"] = vec(d["w"]), vec(d["k12"])
    d["po_d"] = [vec(v) for v in d["po"][:4]]
    d["pi_d"] = [vec(v) for v in d["pi"]]
    return d


@pytest.mark.parametrize("res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("bn_in", [False, True], ids=["plain", "bnrelu"])
@pytest.mark.parametrize("relu", [0, 1], ids=["norelu", "relu"])
@pytest.mark.parametrize("fid", sorted(D.FUSED))
def test_fused_stride1_backward(fid, relu, bn_in, res):
    d = fused_inputs(fid, relu)
    N, H, W, C = d["N"], d["H"], d["W"], d["C"]
    # precondition on the inputs (not a filter on the compared elements): the ReLU mask is decided alike in
    # fp32 and fp64 -- no element of bn(x1) within its own fp32 error of zero
    assert D.mask_margin(d["x1"], d["po"]) > 1.0
    dy, ed, _ = D.bn_bwd_dy(d["g"], d["x1"], d["po"], d["k12"])
    r = D.reference(d["x"], d["w"], 1, 1, None, (*d["pi"], 1) if bn_in else None, dy, d["res"] if res else None, L2,
                    dy_err=ed)
    for dt in (F32, BF16):
        bf = dt == BF16
        fn = lib.dk_dwconv_bwd_bnbwd_bf16 if bf else lib.dk_dwconv_bwd_bnbwd_f32
        nb = (lib.dk_dwconv_bwd_bnbwd_bf16_workspace_bytes if bf else lib.dk_dwconv_bwd_bnbwd_workspace_bytes)(
            N, H, W, C, 3, 3)
        dx, dw = Guarded((N, H, W, C), dt), Guarded((C, 3, 3), F32)
        bn = (*(t.data_ptr() for t in d["pi_d"]), 1) if bn_in else (0, 0, 0, 0, 0)
        rc = fn(d["dev"]["g", dt].data_ptr(), d["dev"]["x1", dt].data_ptr(), N, H, W, C,
                *(t.data_ptr() for t in d["po_d"]), relu, d["k12_d"].data_ptr(), d["dev"]["x", dt].data_ptr(),
                d["w_d"].data_ptr(), 3, 3, 1, L2, dw.ptr, dx.ptr, d["dev"]["res", dt].data_ptr() if res else 0, *bn, 0,
                workspace.get(nb), nb, stream_handle())
        assert rc in (0, 10100), rc
        check_stored("fused {} dx f{}".format(name_of(dt), fid), nchw(dx.result()), r.dx, dt, r.bx, r.bx16, r.bx16c)
        D.check("fused {} dw f{}".format(name_of(dt), fid), dw.result(), r.dw, r.bw)
