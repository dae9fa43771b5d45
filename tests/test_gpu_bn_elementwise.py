"""Every output element of the stand-alone BatchNorm entry points (dorknet_amd/csrc/batchnorm.hip) -- statistics in
one and in two stages, the folds of partial rows at every level, apply, the backward reduce, stage 2 and apply, the
one-shot backward, fp32 and bf16 storage -- against the fp64 reference of the same operation (tests/_bn_ref.py), each
under the bound derived there from the kernel's arithmetic, none excluded.  These entry points are what the fused
producers' and consumers' bitwise tests are measured against (tests/test_gpu_bn_on_load.py, test_gpu_fold.py, ...).

The cases (_bn_ref.CASES) are the smallest that reach each edge of the row loop: several reduce / apply blocks with a
ragged last one, the four-rows-in-flight loop and its remainder, idle threads, several channel slices with idle
groups, fewer rows than lanes, the scalar route (C % 4 != 0, and C % 4 == 0 behind pointers offset by one element).
Channels 0, 1, 2 of x are constant, all zero and of mean 2^8 times the spread.

Outputs are guarded (tests/_guard.py): slices of NaN-bit-filled buffers whose margins must stay intact and in which no
element may remain NaN; partial rows, fold workspaces and [C] vectors likewise (fp64 rows: one spare row that must stay
NaN); mask bytes sit in a 0xAB-filled buffer and must be exactly the reference decision, 0 or 1.

Refusals asserted (status and nothing written): every bf16 entry at C % 4 != 0 (cases 9-12) and behind a pointer
that is not 8-byte aligned (10001); every entry with a workspace one byte short of its query (10002);
dk_bn_apply_bf16 with a mask that is not 4-byte aligned (10001).

Worst err / bound per entry point and storage type on an MI355X (recorded with DORKNET_SLACK_LOG; results, not
tolerances; the number of checks in brackets; bf16 stores attain the interval form's end by construction -- 1.000 is
at the bound, never past it -- the closed form's figure after the slash):

    entry point                            fp32                                          bf16
    dk_bn_stats_partial_f64 + collapse     sums 0.000 (26)
    dk_bn_stats_*            mean          0.964 (39)                                    0.964 (24)
                             std           0.821 (39)                                    0.821 (24)
                             invstd        0.693 (39)                                    0.693 (24)
                             run_mean      0.964 (26)                                    0.964 (16)
                             run_std       0.849 (26)                                    0.849 (16)
    dk_bn_stats_finalize_f32               mean 0.734, std 0.379, invstd 0.355, run_mean 0.734, run_std 0.578 (12, 8)
    dk_bn_bwd_finalize_f32                 dgamma 0.782, dbeta 0.919, k12 0.929 (8 each)
    dk_bn_stats_from_partials_f32          mean 0.957, std 0.676, invstd 0.565, run_mean 0.957, run_std 0.771 (88 each)
    dk_bn_bwd_from_partials_f32            dgamma 0.982, dbeta 0.974, k12 0.976 (44 each)
    dk_bn_reduce_partials_f64              0.014 (22)
    dk_bn_apply_*            y             0.625 (54)                                    1.000 / 0.995 (32)
                             mask          equal (28)                                    equal (16)
    dk_bn_infer_params_f32                 0.950 (3)
    dk_bn_bwd_partial_f64                  0.794 (26)
    dk_relu_bwd_bn_partial_* dx            equal (8)                                     equal (6)
                             partials      0.756 (8)                                     0.756 (6)
    dk_bn_bwd_apply_*        dx            0.557 (130: five launch variants, identical)  1.000 / 0.995 (16)
    dk_bn_bwd_*              dgamma        0.674 (26)                                    0.674 (16)
                             dbeta         0.930 (26)                                    0.930 (16)
                             dx            0.506 (26)                                    1.000 / 0.996 (16)

A second look at the fp32 figures near 1: each is a single fp32 rounding -- (float) of an fp64 mean, sum or quotient,
or the one division of dk_bn_infer_params_f32 -- held to its half ulp u |v|, which a correctly rounded value attains
wherever |v| lies just above a power of two; with up to a thousand channels per vector a figure above 0.9 is expected, and
it is not a sign of a kernel at its limit: the numpy transcription of tests/test_bn_ref_host.py gives the same
0.964 / 0.821 / 0.693 on the same inputs.  The backward partials' 0.794 is case 4's single row: one product whose
x_hat carries its two fp32 roundings against XH = 2 u.  The statistics sums are exact (sums of bf16 values and of
their squares fit fp64 at these sizes); the synthetic rows of six decades show the fp64 folds at 0.014.

No kernel defect was found: every entry point met every bound on the first run.  Two host-side defects were fixed
beforehand, by reading.  bn_bwd_t (dk_bn_bwd_bf16) left a misaligned dx to its third stage to refuse, after the
first two had written dgamma and dbeta: it now refuses before it launches anything.  bn_apply_t chose the 4-element
route from x and y alone, although that route stores a group's four mask bytes as one 32-bit word; it now also
requires a 4-byte-aligned mask, as relu_bwd_bn_partial_t does (fp32 then takes the scalar route, bf16 refuses).
test_apply_mask_offset_by_one_byte holds that route to the same bounds; it was not run against the code before the
fix.
"""
import functools

import numpy as np
import pytest
import torch

from dorknet_amd._hip import HipError, lib, stream_handle
from tests import _bn_ref as B
from tests._guard import MARGIN, Guarded

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
F32 = torch.float32
CIDS = sorted(B.CASES)
EPS, MOM = float(B.BN_EPS), float(B.MOMENTUM)
MASK_FILL = 0xAB


def nm(dt):
    return "bf16" if dt == BF16 else "f32"


def dtypes(cid):
    return (F32, BF16) if cid in B.BF16_CASES else (F32,)


def off_of(cid):
    """Case 13: every pointer one element past an aligned address."""
    return 1 if cid == B.OFFSET_CASE else 0


class Out(Guarded):
    """A guarded output whose pointer lies `off` elements past the 16-byte-aligned slice."""

    def __init__(self, shape, dtype, off=0):
        super().__init__((int(np.prod(shape)) + off,), dtype)
        self.off, self.oshape = off, shape
        self.ptr += off * self.buf.element_size()

    def fill(self, values):
        self.buf[MARGIN + self.off:MARGIN + self.n] = torch.as_tensor(np.asarray(values, dtype=np.float32)).to(self.buf.dtype)
        return self

    def result(self):
        torch.cuda.synchronize()
        ints = self.buf.view(self.itype).cpu()
        assert bool((ints[:MARGIN + self.off] == self.bits).all()), "store before the output"
        assert bool((ints[MARGIN + self.n:] == self.bits).all()), "store past the output"
        out = self.buf[MARGIN + self.off:MARGIN + self.n].double().cpu().numpy().reshape(self.oshape)
        assert not np.isnan(out).any(), "{} elements never written".format(int(np.isnan(out).sum()))
        return out

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf.view(self.itype) == self.bits).all())


class MaskOut:
    """uint8 mask bytes inside a 0xAB-filled buffer; boff: byte offset of the pointer from a 16-byte-aligned address."""

    def __init__(self, shape, boff=0):
        self.shape, self.n, self.boff = shape, int(np.prod(shape)), boff
        self.buf = torch.full((self.n + 2 * MARGIN + boff,), MASK_FILL, dtype=torch.uint8, device="cuda")
        self.ptr = self.buf.data_ptr() + MARGIN + boff
        assert (self.ptr - boff) % 16 == 0

    def result(self):
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        lo = MARGIN + self.boff
        assert (b[:lo] == MASK_FILL).all() and (b[lo + self.n:] == MASK_FILL).all(), "mask store outside the mask"
        return b[lo:lo + self.n].reshape(self.shape)

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf == MASK_FILL).all())


class Rows:
    """fp64 rows [rows][2][C] pre-filled with NaN, with one spare row that must stay NaN."""

    def __init__(self, rows, C):
        self.rows, self.C = rows, C
        self.t = torch.full((rows + 1, 2, C), float("nan"), dtype=torch.float64, device="cuda")
        self.ptr, self.bytes = self.t.data_ptr(), rows * 2 * C * 8

    def result(self, rows=None):
        torch.cuda.synchronize()
        a = self.t.cpu().numpy()
        rows = self.rows if rows is None else rows
        assert np.isnan(a[rows:]).all(), "store past the rows"
        assert not np.isnan(a[:rows]).any(), "partial rows never written"
        return a[:rows]

    def untouched(self):
        torch.cuda.synchronize()
        return bool(torch.isnan(self.t).all())


class In:
    """A host array on the device as `dtype`, its pointer `off` elements past a 16-byte-aligned address."""

    def __init__(self, a, dtype, off=0):
        flat = torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float64).ravel()))
        self.buf = torch.zeros(flat.numel() + 8 + off, dtype=dtype, device="cuda")
        self.buf[off:off + flat.numel()] = flat.to(dtype).cuda()
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + off * self.buf.element_size()


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case(cid):
    d = B.make_inputs(cid)
    c = Case()
    c.d, c.P, c.C, c.off = d, d["P"], d["C"], off_of(cid)
    c.x = {dt: In(d["x"], dt, c.off) for dt in dtypes(cid)}
    c.g = {dt: In(d["g"], dt, c.off) for dt in dtypes(cid)}
    c.bn = [In(v, F32, c.off) for v in d["bn"]]
    c.bnp = tuple(v.ptr for v in c.bn)
    c.k12 = In(d["k12"], F32, c.off)
    c.mask8 = torch.as_tensor(d["mask8"]).cuda()
    return c


def any_case(cid):
    """Inputs for an entry that will refuse them: bf16 copies exist for every case."""
    c = case(cid)
    for dt in (F32, BF16):
        c.x.setdefault(dt, In(c.d["x"], dt, c.off))
        c.g.setdefault(dt, In(c.d["g"], dt, c.off))
    return c


def stored_check(name, got, r, dt):
    """A stored activation against its bound: fp32 the arithmetic's; bf16 the closed form of one rounding store and
    the interval form that implies it, each logged under its own name."""
    if dt == BF16:
        B.check(name + " closed", got, r.ref, r.b16c)
    B.check(name, got, r.ref, r.bound(dt == BF16))


def refused(code, fn, *args):
    with pytest.raises(HipError, match=str(code)):
        fn(*args)


def scratch(nbytes):
    """A workspace of exactly nbytes (in a larger NaN-filled allocation whose tail must stay NaN)."""
    words = B.cdiv(nbytes, 8)
    t = torch.full((words + 16,), float("nan"), dtype=torch.float64, device="cuda")
    return t, words


def scratch_ok(ws):
    t, words = ws
    torch.cuda.synchronize()
    return bool(torch.isnan(t[words:]).all())


@functools.lru_cache(maxsize=None)
def stats_ref(cid, first):
    c = case(cid)
    nblk = B.bn_blocks(c.P, c.C)
    sm = B.stats_sums(c.d["x"], nblk, B.fold_levels(nblk))
    return sm, B.stats_stage2(sm, float(c.P), first, c.d["run_mean0"], c.d["run_std0"])


@functools.lru_cache(maxsize=None)
def bwd_ref(cid, relu, masked=False):
    c = case(cid)
    nblk = B.bn_blocks(c.P, c.C)
    sb = B.bwd_sums(c.d["x"], c.d["g"], c.d["bn"], relu, nblk, B.fold_levels(nblk), c.d["mask8"] if masked else None)
    return sb, B.bwd_stage2(sb, float(c.P))


@functools.lru_cache(maxsize=None)
def apply_ref(cid, relu):
    c = case(cid)
    return B.apply_ref(c.d["x"], c.d["bn"], relu)


@functools.lru_cache(maxsize=None)
def dx_ref(cid, relu, oneshot=False):
    c = case(cid)
    if oneshot:
        r2 = bwd_ref(cid, relu)[1]
        return B.bwd_apply_ref(c.d["x"], c.d["g"], c.d["bn"], relu, r2.k12, r2.e_k12)
    return B.bwd_apply_ref(c.d["x"], c.d["g"], c.d["bn"], relu, c.d["k12"])


def stats_outputs(C, first, c=None):
    """mean, std, invstd, run_mean, run_std as guarded [C] vectors (the running ones prefilled for a blend)."""
    o = {k: Out((C,), F32) for k in B.STATS_FIELDS}
    if not first:
        o["run_mean"].fill(c.d["run_mean0"] if c is not None else RUN0[0][:C])
        o["run_std"].fill(c.d["run_std0"] if c is not None else RUN0[1][:C])
    return o


RUN0 = (np.random.RandomState(5).randn(1100).astype(np.float32),
        (np.random.RandomState(6).rand(1100) + 0.5).astype(np.float32))


def check_stats(name, o, r, running=True):
    for k in B.STATS_FIELDS if running else B.STATS_FIELDS[:3]:
        B.check("{} {}".format(name, k), o[k].result(), getattr(r, k), getattr(r, "e_" + k))


def optr(o):
    return tuple(o[k].ptr for k in B.STATS_FIELDS)


# ---------------------------------------------------------------------------------------------------------
# forward statistics
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", CIDS)
def test_stats_partial_and_collapse(cid):
    c = case(cid)
    P, C = c.P, c.C
    nblk = lib.dk_bn_partial_blocks(P, C)
    assert nblk == B.bn_blocks(P, C)
    assert lib.dk_bn_workspace_bytes(P, C) == nblk * 2 * C * 8
    part = Rows(nblk, C)
    assert lib.dk_bn_stats_partial_f64(c.x[F32].ptr, P, C, part.ptr, part.bytes, stream_handle()) == 0
    rows = part.result()
    sm = B.stats_sums(c.d["x"], nblk, 1)
    B.check("stats_partial f32 | c{} rows".format(cid), B._sum(rows), sm.ref, sm.bound)
    out = Rows(1, C)
    assert lib.dk_bn_collapse_f64(part.ptr, nblk, C, out.ptr, stream_handle()) == 0
    B.check("collapse f32 | c{} sums".format(cid), out.result()[0], sm.ref, sm.bound)


@pytest.mark.parametrize("cid", CIDS)
def test_stats(cid):
    c = case(cid)
    P, C = c.P, c.C
    nbytes = lib.dk_bn_stats_workspace_bytes(P, C)
    nblk = B.bn_blocks(P, C)
    assert nbytes == (nblk + B.fold_rows(nblk)) * 2 * C * 8
    for dt in dtypes(cid):
        fn = lib.dk_bn_stats_bf16 if dt == BF16 else lib.dk_bn_stats_f32
        for first in (1, 0):
            o = stats_outputs(C, first, c)
            ws = scratch(nbytes)
            assert fn(c.x[dt].ptr, P, C, EPS, MOM, first, *optr(o), ws[0].data_ptr(), nbytes, stream_handle()) == 0
            check_stats("stats {} | c{} first{}".format(nm(dt), cid, first), o, stats_ref(cid, first)[1])
            assert scratch_ok(ws)
        o = stats_outputs(C, 1)
        ws = scratch(nbytes)
        assert fn(c.x[dt].ptr, P, C, EPS, MOM, 0, *optr(o)[:3], 0, 0, ws[0].data_ptr(), nbytes, stream_handle()) == 0
        check_stats("stats {} | c{} no running".format(nm(dt), cid), o, stats_ref(cid, 1)[1], running=False)
        assert o["run_mean"].untouched() and o["run_std"].untouched() and scratch_ok(ws)


# ---------------------------------------------------------------------------------------------------------
# stage 2 on synthetic rows: the block_sum2 entry points and the fold levels
# ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def synth(nblk, C, seed=0):
    part = B.synth_rows(nblk, C, seed)
    return part, torch.as_tensor(part).cuda()


def check_bwd2(name, dgamma, dbeta, k12, r2):
    B.check(name + " dgamma", dgamma.result(), r2.dgamma, r2.e_dgamma)
    B.check(name + " dbeta", dbeta.result(), r2.dbeta, r2.e_dbeta)
    B.check(name + " k12", k12.result(), r2.k12, r2.e_k12)


@pytest.mark.parametrize("nblk", [1, 255, 257, 1024])
def test_finalize_direct(nblk):
    C = 6
    part, part_d = synth(nblk, C)
    sm = B.synth_sums(part, 1)
    count = 7.0 * nblk
    for first in (1, 0):
        o = stats_outputs(C, first)
        assert lib.dk_bn_stats_finalize_f32(part_d.data_ptr(), nblk, C, count, EPS, MOM, first, *optr(o),
                                            stream_handle()) == 0
        check_stats("stats_finalize f32 | n{} first{}".format(nblk, first), o,
                    B.stats_stage2(sm, count, first, RUN0[0][:C], RUN0[1][:C]))
    o = stats_outputs(C, 1)
    assert lib.dk_bn_stats_finalize_f32(part_d.data_ptr(), nblk, C, count, EPS, MOM, 0, *optr(o)[:3], 0, 0,
                                        stream_handle()) == 0
    check_stats("stats_finalize f32 | n{} no running".format(nblk), o, B.stats_stage2(sm, count, 1), running=False)
    # backward: one buffer, then distinct local and global buffers of different lengths
    nblk_g = nblk + 3
    glob, glob_d = synth(nblk_g, C, seed=1)
    smg = B.synth_sums(glob, 1)
    for name, gd, ng, r2 in (("same", part_d, nblk, B.bwd_stage2(sm, count)),
                             ("local/global", glob_d, nblk_g, B.bwd_stage2(sm, count, smg))):
        dgamma, dbeta, k12 = Out((C,), F32), Out((C,), F32), Out((2 * C,), F32)
        assert lib.dk_bn_bwd_finalize_f32(part_d.data_ptr(), nblk, gd.data_ptr(), ng, C, count, dgamma.ptr, dbeta.ptr,
                                          k12.ptr, stream_handle()) == 0
        check_bwd2("bwd_finalize f32 | n{} {}".format(nblk, name), dgamma, dbeta, k12, r2)


FOLDS = [(C, n) for C in (4, 64, 65, 130) for n in (1, 255, 256, 257, 513)] + [(4, 65536), (4, 65537)]


@pytest.mark.parametrize("ticketed", [False, True], ids=["levels", "tickets"])
@pytest.mark.parametrize("C,nblk", FOLDS)
def test_from_partials(C, nblk, ticketed):
    part, part_d = synth(nblk, C)
    sm = B.synth_sums(part, B.fold_levels(nblk))
    count = 7.0 * nblk
    nbytes = lib.dk_bn_partials_workspace_bytes(nblk, C)
    assert nbytes == B.fold_rows(nblk) * 2 * C * 8
    nt = lib.dk_bn_fold_tickets_count(C)
    assert nt == B.cdiv(C, 64)
    tickets = torch.zeros(nt + 1, dtype=torch.int32, device="cuda")
    tp = tickets.data_ptr() if ticketed else 0
    tag = "n{} C{} {}".format(nblk, C, "tickets" if ticketed else "levels")
    for first in (1, 0):
        o = stats_outputs(C, first)
        ws = scratch(nbytes)
        assert lib.dk_bn_stats_from_partials_f32(part_d.data_ptr(), nblk, C, count, EPS, MOM, first, *optr(o),
                                                 ws[0].data_ptr(), nbytes, tp, stream_handle()) == 0
        check_stats("stats_from_partials f32 | {} first{}".format(tag, first), o,
                    B.stats_stage2(sm, count, first, RUN0[0][:C], RUN0[1][:C]))
        assert scratch_ok(ws)
    dgamma, dbeta, k12 = Out((C,), F32), Out((C,), F32), Out((2 * C,), F32)
    ws = scratch(nbytes)
    assert lib.dk_bn_bwd_from_partials_f32(part_d.data_ptr(), nblk, C, count, dgamma.ptr, dbeta.ptr, k12.ptr,
                                           ws[0].data_ptr(), nbytes, tp, stream_handle()) == 0
    check_bwd2("bwd_from_partials f32 | " + tag, dgamma, dbeta, k12, B.bwd_stage2(sm, count))
    assert scratch_ok(ws)
    assert int(tickets.cpu().abs().sum()) == 0, "tickets not put back to zero"
    if not ticketed:
        out = Rows(1, C)
        ws = scratch(nbytes)
        assert lib.dk_bn_reduce_partials_f64(part_d.data_ptr(), nblk, C, out.ptr, ws[0].data_ptr(), nbytes,
                                             stream_handle()) == 0
        B.check("reduce_partials f64 | " + tag, out.result()[0], sm.ref, sm.bound)
        assert scratch_ok(ws)


# ---------------------------------------------------------------------------------------------------------
# apply
# ---------------------------------------------------------------------------------------------------------

def run_apply(c, cid, dt, relu, with_mask, mask_boff, name):
    P, C = c.P, c.C
    fn = lib.dk_bn_apply_bf16 if dt == BF16 else lib.dk_bn_apply_f32
    y = Out((P, C), dt, c.off)
    mask = MaskOut((P, C), mask_boff) if with_mask else None
    assert fn(c.x[dt].ptr, P * C, C, *c.bnp, relu, y.ptr, mask.ptr if mask else 0, stream_handle()) == 0
    r = apply_ref(cid, relu)
    stored_check(name + " y", y.result(), r, dt)
    if mask:
        B.check(name + " mask", mask.result(), r.mask.astype(np.float64), np.zeros(r.mask.shape))


@pytest.mark.parametrize("cid", CIDS)
def test_apply(cid):
    c = case(cid)
    for dt in dtypes(cid):
        for relu in (0, 1):
            for with_mask in (False, True):
                run_apply(c, cid, dt, relu, with_mask, c.off,
                          "apply {} | c{} relu{}{}".format(nm(dt), cid, relu, " mask" if with_mask else ""))


def test_apply_mask_offset_by_one_byte():
    """x and y aligned, the mask one byte past an aligned address: fp32 takes the scalar route (the float4 route
    stores four mask bytes as one 32-bit word), bf16 refuses."""
    cid = 3
    c = case(cid)
    for relu in (0, 1):
        run_apply(c, cid, F32, relu, True, 1, "apply f32 | c{} relu{} mask + 1 byte".format(cid, relu))
    y, mask = Out((c.P, c.C), BF16), MaskOut((c.P, c.C), 1)
    refused(10001, lib.dk_bn_apply_bf16, c.x[BF16].ptr, c.P * c.C, c.C, *c.bnp, 1, y.ptr, mask.ptr, stream_handle())
    assert y.untouched() and mask.untouched()


@pytest.mark.parametrize("C", [1, 256, 257])
def test_infer_params(C):
    rs = RUN0[1][:C]
    out = Out((C,), F32)
    src = In(rs, F32)
    assert lib.dk_bn_infer_params_f32(src.ptr, C, out.ptr, stream_handle()) == 0
    ref = 1.0 / rs.astype(np.float64)
    B.check("infer_params f32 | C{}".format(C), out.result(), ref, B.U * ref)      # one correctly rounded division


# ---------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", CIDS)
def test_bwd_partial(cid):
    c = case(cid)
    P, C = c.P, c.C
    nblk = lib.dk_bn_partial_blocks(P, C)
    for relu in (0, 1):
        part = Rows(nblk, C)
        assert lib.dk_bn_bwd_partial_f64(c.x[F32].ptr, c.g[F32].ptr, P, C, *c.bnp, relu, part.ptr, part.bytes,
                                         stream_handle()) == 0
        sb = bwd_ref(cid, relu)[0]
        B.check("bwd_partial f32 | c{} relu{}".format(cid, relu), B._sum(part.result()), sb.ref, sb.bound)


@pytest.mark.parametrize("cid", [2, 6, 8, 9])
def test_relu_bwd_bn_partial(cid):
    c = case(cid)
    P, C = c.P, c.C
    nblk = lib.dk_bn_partial_blocks(P, C)
    want_dx = np.where(c.d["mask8"] != 0, c.d["g"], 0.0)
    for dt in dtypes(cid):
        fn = lib.dk_relu_bwd_bn_partial_bf16 if dt == BF16 else lib.dk_relu_bwd_bn_partial_f64
        for relu in (0, 1):
            dx, part = Out((P, C), dt), Rows(nblk, C)
            assert fn(c.g[dt].ptr, c.mask8.data_ptr(), c.x[dt].ptr, P, C, *c.bnp, relu, dx.ptr, part.ptr, part.bytes,
                      stream_handle()) == 0
            name = "relu_bwd_bn_partial {} | c{} relu{}".format(nm(dt), cid, relu)
            B.check(name + " dx", dx.result(), want_dx, np.zeros(want_dx.shape))       # bit for bit
            sb = bwd_ref(cid, relu, True)[0]
            B.check(name + " part", B._sum(part.result()), sb.ref, sb.bound)


@pytest.mark.parametrize("cid", CIDS)
def test_bwd_apply(cid):
    c = case(cid)
    P, C = c.P, c.C
    for dt in dtypes(cid):
        fn = lib.dk_bn_bwd_apply_bf16 if dt == BF16 else lib.dk_bn_bwd_apply_f32
        for relu in (0, 1):
            got = {}
            try:
                # -1 the built-in launch; 4-7: 8 rows per lane (several blocks), 4 / 8 rows in flight, plain /
                # nontemporal stores
                for var in ((-1, 4, 5, 6, 7) if dt == F32 else (-1,)):
                    lib.dk_debug_set_ew_variant(var)
                    dx = Out((P, C), dt, c.off)
                    assert fn(c.x[dt].ptr, c.g[dt].ptr, P * C, C, *c.bnp, relu, c.k12.ptr, dx.ptr, stream_handle()) == 0
                    got[var] = dx.result()
            finally:
                lib.dk_debug_set_ew_variant(-1)
            r = dx_ref(cid, relu)
            for var, v in got.items():
                stored_check("bwd_apply {} | c{} relu{} variant {}".format(nm(dt), cid, relu, var), v, r, dt)
                assert np.array_equal(v, got[-1]), "launch variant {} differs from the built-in one".format(var)


@pytest.mark.parametrize("cid", CIDS)
def test_bwd_oneshot(cid):
    c = case(cid)
    P, C = c.P, c.C
    nbytes = lib.dk_bn_bwd_workspace_bytes(P, C)
    nblk = B.bn_blocks(P, C)
    assert nbytes == (nblk + B.fold_rows(nblk)) * 2 * C * 8 + 2 * C * 4
    for dt in dtypes(cid):
        fn = lib.dk_bn_bwd_bf16 if dt == BF16 else lib.dk_bn_bwd_f32
        for relu in (0, 1):
            dgamma, dbeta, dx = Out((C,), F32), Out((C,), F32), Out((P, C), dt, c.off)
            ws = scratch(nbytes)
            assert fn(c.x[dt].ptr, c.g[dt].ptr, P, C, *c.bnp, relu, dgamma.ptr, dbeta.ptr, dx.ptr, ws[0].data_ptr(),
                      nbytes, stream_handle()) == 0
            r2 = bwd_ref(cid, relu)[1]
            name = "bwd {} | c{} relu{}".format(nm(dt), cid, relu)
            B.check(name + " dgamma", dgamma.result(), r2.dgamma, r2.e_dgamma)
            B.check(name + " dbeta", dbeta.result(), r2.dbeta, r2.e_dbeta)
            stored_check(name + " dx", dx.result(), dx_ref(cid, relu, True), dt)
            assert scratch_ok(ws)


# ---------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------

def bf16_calls(c, mis=None):
    """(entry, arguments, outputs) of every bf16 entry on case c.  mis: the pointer put two bytes past an aligned
    address -- "x", "g" (the gradient) or "out" (the bf16 output); entries without that pointer are left out."""
    P, C = c.P, c.C
    keep = [In(c.d["x"], BF16, 1), In(c.d["g"], BF16, 1)]
    x = keep[0].ptr if mis == "x" else c.x[BF16].ptr
    g = keep[1].ptr if mis == "g" else c.g[BF16].ptr
    ooff = 1 if mis == "out" else 0
    st = stream_handle()
    calls = []
    if mis in (None, "x"):
        o = stats_outputs(C, 1)
        nb = lib.dk_bn_stats_workspace_bytes(P, C)
        ws = scratch(nb)
        keep.append(ws)
        calls.append((lib.dk_bn_stats_bf16, (x, P, C, EPS, MOM, 1, *optr(o), ws[0].data_ptr(), nb, st), list(o.values())))
    if mis != "g":
        y, mask = Out((P, C), BF16, ooff), MaskOut((P, C))
        calls.append((lib.dk_bn_apply_bf16, (x, P * C, C, *c.bnp, 1, y.ptr, mask.ptr, st), [y, mask]))
    dx = Out((P, C), BF16, ooff)
    calls.append((lib.dk_bn_bwd_apply_bf16, (x, g, P * C, C, *c.bnp, 1, c.k12.ptr, dx.ptr, st), [dx]))
    dgamma, dbeta, dx2 = Out((C,), F32), Out((C,), F32), Out((P, C), BF16, ooff)
    nb2 = lib.dk_bn_bwd_workspace_bytes(P, C)
    ws2 = scratch(nb2)
    keep.append(ws2)
    calls.append((lib.dk_bn_bwd_bf16, (x, g, P, C, *c.bnp, 1, dgamma.ptr, dbeta.ptr, dx2.ptr, ws2[0].data_ptr(), nb2, st),
                  [dgamma, dbeta, dx2]))
    dx3, part = Out((P, C), BF16, ooff), Rows(lib.dk_bn_partial_blocks(P, C), C)
    calls.append((lib.dk_relu_bwd_bn_partial_bf16, (g, c.mask8.data_ptr(), x, P, C, *c.bnp, 1, dx3.ptr, part.ptr,
                                                    part.bytes, st), [dx3, part]))
    return calls, keep


@pytest.mark.parametrize("cid", B.SCALAR_CASES)
def test_bf16_refuses_channels_not_a_multiple_of_four(cid):
    calls, keep = bf16_calls(any_case(cid))
    assert len(calls) == 5
    for fn, args, outs in calls:
        refused(10001, fn, *args)
        assert all(o.untouched() for o in outs), fn.__name__


@pytest.mark.parametrize("mis", ["x", "g", "out"])
def test_bf16_refuses_misaligned_pointer(mis):
    calls, keep = bf16_calls(case(3), mis)
    assert len(calls) == {"x": 5, "g": 3, "out": 4}[mis]
    for fn, args, outs in calls:
        refused(10001, fn, *args)
        assert all(o.untouched() for o in outs), (fn.__name__, mis)


def test_short_workspace_refused():
    """Every entry that takes a workspace, one byte short of its query: 10002 and nothing written."""
    cid = 2
    c = case(cid)
    P, C = c.P, c.C
    st = stream_handle()
    nblk = lib.dk_bn_partial_blocks(P, C)
    part = Rows(nblk, C)
    refused(10002, lib.dk_bn_stats_partial_f64, c.x[F32].ptr, P, C, part.ptr, part.bytes - 1, st)
    refused(10002, lib.dk_bn_bwd_partial_f64, c.x[F32].ptr, c.g[F32].ptr, P, C, *c.bnp, 1, part.ptr, part.bytes - 1, st)
    assert part.untouched()
    for dt in (F32, BF16):
        o = stats_outputs(C, 1)
        nb = lib.dk_bn_stats_workspace_bytes(P, C)
        ws = scratch(nb)
        refused(10002, lib.dk_bn_stats_bf16 if dt == BF16 else lib.dk_bn_stats_f32, c.x[dt].ptr, P, C, EPS, MOM, 1,
                *optr(o), ws[0].data_ptr(), nb - 1, st)
        assert all(v.untouched() for v in o.values()) and bool(torch.isnan(ws[0]).all())
        dgamma, dbeta, dx = Out((C,), F32), Out((C,), F32), Out((P, C), dt)
        nb = lib.dk_bn_bwd_workspace_bytes(P, C)
        ws = scratch(nb)
        refused(10002, lib.dk_bn_bwd_bf16 if dt == BF16 else lib.dk_bn_bwd_f32, c.x[dt].ptr, c.g[dt].ptr, P, C, *c.bnp,
                1, dgamma.ptr, dbeta.ptr, dx.ptr, ws[0].data_ptr(), nb - 1, st)
        assert dgamma.untouched() and dbeta.untouched() and dx.untouched() and bool(torch.isnan(ws[0]).all())
        dx, part = Out((P, C), dt), Rows(nblk, C)
        refused(10002, lib.dk_relu_bwd_bn_partial_bf16 if dt == BF16 else lib.dk_relu_bwd_bn_partial_f64, c.g[dt].ptr,
                c.mask8.data_ptr(), c.x[dt].ptr, P, C, *c.bnp, 1, dx.ptr, part.ptr, part.bytes - 1, st)
        assert dx.untouched() and part.untouched()
    for nrows in (1, 513):      # the query is one row at least
        Cs = 65
        _, part_d = synth(nrows, Cs)
        nb = lib.dk_bn_partials_workspace_bytes(nrows, Cs)
        ws = scratch(nb)
        o = stats_outputs(Cs, 1)
        refused(10002, lib.dk_bn_stats_from_partials_f32, part_d.data_ptr(), nrows, Cs, 7.0 * nrows, EPS, MOM, 1,
                *optr(o), ws[0].data_ptr(), nb - 1, 0, st)
        dgamma, dbeta, k12 = Out((Cs,), F32), Out((Cs,), F32), Out((2 * Cs,), F32)
        refused(10002, lib.dk_bn_bwd_from_partials_f32, part_d.data_ptr(), nrows, Cs, 7.0 * nrows, dgamma.ptr,
                dbeta.ptr, k12.ptr, ws[0].data_ptr(), nb - 1, 0, st)
        out = Rows(1, Cs)
        refused(10002, lib.dk_bn_reduce_partials_f64, part_d.data_ptr(), nrows, Cs, out.ptr, ws[0].data_ptr(), nb - 1, st)
        assert all(v.untouched() for v in o.values()) and dgamma.untouched() and dbeta.untouched()
        assert k12.untouched() and out.untouched() and bool(torch.isnan(ws[0]).all())
