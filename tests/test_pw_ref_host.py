"""tests/_pw_ref.py on the CPU: the fp64 reference agrees with the oracle, its per-element bounds admit an honest
fp32 implementation (torch-CPU: bn_operand_f32, an fp32 matmul, fp32 sums for dw; for bf16 storage the operands
rounded as documented, the reduction in fp32 and the stores rounded to nearest even) on every case in three
summation orders (torch's, the reduction reversed, the reduction split in four and combined), and they reject
wrong kernels -- each a mutation of that implementation of a kind a pointwise kernel can have.

Worst err / bound of the honest implementation over the 21 cases (recorded with DORKNET_SLACK_LOG; results, not
tolerances; fp32 over the three summation orders / bf16; a bf16 store attains the interval form's end by
construction, so its 1.000 is "at the bound", the closed form's figure in brackets):

    y                         0.204 / 1.000 (0.994)       dx (widened, lattice)     0.099 / 1.000 (0.994)
    dw                        0.219 / 0.950               dw, dy formed on load     0.209 / 0.900
    dy_out                    0.624 / 1.000 (0.996)       dx, dy formed on load     0.131 / 1.000 (0.741)
    dx against stored dy_out  0.123 / 1.000 (0.991)
    statistics | stored       sum 0.000, squares 0.327 / 0.000, 0.015      | reference   0.051 / 1.000
    partials   | stored       g 0.000, g x_hat 0.755 / 0.000, 0.755        | reference   0.013 / 1.000

Mutants, worst err / bound and (normwise error of the mutated tensor):
     1 ragged tile's last pixel left at zero          5.5e4  (6.0e-2)
     2 last k-step dropped, fp32 (2 of 512 channels)  4.7e2  (6.5e-2);  bf16 (16 of 512)  2.3e6  (1.8e-1)
     3 32-column block of w shifted by one row        5.0e4  (7.1e-1)
     4 bias added to column k + 32                    1.0e5  (8.8e-1)
     5 on-load ReLU skipped for one of 512 channels   8.8e2  (5.0e-2)
     6 residual twice / omitted on the last tile      5.6e4  (2.3e-1) each
     7 bf16 store truncating                          2.0e4  (3.3e-3); 1.9 against the closed form alone
     8 l2 term dropped (M = 5)                        1.7e3  (5.5e-5)
     9 weight gradient misses the last ragged tile    1.7e3  (3.2e-1)
    10 dy without its k2 x_hat term                   3.1e4  (1.6e-1)
    11 statistics over the unrounded bf16 y           5.9e9 (sum), 1.2e10 (squares) of the stored-sums bound
    12 partials with the ReLU mask ignored            7.9e12 of the stored-sums bound
    13 stride 2 sampled at (2 oh + 1, 2 ow)           1.3e5  (1.4)
    truncated bf16 weight operand                     1.7e6 on a bf16 y of raw activations (4.4e-3);  1.95 behind a
                                                      BatchNorm on load;  invisible to every weight gradient
What a normwise 1e-4 lets through, asserted below: at these shapes only mutant 8 (and, under the 1e-2 the
suite holds bf16 tensors to, mutant 7 and the truncated weight operand).  The others are wrong in one pixel,
one k-step or one channel of a tensor this small -- a share 1 / sqrt(M) or sqrt(2 / C) of the norm -- and are
above 1e-4 here; the normwise layer tests miss them because their seven shapes reach neither the ragged
429-pixel tiles nor the statistics and partial sums at all (mutants 11 and 12 leave y and dx untouched), and
the kernel-against-kernel tests because the mutation is common to both sides.  Mutant 8 needs the smallest
case: at M = 429 the M-term bound on dw (0.014) is above 1e-3 |w|; at M = 5 it is not.
"""
import numpy as np
import pytest
import torch

from oracle import ref as oref
from tests import _pw_ref as P

f = np.float32
L2 = float(np.float32(1e-3))
CIDS = sorted(P.CASES)
ORDERS = ("torch", "rev", "split4")
MODES = [(False, o) for o in ORDERS] + [(True, "torch")]     # the other summation orders in fp32


# ---------------------------------------------------------------------------------------------------------
# the honest implementation
# ---------------------------------------------------------------------------------------------------------

def q16(a):
    """fp32 -> bf16 (nearest even) -> fp32."""
    return torch.tensor(np.ascontiguousarray(a, dtype=f)).to(torch.bfloat16).float().numpy()


def trunc16(a):
    return (np.ascontiguousarray(a, dtype=f).view(np.uint32) & np.uint32(0xFFFF0000)).view(f)


def mm(a, b, order="torch"):
    """a (M, R) @ b (R, N) in fp32, the reduction over R in the given order."""
    a, b = torch.tensor(np.ascontiguousarray(a, dtype=f)), torch.tensor(np.ascontiguousarray(b, dtype=f))
    if order == "torch":
        return (a @ b).numpy()
    if order == "rev":
        return (a.flip(1) @ b.flip(0)).numpy()
    R = a.shape[1]
    cut = [R * i // 4 for i in range(5)]
    p = [a[:, cut[i]:cut[i + 1]] @ b[cut[i]:cut[i + 1]] for i in range(4)]
    return ((p[0] + p[1]) + (p[2] + p[3])).numpy()


def h_weights(w, bf16):
    return q16(w) if bf16 else np.asarray(w, dtype=f)


def h_operand(x, bn, stride, bf16):
    """The sampled forward / weight-gradient operand as the MFMA sees it (fp32 array)."""
    a = P.sample(P.bn_operand_f32(x, bn), stride)
    return q16(a) if bf16 and bn is not None else a


def h_store(v, bf16):
    return q16(v) if bf16 else np.asarray(v, dtype=f)


def h_forward(d, bn=None, bias=False, bf16=False, order="torch", w=None, a=None):
    a = h_operand(d["x"], bn, d["stride"], bf16) if a is None else a
    y = mm(P.rows(a), h_weights(d["w"] if w is None else w, bf16).T, order)
    if bias:
        y = y + d["bias"]
    return h_store(P.unrows(y, d["N"], d["OH"], d["OW"]), bf16)


def h_dy(d, relu):
    """dy of the following BatchNorm's backward in fp32, bn_bwd_elem's operation order."""
    m, i, ga, b = (np.asarray(v, dtype=f)[None, :, None, None] for v in d["po"])
    K = d["K"]
    k1, k2 = d["k12"][:K][None, :, None, None], d["k12"][K:][None, :, None, None]
    x1, g = d["x1"].astype(f), d["g"].astype(f)
    xh = (x1 - m) * i
    if relu:
        g = np.where(ga * xh + b > 0, g, f(0))
    return (ga * i) * ((g - k1) - xh * k2)


def h_dgrad(d, dy, res=False, bf16=False, formed=False, order="torch", lattice=False):
    """dx as stored (fp32 array); dy the operand's fp32 values (rounded here when formed on load in bf16)."""
    dyo = q16(dy) if bf16 and formed else np.asarray(dy, dtype=f)
    dx = P.unrows(mm(P.rows(dyo), h_weights(d["w"], bf16), order), d["N"], d["OH"], d["OW"])
    if lattice:
        return h_store(dx, bf16)
    if res:
        on = P.widen(np.ones((d["N"], 1, d["OH"], d["OW"])), d["stride"]) > 0
        r32 = d["res"].astype(f)
        return h_store(np.where(on, P.widen(dx, d["stride"]).astype(f) + r32, r32), bf16)
    return h_store(P.widen(dx, d["stride"]), bf16)


def h_wgrad(d, dyo, ao, l2=0.0, order="torch"):
    dw = mm(P.rows(dyo).T, P.rows(ao), order)
    return dw + f(l2) * d["w"] if l2 else dw


def h_stats(stored):
    s = P.rows(np.asarray(stored, dtype=np.float64))
    return np.stack([s.sum(0), (s * s).sum(0)])[None]


def h_part(stored, xl, bn, mask=True):
    """(1, 2, C): fp32 x_hat and mask, fp64 products and sums (gemm_engine.h bn_bwd_contrib)."""
    m, i, ga, b = (np.asarray(v, dtype=f)[None, :, None, None] for v in bn[:4])
    xh = (xl.astype(f) - m) * i
    g = np.asarray(stored, dtype=f)
    if bn[4] and mask:
        g = np.where(ga * xh + b > 0, g, f(0))
    g, xh = P.rows(g.astype(np.float64)), P.rows(xh.astype(np.float64))
    return np.stack([g.sum(0), (g * xh).sum(0)])[None]


def stored_check(name, got, r, bf16):
    if bf16:
        P.check(name + " closed", got, r.ref, r.b16c)
    P.check(name, got, r.ref, r.bound(bf16))


# ---------------------------------------------------------------------------------------------------------
# the reference equals the oracle
# ---------------------------------------------------------------------------------------------------------

def _close(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("cid", CIDS)
def test_reference_agrees_with_oracle(cid):
    d = P.make_inputs(cid)
    w64, b64, st = d["w"].astype(np.float64), d["bias"].astype(np.float64), d["stride"]
    for bias in (False, True):
        for l2 in (0.0, L2):
            y, cache = oref.pointwise_forward(d["x"], w64, b64 if bias else None, st)
            dx, dw, _ = oref.pointwise_backward(d["dy"], w64, cache, st, bias, l2)
            r = P.forward(d["x"], d["w"], st, d["bias"] if bias else None)
            _close(r.ref, y)
            _close(P.dgrad(d["dy"], d["w"], st).ref, dx)
            _close(P.dgrad(d["dy"], d["w"], st, lattice=True).ref, dx[:, :, ::st, ::st])
            _close(P.wgrad(d["dy"], r.a, d["w"], l2).ref, dw)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("cid", CIDS)
def test_bn_compositions_agree_with_oracle(cid, relu):
    """BatchNorm (+ ReLU) on load -> forward, and the following BatchNorm's backward -> dgrad / wgrad, through
    oracle.ref.bn_forward_test / bn_backward / relu_* (the folded coefficients k1 = mean(g'), k2 = mean(g' x_hat)
    of that BatchNorm's own batch statistics)."""
    d = P.make_inputs(cid)
    w64, st = d["w"].astype(np.float64), d["stride"]
    m, i, ga, be = (np.asarray(v, dtype=np.float64) for v in d["pi"])
    bc = lambda v: v[None, :, None, None]    # noqa: E731
    a = oref.bn_forward_test(d["x"], bc(ga), bc(be), bc(m), bc(1.0 / i))
    if relu:
        a, _ = oref.relu_forward(a)
    y, cache = oref.pointwise_forward(a, w64, None, st)
    r = P.forward(d["x"], d["w"], st, None, (*d["pi"], relu))
    _close(r.ref, y)
    # the following BatchNorm in training mode on x1, its backward applied to g
    ga2, be2 = (np.asarray(v, dtype=np.float64) for v in d["po"][2:])
    out, bcache, _, _ = oref.bn_forward_train(d["x1"], bc(ga2), bc(be2), None, None)
    g = d["g"]
    if relu:
        _, mask = oref.relu_forward(out)
        g = oref.relu_backward(g, mask)
    dy_o, _, _ = oref.bn_backward(g, bc(ga2), bcache)
    mean, invstd = d["x1"].mean(axis=(0, 2, 3)), 1.0 / bcache["std"].ravel()
    xh = (d["x1"] - bc(mean)) * bc(invstd)
    k12 = np.concatenate([g.mean(axis=(0, 2, 3)), (g * xh).mean(axis=(0, 2, 3))])
    dy, _, _ = P.bn_bwd_dy(d["g"], d["x1"], (mean, invstd, ga2, be2, relu), k12)
    _close(dy, dy_o)
    dx, dw, _ = oref.pointwise_backward(dy_o, w64, cache, st, False, L2)
    _close(P.dgrad(dy, d["w"], st).ref, dx)
    _close(P.wgrad(dy, r.a, d["w"], L2).ref, dw)


@pytest.mark.parametrize("cid", CIDS)
def test_inputs_keep_the_relu_masks_decided(cid):
    """Precondition of every ReLU case: no element of either BatchNorm's output lies within
    8 u (|gamma x_hat| + |beta|) of zero, so fp32 and fp64 decide the masks alike."""
    assert P.margins(P.make_inputs(cid)) > 1.0


def test_widened_zeros_have_a_zero_bound():
    d = P.make_inputs(3)
    for res in (None, d["res"]):
        r = P.dgrad(d["dy"], d["w"], 2, res)
        off = P.widen(np.ones((d["N"], 1, d["OH"], d["OW"])), 2) == 0
        off = np.broadcast_to(off, r.A.shape)
        assert (r.A[off] == 0).all() and (r.b16[off] == 0).all() and (r.A[~off] > 0).all()
        assert (r.ref[off] == (0 if res is None else res[off])).all()


# ---------------------------------------------------------------------------------------------------------
# the bounds admit the honest implementation
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bf16,order", MODES, ids=["{}-{}".format("bf16" if b else "f32", o) for b, o in MODES])
@pytest.mark.parametrize("cid", CIDS)
def test_bounds_admit_the_honest_forward_and_wgrad(cid, bf16, order):
    d = P.make_inputs(cid)
    st, t = d["stride"], "c{} {}".format(cid, "bf16" if bf16 else "f32")
    for bn in (None, 0, 1):
        bnp = None if bn is None else (*d["pi"], bn)
        for bias in (False, True):
            r = P.forward(d["x"], d["w"], st, d["bias"] if bias else None, bnp, bf16)
            y = h_forward(d, bnp, bias, bf16, order)
            stored_check(t + " fwd y", y, r, bf16)
            P.stats_checks(t + " fwd stats", h_stats(y), y, r.ref, r.bound(bf16))
        for l2 in (0.0, L2):
            rw = P.wgrad(d["dy"], r.a, d["w"], l2, None, r.ea)
            P.check(t + " wgrad dw", h_wgrad(d, d["dy"].astype(f), h_operand(d["x"], bnp, st, bf16), l2, order),
                    rw.ref, rw.A)


@pytest.mark.parametrize("bf16,order", MODES, ids=["{}-{}".format("bf16" if b else "f32", o) for b, o in MODES])
@pytest.mark.parametrize("cid", CIDS)
def test_bounds_admit_the_honest_dgrad(cid, bf16, order):
    d = P.make_inputs(cid)
    st, t = d["stride"], "c{} {}".format(cid, "bf16" if bf16 else "f32")
    for res in (False, True):
        r = P.dgrad(d["dy"], d["w"], st, d["res"] if res else None, bf16=bf16)
        dx = h_dgrad(d, d["dy"], res, bf16, False, order)
        stored_check(t + " dgrad dx", dx, r, bf16)
        if res and st > 1:
            continue    # (partials beside a residual at stride > 1 are refused)
        for relu in (0, 1):
            bn = (*d["pi"], relu)
            P.part_checks(t + " dgrad part", h_part(P.sample(dx, st), P.sample(d["xg"], st), bn), P.sample(dx, st),
                          P.sample(d["xg"], st), bn, P.sample(r.ref, st), P.sample(r.bound(bf16), st))
    r = P.dgrad(d["dy"], d["w"], st, bf16=bf16, lattice=True)
    stored_check(t + " lattice dx", h_dgrad(d, d["dy"], False, bf16, False, order, lattice=True), r, bf16)


@pytest.mark.parametrize("bf16,order", MODES, ids=["{}-{}".format("bf16" if b else "f32", o) for b, o in MODES])
@pytest.mark.parametrize("cid", [c for c in CIDS if P.CASES[c][2] == 1])
def test_bounds_admit_the_honest_bn_backward_on_load(cid, bf16, order):
    """dy formed in fp32, written through, the dgrad (+ residual, partials) and the fused weight gradient."""
    d = P.make_inputs(cid)
    t = "c{} {}".format(cid, "bf16" if bf16 else "f32")
    for relu in (0, 1):
        dy, ed, _ = P.bn_bwd_dy(d["g"], d["x1"], (*d["po"], relu), d["k12"])
        dy32 = h_dy(d, relu)
        P.check(t + " bnbwd dy_out", h_store(dy32, bf16), dy, P.bf16_bound(dy, ed) if bf16 else ed)
        if bf16:
            P.check(t + " bnbwd dy_out closed", h_store(dy32, bf16), dy, P.bf16_closed(dy, ed))
        dys = h_store(dy32, bf16).astype(np.float64)
        for res in (False, True):
            r = P.dgrad(dy, d["w"], 1, d["res"] if res else None, ed, bf16, True)
            dx = h_dgrad(d, dy32, res, bf16, True, order)
            stored_check(t + " bnbwd dx", dx, r, bf16)
            rs = P.dgrad(dys, d["w"], 1, d["res"] if res else None, bf16=bf16)
            stored_check(t + " bnbwd dx|dy_out", dx, rs, bf16)
            bn = (*d["pi"], 1)
            P.part_checks(t + " bnbwd part", h_part(dx, d["x"], bn), dx, d["x"], bn, r.ref, r.bound(bf16))
        for bn in (None, 1):
            bnp = None if bn is None else (*d["pi"], bn)
            fw = P.forward(d["x"], d["w"], 1, None, bnp, bf16)
            rw = P.wgrad(dy, fw.a, d["w"], L2, P.operand_err(dy, ed, bf16), fw.ea)
            dw = h_wgrad(d, q16(dy32) if bf16 else dy32, h_operand(d["x"], bnp, 1, bf16), L2, order)
            P.check(t + " fused dw", dw, rw.ref, rw.A)


# ---------------------------------------------------------------------------------------------------------
# the bounds reject wrong kernels
# ---------------------------------------------------------------------------------------------------------

def _rel(a, b):
    return float(np.linalg.norm((np.asarray(a, np.float64) - b).ravel()) / np.linalg.norm(b.ravel()))


def mutant(k):
    """(name, got, ref, bound): a mutation of the honest implementation against the bound that must reject it."""
    if k == "1":        # the last pixel of a ragged tile (pixel 428 of 429) left at zero
        d = P.make_inputs(1)
        r, y = P.forward(d["x"], d["w"], 1), h_forward(d).copy()
        y[-1, :, -1, -1] = 0
        return "ragged tile's last pixel unwritten", y, r.ref, r.A
    if k == "2f":       # the last k-step of the fp32 reduction (2 channels of 512) dropped
        d = P.make_inputs(14)
        w = d["w"].copy()
        w[:, -2:] = 0
        r = P.forward(d["x"], d["w"], 1)
        return "last fp32 k-step dropped", h_forward(d, w=w), r.ref, r.A
    if k == "2h":       # the last bf16 k-step (16 channels of 512) dropped
        d = P.make_inputs(14)
        w = d["w"].copy()
        w[:, -16:] = 0
        r = P.forward(d["x"], d["w"], 1, bf16=True)
        return "last bf16 k-step dropped", h_forward(d, bf16=True, w=w), r.ref, r.b16
    if k == "3":        # one 32-column block of w used with its rows shifted by one
        d = P.make_inputs(8)
        w = d["w"].copy()
        w[32:64] = np.roll(w[32:64], 1, axis=0)
        r = P.forward(d["x"], d["w"], 1)
        return "32-column block of w shifted", h_forward(d, w=w), r.ref, r.A
    if k == "4":        # the bias added to column k + 32
        d = P.make_inputs(1)
        r = P.forward(d["x"], d["w"], 1, d["bias"])
        return "bias on column k + 32", h_forward(d) + np.roll(d["bias"], 32)[None, :, None, None], r.ref, r.A
    if k == "5":        # the ReLU of the on-load BatchNorm skipped for one channel
        d = P.make_inputs(14)
        bn = (*d["pi"], 1)
        a = h_operand(d["x"], bn, 1, False).copy()
        a[:, 7] = h_operand(d["x"], (*d["pi"], 0), 1, False)[:, 7]
        r = P.forward(d["x"], d["w"], 1, None, bn)
        return "on-load ReLU skipped for one channel", h_forward(d, a=a), r.ref, r.A
    if k in ("6a", "6b"):   # the residual added twice / omitted on the last (ragged) 64-pixel tile
        d = P.make_inputs(1)
        r = P.dgrad(d["dy"], d["w"], 1, d["res"])
        dx = P.rows(h_dgrad(d, d["dy"], True)).copy()
        dx[384:] += (1 if k == "6a" else -1) * P.rows(d["res"].astype(f))[384:]
        return ("residual twice on the last tile" if k == "6a" else "residual omitted on the last tile",
                P.unrows(dx, d["N"], d["OH"], d["OW"]), r.ref, r.A)
    if k == "7":        # a truncating bf16 store instead of round-to-nearest-even
        d = P.make_inputs(1)
        r = P.forward(d["x"], d["w"], 1, bf16=True)
        return "bf16 store truncating", trunc16(h_forward(d, w=q16(d["w"]))), r.ref, r.b16
    if k == "8":        # the l2 term dropped (case 2, M = 5: the M-term bound of a long reduction hides 1e-3 w)
        d = P.make_inputs(2)
        r = P.wgrad(d["dy"], d["x"], d["w"], L2)
        return "l2 term dropped", h_wgrad(d, d["dy"].astype(f), d["x"].astype(f), 0.0), r.ref, r.A
    if k == "9":        # the weight gradient misses the last ragged tile's pixels
        d = P.make_inputs(1)
        r = P.wgrad(d["dy"], d["x"], d["w"], L2)
        dy = P.rows(d["dy"].astype(f)).copy()
        dy[384:] = 0
        return ("wgrad misses the last tile", h_wgrad(d, P.unrows(dy, d["N"], d["OH"], d["OW"]), d["x"].astype(f), L2),
                r.ref, r.A)
    if k == "10":       # dy formed without its k2 x_hat term
        d = P.make_inputs(1)
        dy, ed, _ = P.bn_bwd_dy(d["g"], d["x1"], (*d["po"], 1), d["k12"])
        dd = dict(d, k12=np.concatenate([d["k12"][:64], np.zeros(64, f)]))
        r = P.dgrad(dy, d["w"], 1, None, ed, False, True)
        return "dy without k2 x_hat", h_dgrad(d, h_dy(dd, 1)), r.ref, r.A
    if k == "13":       # stride 2: a sampled at (2 oh + 1, 2 ow)
        d = P.make_inputs(3)
        r = P.forward(d["x"], d["w"], 2)
        a = d["x"].astype(f)[:, :, 1::2, ::2]
        a = np.concatenate([a, a[:, :, -1:]], axis=2)     # (H = 13: six odd rows; the seventh repeats the last)
        return "stride-2 lattice off by one row", h_forward(d, a=a), r.ref, r.A
    raise KeyError(k)


BELOW_1E4 = {"8"}       # the mutants a normwise 1e-4 lets through at these shapes (asserted below)


@pytest.mark.parametrize("k", ["1", "2f", "2h", "3", "4", "5", "6a", "6b", "7", "8", "9", "10", "13"])
def test_bounds_reject_mutants(k):
    name, got, ref, bound = mutant(k)
    ratio, at = P.worst(got, ref, bound)
    norm = _rel(got, ref)
    print("mutant {} ({}): worst err/bound {:.3g} at {}, normwise {:.3g}".format(k, name, ratio, at, norm))
    assert ratio > 1.0, (name, ratio)
    if k == "7":
        # against the closed form alone a truncating store stays within a factor of 2; bf16 tensors are held
        # normwise to 1e-2 elsewhere in the suite, which passes it
        r = P.forward(P.make_inputs(1)["x"], P.make_inputs(1)["w"], 1, bf16=True)
        assert 1.0 < P.worst(got, ref, r.b16c)[0] < 2.0 and 1e-4 < norm < 1e-2
    else:
        assert (norm < 1e-4) == (k in BELOW_1E4), (name, norm)


def test_bounds_reject_statistics_mutants():
    """11: statistics over the unrounded bf16 y; 12: partials with the ReLU mask ignored; and a ragged row
    dropped from the statistics -- all through the sums-of-the-stored-outputs check."""
    d = P.make_inputs(1)
    r = P.forward(d["x"], d["w"], 1, bf16=True)
    y32 = h_forward(d, w=q16(d["w"]))       # fp32 values before the store
    y = q16(y32)
    with pytest.raises(AssertionError, match="stored"):
        P.stats_checks("m11", h_stats(y32), y, r.ref, r.b16)
    P.stats_checks("m11 ref only", h_stats(y), y, r.ref, r.b16)
    s, s32 = P.rows(y.astype(np.float64)), P.rows(y32.astype(np.float64))
    acc = P.EPS * (s.shape[0] + 3)
    print("mutant 11: err/bound {:.3g} (sum), {:.3g} (squares)".format(
        P.worst(s32.sum(0), s.sum(0), acc * np.abs(s).sum(0))[0],
        P.worst((s32 * s32).sum(0), (s * s).sum(0), acc * (s * s).sum(0))[0]))
    short = y.copy()
    short[-1, :, -1, -1] = 0
    with pytest.raises(AssertionError, match="stored"):
        P.stats_checks("dropped row", h_stats(short), y, r.ref, r.b16)
    rd = P.dgrad(d["dy"], d["w"], 1)
    dx = h_dgrad(d, d["dy"])
    bn = (*d["pi"], 1)
    with pytest.raises(AssertionError, match="stored"):
        P.part_checks("m12", h_part(dx, d["x"], bn, mask=False), dx, d["x"], bn, rd.ref, rd.A)
    g = P.rows(dx.astype(np.float64))
    m = P.rows(P.bn_operand(d["x"], bn)[2] > 0)
    print("mutant 12: err/bound {:.3g}".format(
        P.worst(g.sum(0), (g * m).sum(0), P.EPS * (g.shape[0] + 3) * np.abs(g * m).sum(0))[0]))


def test_truncated_weight_operand():
    """The bf16 weight operand rounded by truncation instead of to nearest even.  Rejected where the
    activations are raw bf16 and y or dx is stored in bf16 (the reference's wq is exact, and the interval
    form leaves an element whose reference lies next to a bf16 value no room for another value); NOT
    rejectable behind a BatchNorm on load (the operand's own 2^-8 slack is as large as the weight's error)
    and not visible in any weight gradient (the bf16 weight gradient's operands are dy and a; w enters only
    as the fp32 l2 term)."""
    d = P.make_inputs(1)
    wt = trunc16(d["w"])
    r = P.forward(d["x"], d["w"], 1, bf16=True)
    y = q16(P.unrows(mm(P.rows(d["x"].astype(f)), wt.T), d["N"], d["OH"], d["OW"]))
    raw = P.worst(y, r.ref, r.b16)[0]
    bn = (*d["pi"], 1)
    rb = P.forward(d["x"], d["w"], 1, None, bn, True)
    yb = q16(P.unrows(mm(P.rows(h_operand(d["x"], bn, 1, True)), wt.T), d["N"], d["OH"], d["OW"]))
    behind_bn = P.worst(yb, rb.ref, rb.b16)[0]
    print("truncated weight operand: raw bf16 y {:.3g}, behind BN on load {:.3g}, normwise {:.3g}".format(
        raw, behind_bn, _rel(y, r.ref)))
    assert raw > 1.0 and behind_bn > 1.0
