"""The tiled engine's host side without a GPU (csrc/gemm_engine.h and the entries of gemm_conv.hip,
gemm_pw.hip, gemm_bf16.hip and gemm_dense.hip that tests/test_pw_args_host.py does not cover): which
arguments every entry refuses, with which status and in which order against a short workspace, and
what every row / workspace query returns over a grid of shapes and knob settings.  Refusals happen
before any HIP call, so the pointers are fake (aligned addresses that are never dereferenced) and
nothing is launched:
  * an entry with a workspace is always given one a byte short of what it checks for, so even valid
    arguments end in a refusal (`_ws_extra=1` completes it only together with a refused argument);
  * an entry without one is called only with argument sets it refuses;
  * `stats` and `part` are NULL wherever a call would otherwise proceed (a `part` is given only
    next to the argument that is refused).
The queries do not read the occupancy: the expected values are restated here from the tile tables
and hold with or without a GPU."""
import os

import pytest

from dorknet_amd import _hip

pytestmark = pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="run __graft_entry__.build() first")

# KnobId (csrc/dk_common.h)
KNOB_ROW, KNOB_SPLIT, KNOB_WGRAD_BLOCKS = 0, 1, 18

BN = ["bn_mean", "bn_invstd", "bn_gamma", "bn_beta"]
OUT = ["out_mean", "out_invstd", "out_gamma", "out_beta", "k12"]
CONV = dict(N=2, H=5, W=7, C=64, K=64, R=3, S=3, stride=1, pad=1, OH=5, OW=7)  # 70 pixels
WG = dict(N=2, H=5, W=7, Cp=64, C=64, K=64, R=3, S=3, stride=1, pad=1, OH=5, OW=7)
PHASE = dict(N=2, OH=3, OW=4, Kp=64, K=64, C=64, R=3, S=3, stride=2, pad=1, H=5, W=7)
PW = dict(N=2, H=5, W=7, C=64, K=64, stride=1, OH=5, OW=7)
PWD = dict(N=2, OH=5, OW=7, K=64, C=64, stride=1)
# tensors past 2 GiB: N for the tensor the batch scales, a large output grid for the other one
BIG_N = dict(N=240000)            # 240000 x 5 x 7 x 64 x 4 bytes
BIG_OUT = dict(OH=2100, OW=2100)  # 2 x 2100 x 2100 x 64 x 4 bytes
BIG_IN = dict(H=2100, W=2100)


def _lib(query, *names):
    # (a size below 1 is refused as an argument; the split rule is not asked about an empty problem)
    return lambda v: 0 if min(v[n] for n in names) < 1 else getattr(_hip.lib, query)(*[v[n] for n in names])


def _pw_f32(v):  # (dk_pwconv_wgrad_workspace_bytes is the larger of the two dtypes' needs: not what an entry checks)
    return _lib("dk_conv2d_wgrad_workspace_bytes", "N", "OH", "OW", "K", "C", "R", "S")(dict(v, R=1, S=1))


def _pw_bf16(v):
    return _lib("dk_conv2d_wgrad_bf16_workspace_bytes", "N", "OH", "OW", "K", "C", "R", "S")(dict(v, R=1, S=1))


CONV_WS = _lib("dk_conv2d_wgrad_workspace_bytes", "N", "OH", "OW", "K", "Cp", "R", "S")
CONV_WS16 = _lib("dk_conv2d_wgrad_bf16_workspace_bytes", "N", "OH", "OW", "K", "Cp", "R", "S")
PHASE_WS = _lib("dk_conv2d_dgrad_phase_workspace_bytes", "K", "C", "R", "S", "stride")

# name -> `scalars`: valid scalars; `null`: pointers NULL in the valid call (stats and part always);
# `required`: NULL is refused; `aligned`: 4 past a 16-byte boundary is refused; `aligned16`: of those,
# the ones also refused 8 past it (entries with a workspace: the rest go on to the workspace; entries
# without one cannot be asked); `unchecked`: NULL and 4 past a boundary are not looked at before the
# workspace; `optional`: NULL is a valid call; `bad`: argument sets refused as arguments; `late`:
# argument sets that a short workspace hides (refused as arguments only with a full one); `need`: the
# size the entry checks (None: no workspace, every call must be a refusal)
ENTRIES = {
    # ---- dense convolution, fp32 (gemm_conv.hip) ----
    "dk_conv2d_fwd_f32": dict(
        scalars=CONV, null=[], required=[], aligned=["x", "w_krsc"], aligned16=["x", "w_krsc"],
        bad=[dict(C=6), dict(C=66), BIG_N], need=None),
    "dk_conv2d_fwd_bnx_f32": dict(
        scalars=CONV, null=[], required=BN, aligned=["x", "w_krsc"] + BN, aligned16=["x", "w_krsc"] + BN,
        bad=[dict(C=6), dict(C=66), BIG_N, dict(C=2052)], need=None),
    # (bn_mean NULL is "no input BN": the call would be launched)
    "dk_conv2d_fwd_ex_f32": dict(
        scalars=CONV, null=[], required=BN[1:], aligned=["x", "w_krsc"] + BN, aligned16=["x", "w_krsc"] + BN,
        bad=[dict(C=6), dict(C=66), BIG_N, dict(C=2052)], need=None),
    "dk_conv2d_dgrad_f32": dict(
        scalars=CONV, null=[], required=[], aligned=["dy", "w_crsk"], aligned16=["dy", "w_crsk"],
        bad=[dict(K=6), dict(K=66), BIG_N], need=None),
    "dk_conv2d_dgrad_phase_f32": dict(
        scalars=PHASE, null=[], required=[], aligned=["dy", "ws"], aligned16=["dy", "ws"],
        unchecked=["w_kcrs", "dx"],
        bad=[dict(Kp=66), dict(Kp=60), dict(stride=0), dict(stride=9), dict(N=0), dict(C=0)],
        late=[BIG_OUT, BIG_IN], need=PHASE_WS),
    "dk_conv2d_wgrad_f32": dict(
        scalars=WG, null=[], required=[], aligned=["x"], aligned16=["x"],
        unchecked=["dy", "w_kcrs", "dw_kcrs", "ws"],
        bad=[dict(Cp=66), BIG_N, BIG_OUT], need=CONV_WS),
    "dk_conv2d_wgrad_bnx_f32": dict(
        scalars=WG, null=[], required=BN, aligned=["x"] + BN, aligned16=["x"] + BN,
        unchecked=["dy", "w_kcrs", "dw_kcrs", "ws"],
        bad=[dict(Cp=66), BIG_N, BIG_OUT], need=CONV_WS),
    # (bn_mean NULL is "no input BN"; a misaligned g or bn_x is refused only after the workspace)
    "dk_conv2d_wgrad_bnbwd_f32": dict(
        scalars=WG, null=[], required=OUT + BN[1:], aligned=["x"] + BN, aligned16=["x"] + BN,
        unchecked=["w_kcrs", "dw_kcrs", "ws"], optional=["bn_mean"],
        bad=[dict(Cp=66), dict(K=66), BIG_N, BIG_OUT],
        late=[dict(g=0x100004), dict(g=0x100008), dict(bn_x=0x101004), dict(bn_x=0x101008)], need=CONV_WS),
    # ---- dense convolution, bf16 (gemm_bf16.hip) ----
    "dk_conv2d_fwd_ex_bf16": dict(
        scalars=CONV, null=[], required=BN[1:], aligned=["x", "y", "w_krsc", "bias"] + BN,
        aligned16=["w_krsc", "bias"] + BN,
        bad=[dict(C=0), dict(C=6), dict(K=0), dict(K=6), dict(N=0), dict(R=0), dict(S=0), dict(stride=0), dict(OH=0),
             dict(OW=0), BIG_N, BIG_OUT, dict(C=2052)], need=None),
    "dk_conv2d_dgrad_bf16": dict(
        scalars=CONV, null=[], required=["dx"], aligned=["dy", "w_crsk"], aligned16=["w_crsk"],
        bad=[dict(K=0), dict(K=6), dict(C=0), dict(N=0), dict(R=0), dict(S=0), BIG_N, BIG_IN], need=None),
    "dk_conv2d_dgrad_phase_bf16": dict(
        scalars=PHASE, null=[], required=["dx"], aligned=["dy", "ws"], aligned16=["ws"],
        unchecked=["w_kcrs"],
        bad=[dict(Kp=66), dict(Kp=60), dict(K=0, Kp=0), dict(stride=0), dict(stride=9), dict(N=0), dict(C=0),
             dict(R=0), dict(S=0)],
        late=[BIG_OUT, BIG_IN], need=PHASE_WS),
    "dk_conv2d_wgrad_bf16": dict(
        scalars=WG, null=[], required=["dw_kcrs"], aligned=["x", "dy", "ws"], aligned16=["ws"],
        unchecked=["w_kcrs"],
        bad=[dict(Cp=0, C=0), dict(Cp=66), dict(C=0), dict(C=65), dict(K=0), dict(K=66), dict(N=0), dict(R=0),
             dict(S=0), dict(stride=0), BIG_N, BIG_OUT], need=CONV_WS16),
    "dk_conv2d_wgrad_bnx_bf16": dict(
        scalars=WG, null=[], required=["dw_kcrs"] + BN, aligned=["x", "dy", "ws"] + BN, aligned16=["ws"] + BN,
        unchecked=["w_kcrs"],
        bad=[dict(Cp=0, C=0), dict(Cp=66), dict(C=0), dict(C=65), dict(K=0), dict(K=66), dict(N=0), dict(R=0),
             dict(S=0), dict(stride=0), BIG_N, BIG_OUT], need=CONV_WS16),
    # ---- pointwise (gemm_pw.hip, gemm_bf16.hip) ----
    # (a channel count or pointer that rules out 16-byte loads selects the scalar loaders: refused
    # only at stride > 1)
    "dk_pwconv_fwd_f32": dict(
        scalars=PW, null=[], required=[], aligned=[], aligned16=[],
        bad=[BIG_N, dict(C=6, stride=2), dict(x=0x100004, stride=2), dict(w_kc=0x105008, stride=2)], need=None),
    "dk_pwconv_fwd_bnx_f32": dict(
        scalars=PW, null=[], required=BN, aligned=["x", "w_kc"] + BN, aligned16=["x", "w_kc"] + BN,
        bad=[dict(C=6), dict(C=66), BIG_N, dict(C=2052)], need=None),
    "dk_pwconv_dgrad_f32": dict(
        scalars=PWD, null=[], required=[], aligned=[], aligned16=[], bad=[BIG_N], need=None),
    # (bn_x and part NULL: the plain form.  With both, the fp32 entry takes any alignment of the input
    # BatchNorm -- scalar partial loads -- where the bf16 entry refuses it)
    "dk_pwconv_dgrad_ex_f32": dict(
        scalars=PWD, null=["residual", "bn_x"], required=[], aligned=[], aligned16=[],
        bad=[BIG_N, dict(part=0x200000), dict(bn_x=0x10a000),
             dict(part=0x200000, bn_x=0x10a000, bn_mean=None), dict(part=0x200000, bn_x=0x10a000, bn_beta=None),
             dict(part=0x200000, bn_x=0x10a000, residual=0x109000, stride=2)], need=None),
    "dk_pwconv_dgrad_ex_bf16": dict(
        scalars=PWD, null=["residual", "bn_x"], required=["dy", "dx"], aligned=["dy", "dx", "w_kc"],
        aligned16=["w_kc"],
        bad=[dict(N=0), dict(OH=0), dict(OW=0), dict(K=0), dict(K=6), dict(C=0), dict(C=6), dict(stride=0),
             dict(stride=9), BIG_N, dict(N=240000, K=4), dict(N=3800, K=4, stride=8), dict(N=70000, OH=200, OW=200),
             dict(residual=0x109004), dict(part=0x200000), dict(bn_x=0x10a000), dict(part=0x200000, bn_x=0x10a004),
             dict(part=0x200000, bn_x=0x10a000, bn_gamma=None), dict(part=0x200000, bn_x=0x10a000, bn_beta=0x10e004),
             dict(part=0x200000, bn_x=0x10a000, bn_mean=0x10b008),
             dict(part=0x200000, bn_x=0x10a000, residual=0x109000, stride=2)], need=None),
    # (part is NULL in the valid call, which is a refusal already: every other one is asked with a part)
    "dk_pwconv_dgrad_lattice_f32": dict(
        scalars=dict(PWD, stride=2), null=[], required=[], aligned=[], aligned16=[],
        bad=[{}] + [dict(o, part=0x200000) for o in (
            BIG_N, dict(N=240000, K=4), dict(stride=1), dict(stride=0), dict(dx_lat=None), dict(bn_x=None),
            dict(bn_mean=None), dict(bn_invstd=None), dict(bn_gamma=None), dict(bn_beta=None))], need=None),
    "dk_pwconv_wgrad_f32": dict(
        scalars=PW, null=[], required=[], aligned=["x"], aligned16=["x"],
        unchecked=["dy", "w_kc", "dw_kc", "ws"],
        bad=[dict(C=6), dict(C=66), BIG_N, BIG_OUT], need=_pw_f32),
    "dk_pwconv_wgrad_bnx_f32": dict(
        scalars=PW, null=[], required=BN, aligned=["x"] + BN, aligned16=["x"] + BN,
        unchecked=["dy", "w_kc", "dw_kc", "ws"],
        bad=[dict(C=6), dict(C=66), BIG_N, BIG_OUT], need=_pw_f32),
    # (bn_mean NULL is "no input BN"; the input BatchNorm is looked at only after the workspace)
    "dk_pwconv_wgrad_bnx_bf16": dict(
        scalars=PW, null=[], required=[], aligned=["x", "dy"], aligned16=[],
        unchecked=["w_kc", "dw_kc", "ws", "bn_mean"], optional=["bn_mean"],
        bad=[dict(C=6), dict(C=66), dict(K=6), dict(K=66), BIG_N, BIG_OUT],
        late=[dict(bn_invstd=None), dict(bn_gamma=None), dict(bn_beta=None), dict(bn_mean=0x10f004),
              dict(bn_beta=0x112008)], need=_pw_bf16),
    # ---- dense layer (gemm_dense.hip): the workspace is all it looks at ----
    "dk_dense_wgrad_f32": dict(
        scalars=dict(B=70, IN=64, OUT=64), null=[], required=[], aligned=[], aligned16=[],
        unchecked=["x", "dy", "w_io", "dw_io", "ws"],
        bad=[], need=_lib("dk_dense_wgrad_workspace_bytes", "B", "IN", "OUT")),
}
WITH_WS = [n for n in ENTRIES if ENTRIES[n]["need"]]


def params(name):
    return _hip.lib.declarations[name][1]


def addr(name, pname):
    return 0x100000 + 0x1000 * [p for _, p in params(name)].index(pname)


def call(name, **over):
    """Call `name` with valid arguments (every pointer a distinct 16-byte-aligned fake address or,
    where the entry's table says so, NULL; the workspace one byte short) except for `over`."""
    spec = ENTRIES[name]
    assert spec["need"] or over.pop("_refusal", False), "an entry without a workspace takes refused calls only"
    vals = dict(spec["scalars"])
    vals.update({p: None for p in spec["null"] + ["stats", "part"]})
    vals.update({k: v for k, v in over.items() if not k.startswith("_")})
    # a full workspace, statistics or partials only where the call is known to be refused as arguments
    assert over.get("_args", False) or (vals["stats"] is None and vals["part"] is None and "_ws_extra" not in over)
    args = []
    for ctype, pname in params(name):
        if pname in vals:
            args.append(vals[pname])
        elif pname == "ws_bytes":
            need = spec["need"](vals)
            # (a shape whose need is 0 cannot be a byte short: it is asked only where it is refused as an argument)
            assert need or over.get("_args", False)
            args.append(need - 1 + over.get("_ws_extra", 0) if need else 0)
        elif pname == "stream":
            args.append(None)
        elif "*" in ctype:
            args.append(addr(name, pname))
        else:
            args.append(0)  # relu flags, l2
    return getattr(_hip.lib, name)(*args)


def refused(name, **over):
    with pytest.raises(_hip.HipError, match="bad arguments"):
        call(name, _refusal=True, _args=True, **over)


def short(name, **over):
    assert ENTRIES[name]["need"]
    with pytest.raises(_hip.HipError, match="workspace too small"):
        call(name, **over)


def test_the_tables_use_the_fake_addresses():
    # the literal addresses in ENTRIES are the ones call() would pass (+ 4 or 8)
    for name, p, a in [("dk_conv2d_wgrad_bnbwd_f32", "g", 0x100000), ("dk_conv2d_wgrad_bnbwd_f32", "bn_x", 0x101000),
                       ("dk_pwconv_fwd_f32", "x", 0x100000), ("dk_pwconv_fwd_f32", "w_kc", 0x105000),
                       ("dk_pwconv_dgrad_ex_f32", "residual", 0x109000), ("dk_pwconv_dgrad_ex_f32", "bn_x", 0x10a000),
                       ("dk_pwconv_dgrad_ex_bf16", "residual", 0x109000), ("dk_pwconv_dgrad_ex_bf16", "bn_x", 0x10a000),
                       ("dk_pwconv_dgrad_ex_bf16", "bn_mean", 0x10b000), ("dk_pwconv_dgrad_ex_bf16", "bn_beta", 0x10e000),
                       ("dk_pwconv_wgrad_bnx_bf16", "bn_mean", 0x10f000), ("dk_pwconv_wgrad_bnx_bf16", "bn_beta", 0x112000)]:
        assert addr(name, p) == a, (name, p, hex(addr(name, p)))
    assert sorted(ENTRIES) == sorted(n for n in ENTRIES if n in _hip.lib.declarations)


@pytest.mark.parametrize("name", WITH_WS)
def test_workspace_one_byte_short(name):
    # valid arguments: the workspace is what is refused, at the size the entry itself checks
    short(name)
    for p in ENTRIES[name].get("optional", []):  # "no input BN"
        short(name, **{p: None})


@pytest.mark.parametrize("name", list(ENTRIES))
def test_null_and_misaligned_pointers(name):
    spec = ENTRIES[name]
    for p in spec["required"]:
        refused(name, **{p: None})
    for p in spec["aligned"]:
        refused(name, **{p: addr(name, p) + 4})
    for p in spec["aligned16"]:
        refused(name, **{p: addr(name, p) + 8})
    if not spec["need"]:
        return
    for p in set(spec["aligned"]) - set(spec["aligned16"]):  # bf16 tensors, read in 8-byte groups
        short(name, **{p: addr(name, p) + 8})
    for p in spec["unchecked"]:
        short(name, **{p: addr(name, p) + 4})
        short(name, **{p: None})


@pytest.mark.parametrize("name", list(ENTRIES))
def test_scalars_and_their_order_against_the_workspace(name):
    spec = ENTRIES[name]
    for over in spec["bad"]:
        refused(name, **over)  # a bad argument wins over the short workspace
    for over in spec.get("late", []):
        short(name, **over)  # the workspace is looked at first ...
        refused(name, _ws_extra=1, **over)  # ... and a full one leaves the argument to refuse


def test_phase_dgrads_report_a_short_workspace_before_the_2gib_limits():
    for name in ("dk_conv2d_dgrad_phase_f32", "dk_conv2d_dgrad_phase_bf16"):
        # Kp != roundup4(K) has the workspace's status, with a short workspace and with a full one
        for extra in ({}, dict(_ws_extra=1, _args=True)):
            with pytest.raises(_hip.HipError, match="workspace too small"):
                call(name, Kp=68, K=61, **extra)
            with pytest.raises(_hip.HipError, match="workspace too small"):
                call(name, Kp=64, K=60, **extra)
        short(name, Kp=64, K=61)
        short(name, **dict(BIG_OUT, **BIG_IN))
        refused(name, _ws_extra=1, **dict(BIG_OUT, **BIG_IN))
    # the weight gradients look at the 2 GiB limit of dy first (`bad` above) and at nothing after the workspace
    for name in ("dk_conv2d_wgrad_f32", "dk_conv2d_wgrad_bnx_f32", "dk_pwconv_wgrad_f32", "dk_pwconv_wgrad_bnx_f32"):
        short(name, K=6)  # (fp32: K % 4 only selects the scalar loader of dy)


def test_pointwise_wgrad_workspace_is_the_larger_of_the_two_dtypes():
    lib = _hip.lib
    for M, K, C in [(70, 64, 64), (257, 128, 128), (129, 256, 64), (65, 64, 512)]:
        f, h = _pw_f32(dict(N=1, OH=1, OW=M, K=K, C=C)), _pw_bf16(dict(N=1, OH=1, OW=M, K=K, C=C))
        assert lib.dk_pwconv_wgrad_workspace_bytes(1, 1, M, K, C) == max(f, h)


# ---- the row / workspace queries ----
# tile tables of csrc/gemm_engine.h: (BM, BN, BK) per row configuration (knob 0) and per split-K one (knob 1)
ROW_CFG = [(256, 64, 16), (128, 64, 16), (128, 64, 32), (256, 64, 32), (128, 128, 16), (128, 128, 32), (64, 64, 16),
           (128, 32, 16), (64, 64, 32), (256, 128, 16), (64, 64, 64), (128, 64, 64), (64, 128, 16), (64, 128, 32),
           (128, 64, 16), (128, 64, 32), (128, 128, 32), (128, 128, 16)]
SPLIT_CFG = [(64, 64, 16), (64, 64, 32), (64, 64, 64), (128, 128, 16), (128, 128, 32), (128, 64, 32), (64, 128, 32)]
PLAIN, CONVK = "plain", "conv"


def cdiv(a, b):
    return -(-a // b)


def row_config(N, K, kind, bf16, knobs):
    """The row tile of an M x N output with reduction K (row_config): the kinds the queries here use."""
    if knobs.get(KNOB_ROW, -1) >= 0:
        return knobs[KNOB_ROW]
    if bf16 and kind == CONVK and K > 128:
        return 16 if N >= 128 else 15
    if kind == CONVK and K <= 128 and N <= 64:
        return 14
    return 6 if K <= 128 else 8


def stats_rows(M, N, K, kind, bf16, knobs):
    return cdiv(M, ROW_CFG[row_config(N, K, kind, bf16, knobs)][0])


def splitk_bytes(M, N, Kred, bf16, knobs):
    """splitk_ws_bytes: the split-K tile (splitk_config), the splits wgrad_splits sizes for, one fp32
    M x N slab per split."""
    if knobs.get(KNOB_SPLIT, -1) >= 0:
        cfg = knobs[KNOB_SPLIT]
    elif bf16 and M >= 128 and N >= 128:
        cfg = 4
    elif M <= 64 and N > 64:
        cfg = 6
    else:
        cfg = 1
    BM, BN, BK = SPLIT_CFG[cfg]
    target = knobs.get(KNOB_WGRAD_BLOCKS, -1)
    tiles, KT = cdiv(M, BM) * cdiv(N, BN), cdiv(Kred, BK)
    splits = max(1, min(KT, cdiv(target if target > 0 else 1024, tiles)))
    return cdiv(KT, cdiv(KT, splits)) * M * N * 4


PIXELS = {1: (1, 1, 1), 63: (1, 7, 9), 64: (2, 4, 8), 65: (1, 5, 13), 129: (3, 1, 43), 257: (1, 1, 257)}
CH = (4, 64, 128, 256, 512)
GRID = [(M, K, C, R) for M in PIXELS for K in CH for C in CH for R in (1, 3, 5)]  # R x S = 1, 9, 25

# query -> (its arguments, its expected value) at a grid point, under the knobs set
QUERIES = {
    "dk_conv2d_fwd_stats_rows": (
        lambda M, K, C, R: PIXELS[M] + (K, C, R, R),
        lambda M, K, C, R, kn: stats_rows(M, K, R * R * C, CONVK, False, kn)),
    "dk_conv2d_fwd_bf16_stats_rows": (
        lambda M, K, C, R: PIXELS[M] + (K, C, R, R),
        lambda M, K, C, R, kn: stats_rows(M, K, R * R * C, CONVK, True, kn)),
    "dk_conv2d_wgrad_workspace_bytes": (
        lambda M, K, C, R: PIXELS[M] + (K, C, R, R),
        lambda M, K, C, R, kn: splitk_bytes(K, R * R * C, M, False, kn)),
    "dk_conv2d_wgrad_bf16_workspace_bytes": (
        lambda M, K, C, R: PIXELS[M] + (K, C, R, R),
        lambda M, K, C, R, kn: splitk_bytes(K, R * R * C, M, True, kn)),
    "dk_conv2d_dgrad_phase_workspace_bytes": (
        lambda M, K, C, R: (K, C, R, R, 2),
        lambda M, K, C, R, kn: C * R * R * K * 4),
    "dk_pwconv_dgrad_stats_rows": (
        lambda M, K, C, R: PIXELS[M] + (K, C),
        lambda M, K, C, R, kn: stats_rows(M, C, K, PLAIN, False, kn)),
    "dk_pwconv_dgrad_bf16_stats_rows": (
        lambda M, K, C, R: PIXELS[M] + (K, C, R),  # (the stride does not enter)
        lambda M, K, C, R, kn: stats_rows(M, C, K, PLAIN, True, kn)),
    "dk_pwconv_wgrad_workspace_bytes": (
        lambda M, K, C, R: PIXELS[M] + (K, C),
        lambda M, K, C, R, kn: max(splitk_bytes(K, C, M, False, kn), splitk_bytes(K, C, M, True, kn))),
    "dk_dense_wgrad_workspace_bytes": (
        lambda M, K, C, R: (M, K, C),
        lambda M, K, C, R, kn: splitk_bytes(K, C, M, False, kn)),
}

KNOB_SETS = ([{}] + [{KNOB_ROW: v} for v in range(len(ROW_CFG))] + [{KNOB_SPLIT: v} for v in range(len(SPLIT_CFG))] +
             [{KNOB_WGRAD_BLOCKS: v} for v in (1, 64, 256, 4096)] + [{KNOB_ROW: 9, KNOB_SPLIT: 3, KNOB_WGRAD_BLOCKS: 16}])


@pytest.fixture
def set_knobs():
    """Sets knobs for one test and restores every one of them afterwards."""
    lib = _hip.lib
    touched = set()

    def set_(knobs):
        for kind in list(touched):
            lib.dk_debug_set_gemm_config(kind, -1)
        touched.clear()
        for kind, v in knobs.items():
            touched.add(kind)
            lib.dk_debug_set_gemm_config(kind, v)
    yield set_
    for kind in (KNOB_ROW, KNOB_SPLIT, KNOB_WGRAD_BLOCKS):
        lib.dk_debug_set_gemm_config(kind, -1)


@pytest.mark.parametrize("knobs", KNOB_SETS, ids=lambda k: "-".join("knob{}={}".format(*kv) for kv in k.items()) or "default")
def test_queries_over_the_grid(knobs, set_knobs):
    lib = _hip.lib
    assert lib.dk_debug_set_gemm_config(KNOB_ROW, -1) == len(ROW_CFG)
    assert lib.dk_debug_set_gemm_config(KNOB_SPLIT, -1) == len(SPLIT_CFG)
    set_knobs(knobs)
    for query, (arguments, expected) in QUERIES.items():
        fn = getattr(lib, query)
        bad = [(p, got, want) for p in GRID
               for got, want in [(int(fn(*arguments(*p))), expected(*p, knobs))] if got != want]
        assert not bad, (query, bad[:8])


def test_the_grid_reaches_every_rule():
    # every branch of the two restated rules is taken somewhere on the grid, so each is compared with the library
    rows = {(row_config(K, R * R * C, CONVK, h, {}), h) for M, K, C, R in GRID for h in (False, True)}
    assert rows == {(6, False), (8, False), (14, False), (6, True), (14, True), (15, True), (16, True)}
    assert {row_config(C, K, PLAIN, h, {}) for M, K, C, R in GRID for h in (False, True)} == {6, 8}

    def cfg(M, N, h):
        return 4 if h and M >= 128 and N >= 128 else 6 if M <= 64 and N > 64 else 1
    assert {(cfg(K, R * R * C, h), h) for M, K, C, R in GRID for h in (False, True)} == {
        (1, False), (6, False), (1, True), (4, True), (6, True)}
    # more than one row tile, a ragged last one, and a split count the reduction length caps
    assert [stats_rows(M, 64, 576, CONVK, False, {}) for M in PIXELS] == [1, 1, 1, 2, 3, 5]
    assert [stats_rows(M, 64, 576, CONVK, True, {}) for M in PIXELS] == [1, 1, 1, 1, 2, 3]
    assert [splitk_bytes(64, 64, M, False, {}) // (64 * 64 * 4) for M in PIXELS] == [1, 2, 2, 3, 5, 9]
    assert splitk_bytes(64, 64, 257, False, {KNOB_WGRAD_BLOCKS: 4}) == 3 * 64 * 64 * 4


def test_degenerate_phase_workspace():
    lib = _hip.lib
    for K, C, R, S, stride in [(0, 64, 3, 3, 2), (64, 0, 3, 3, 2), (64, 64, 0, 3, 2), (64, 64, 3, 0, 2), (64, 64, 3, 3, 0)]:
        assert lib.dk_conv2d_dgrad_phase_workspace_bytes(K, C, R, S, stride) == 0
    assert lib.dk_conv2d_dgrad_phase_workspace_bytes(61, 3, 5, 5, 2) == 3 * 25 * 64 * 4  # K rounded up to 4
