"""Every producer of BatchNorm partial rows against its row query (tests/_partials.py TABLE).

A kernel that produces an output also writes fp64 partial rows part[rows][2][C]; the caller sizes
the buffer from a separate dk_*_rows() query and a fold (in-launch, or dk_bn_*_from_partials_f32)
reduces all `rows` rows.  Query and launch compute the count independently, from tile / segment
rules that depend on the storage type, the shape and the tuning knobs: if they disagree, rows stay
unwritten (uninitialised memory in dgamma, dbeta, k12, mean, std) or the kernel writes past the
buffer, and an armed fold is refused without an error.  Per entry:

  * row contract: rows > 0; into rows + 2 rows of NaN the unarmed launch returns 0, leaves every
    element of part[:rows] finite and both guard rows NaN, and every other output finite;
  * armed: with dk_bn_fold_arm_* armed for exactly `rows` rows the launch returns DK_FOLDED and
    the in-launch results equal the separate fold's (check_stats / check_bwd);
  * reference: part[:rows].sum(0) against plain torch fp64 sums over the values the kernel
    stored, per channel |sum - ref| <= (k + 4) 2^-24 sum|term| -- k the longest fp32 chain the
    kernel accumulates before widening to fp64 (read from the kernel, cited in the table), + 4
    for forming the term in fp32;
  * under a knob: the row contract again with the producer's tuning knob off its default.

With DORKNET_PARTIALS_REPORT=<file> the run writes the observed rows, k and err / bound per entry
(profiles/partial_rows_contract.md is that file)."""
import os

import numpy as np
import pytest
import torch

from dorknet_amd._hip import lib
from tests._partials import BF16, F32, NAN, TABLE, check_bwd, check_stats, dw_dgrad, dw_fwd, knobs

pytestmark = pytest.mark.gpu

IDS = [e["id"] for e in TABLE]
_report = {}


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    path = os.environ.get("DORKNET_PARTIALS_REPORT")
    if not path or not _report:
        return
    with open(path, "w") as f:
        f.write("# BatchNorm partial rows: query vs launch, and the sums against fp64\n\n"
                "Written by `tests/test_gpu_partial_rows.py` (DORKNET_PARTIALS_REPORT) on an MI355X.  rows: the\n"
                "entry's row query at the test shape; k: the longest fp32 accumulation before the kernel widens\n"
                "to fp64 (source line in `tests/_partials.py`); err / bound: the worst channel's\n"
                "|sum - ref| / ((k + 4) 2^-24 sum|term|) against torch fp64 sums of the stored values (must be < 1).\n\n"
                "| entry | entry point | row query | type | shape | rows | k | err / bound |\n"
                "|---|---|---|---|---|---|---|---|\n")
        for e in TABLE:
            if e["id"] in _report:
                rows, ratio = _report[e["id"]]
                f.write("| {} | `{}` | `{}` | {} | {} | {} | {} | {:.3g} |\n".format(
                    e["id"], e["entry"], e["query"], e["dtype"], "x".join(str(v) for v in e["shape"]), rows, e["k"],
                    ratio))


def row_contract(case):
    assert case.rows > 0
    part = torch.full((case.rows + 2, 2, case.C), NAN, dtype=torch.float64, device="cuda")
    case.poison()
    assert case.launch(part.data_ptr()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(part[:case.rows]).all()), "a row the query counts was not written"
    assert bool(torch.isnan(part[case.rows:]).all()), "a row past the query's count was written"
    for t in case.outs:
        assert bool(torch.isfinite(t.float()).all()), "an output element was not written"
    return part


@pytest.mark.parametrize("e", TABLE, ids=IDS)
def test_row_contract(e):
    other = None
    if e["other"] is not None:
        with knobs(e["other"]):
            other = e["make"]().rows
    with knobs(e["force"]):
        case = e["make"]()
        # the forced variant is the one that ran: under the other variant's knobs the query gives
        # another count, and exactly this one's rows are written
        assert other != case.rows, "the variants' row counts do not tell them apart at this shape"
        row_contract(case)


@pytest.mark.parametrize("e", TABLE, ids=IDS)
def test_armed_fold(e):
    with knobs(e["force"]):
        case = e["make"]()
        assert case.rows > 0
        rng = np.random.RandomState(len(e["id"]))
        if case.kind == "stats":
            check_stats(case.launch, case.rows, case.C, case.P, rng)
        else:
            check_bwd(case.launch, case.rows, case.C, case.P)


@pytest.mark.parametrize("e", TABLE, ids=IDS)
def test_sums_match_fp64_reference(e):
    with knobs(e["force"]):
        case = e["make"]()
        part = row_contract(case)
    s = part[:case.rows].sum(0)
    ref, mag = case.ref()
    bound = (e["k"] + 4) * 2.0 ** -24 * mag
    err = (s - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print("{}: rows {} k {} err/bound {:.3g}".format(e["id"], case.rows, e["k"], ratio))
    _report[e["id"]] = (case.rows, ratio)
    # (a channel whose fused ReLU masks every element has sum|term| = 0: its sums must be exactly 0)
    assert float(mag.max()) > 0
    assert ratio < 1.0, (e["id"], ratio, e["k_src"])


KNOBBED = [e for e in TABLE if e["knob"] is not None]


@pytest.mark.parametrize("e", KNOBBED, ids=[e["id"] for e in KNOBBED])
def test_row_contract_under_knob(e):
    with knobs(e["force"] + tuple(e["knob"])):
        row_contract(e["make"]())


def test_bf16_depthwise_writes_fewer_rows():
    """At 2 x 64 x 30 x 30 the fp32 depthwise forward and stride-1 dgrad run three row segments per
    column, the bf16 launches whole columns: a bf16 buffer sized by the fp32 query keeps unwritten rows."""
    for make in (dw_fwd, dw_dgrad):
        r32, r16 = make(F32, 2, 64, 30, 30, 1).rows, make(BF16, 2, 64, 30, 30, 1).rows
        assert 0 < r16 < r32, (make.__name__, r16, r32)
    assert lib.dk_dwconv_dgrad_bf16_stats_rows(2, 30, 30, 64, 2) == 0
    assert lib.dk_dwconv_dgrad_stats_rows(2, 30, 30, 64, 2) == 0
