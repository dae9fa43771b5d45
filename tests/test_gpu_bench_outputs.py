"""bench.py's plain run, --full and --dump-outputs (run in-process on a small batch).

A plain run prints the contract fields only and takes no run beside its timed steps; --full adds
the breakdown and the dominant entry's roofline; --dump-outputs writes the last timed step's loss,
probabilities, parameters and gradients as float32 .npy files, sampled with a fixed seed above the
size limit.
"""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONTRACT = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")


def run_bench(monkeypatch, capsys, *argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "8",
                                      *argv])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def load_dir(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_outputs(monkeypatch, capsys, tmp_path):
    import bench
    calls = []
    monkeypatch.setattr(bench, "Instrument", lambda *a, **k: calls.append("Instrument"))
    monkeypatch.setattr(bench, "cpu_baseline", lambda *a, **k: calls.append("cpu_baseline"))
    out = run_bench(monkeypatch, capsys, "--dump-outputs", str(tmp_path / "a"))
    assert calls == []
    for k in CONTRACT:
        assert k in out, k
    assert out["steps"] == 2 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "images/s" and out["higher_is_better"] is True and out["dtype"] == "fp32"
    assert out["ms_per_step"] > 0
    assert abs(out["value"] - 8 / (out["ms_per_step"] * 1e-3)) <= 1e-3 * out["value"] + 0.01
    assert out["roofline"] is None and out["cpu_baseline"] is None and "breakdown" not in out

    a = load_dir(str(tmp_path / "a"))
    assert a["probs"].shape == (8, 120) and a["loss"].size == 1
    assert np.allclose(a["probs"].sum(axis=1), 1.0, atol=1e-5)
    assert a["param.conv0.weights"].shape == (64, 3, 5, 5)
    assert a["grad.res3_pw_skip.weights"].shape == a["param.res3_pw_skip.weights"].shape
    assert any(k.startswith("grad.res8_dw2_pw_bn.") for k in a)
    for k, v in a.items():
        assert v.dtype == np.float32, k
        assert np.isfinite(v).all(), k
    assert sum(v.nbytes for v in a.values()) <= 64e6

    # above the limit every array keeps the same share of its elements, the same ones every time
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 20)
    for name in ("b", "c"):
        run_bench(monkeypatch, capsys, "--dump-outputs", str(tmp_path / name))
    b, c = load_dir(str(tmp_path / "b")), load_dir(str(tmp_path / "c"))
    assert sorted(b) == sorted(a) == sorted(c)
    total = sum(os.path.getsize(os.path.join(str(tmp_path / "b"), f)) for f in os.listdir(str(tmp_path / "b")))
    assert total <= (1 << 20) + 256 * len(b)
    w = "param.res8_dw2_pw.weights"
    assert b[w].ndim == 1 and 0 < b[w].size < a[w].size and b[w].size == c[w].size
    # the sample is a fixed selection: the initial weights are seeded, and after the same three
    # steps two runs agree to rounding on every sampled element
    assert np.allclose(b[w], c[w], rtol=1e-3, atol=1e-5)


@pytest.mark.gpu
def test_full_run_adds_breakdown_and_roofline(monkeypatch, capsys):
    out = run_bench(monkeypatch, capsys, "--full", "--cpu-sample", "0")
    for k in CONTRACT:
        assert k in out, k
    assert out["cpu_baseline"] is None
    assert out["roofline"]["kernel"] in out["breakdown"]
    assert out["roofline"]["calls_per_step"] >= 1
    assert out["breakdown"]["_total_instrumented_ms"] > 0
    assert 0 < out["step_roofline_frac"]
