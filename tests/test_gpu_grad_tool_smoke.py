"""tools/grad_time.py end to end at its small size, with one hidden layer and with --hidden2 8: one repeat, a 20 ms window, 4 096 environments only
(--sizes 4096).  No figure is compared: the tool runs a product path that tests/test_gpu_grad_mlp.py checks against float64, and this is about the tool and
its option still running and writing their records."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 240


def record(tmp_path, *options):
    out = tmp_path / "record.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "grad_time.py"), *options, "--repeats", "1", "--window", "0.02", "--sizes", "4096", "--out", str(out)],
                       capture_output=True, text=True, timeout=LIMIT_S)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(out.read_text())


def test_grad_time_runs_and_writes_its_record(tmp_path):
    """the record compared in SHAPE — head keys, the summary keys of that population, row fields — with the committed record of the tool's full run,
    profiles/grad_time.json"""
    doc = record(tmp_path)
    with open(os.path.join(ROOT, "profiles", "grad_time.json")) as f:
        ref = json.load(f)
    assert [k for k in doc if k != "summary"] == [k for k in ref if k != "summary"]
    assert doc["n_envs"] == [4096] and doc["repeats"] == 1
    small = {k: v for k, v in ref["summary"].items() if "/n4096/" in k}
    assert len(small) == 2 * 2 * 2 * 5 and set(doc["summary"]) == set(small)
    for k, row in doc["summary"].items():
        assert list(row) == list(small[k]) and row["median"] > 0 and len(row["repeats"]) == 1
    assert set(doc["ratios"]) == {k for k in ref["ratios"] if "/n4096/" in k}
    assert all(list(v) == list(next(iter(ref["ratios"].values()))) for v in doc["ratios"].values())


def test_grad_time_hidden2_runs_and_writes_its_record(tmp_path):
    """the record names the two-layer run (hidden2, the nets "32x8" and "64x8"), holds every row of that population with a positive median, and the ratios of
    every row"""
    doc = record(tmp_path, "--hidden2", "8")
    assert doc["hidden2"] == 8 and doc["nets"] == ["32x8", "64x8"] and doc["n_envs"] == [4096] and doc["repeats"] == 1
    rows = {f"{f}/n4096/{net}/{act}" for f in ("cartpole", "pendulum") for net in ("32x8", "64x8") for act in ("relu", "tanh_fast")}
    assert set(doc["summary"]) == {f"{row}/{c}" for row in rows for c in ("ppo", "ppo4", "value", "logp", "torch")}
    for row in doc["summary"].values():
        assert row["median"] > 0 and len(row["repeats"]) == 1
    assert set(doc["ratios"]) == rows
    assert all({"torch_over_ppo", "faster_beyond_spread", "ppo4_over_ppo", "ppo_over_logp"} <= set(v) for v in doc["ratios"].values())
