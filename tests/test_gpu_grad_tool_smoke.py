"""tools/grad_time.py end to end at its small size: one repeat, a 20 ms window, 4 096 environments only (--sizes 4096), its record compared in SHAPE — head keys,
the summary keys of that population, row fields — with the committed record of its full run, profiles/grad_time.json.  No figure is compared: the tool runs a
product path that tests/test_gpu_grad_mlp.py checks against float64, and this is about the tool still running and writing what it wrote."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 240


def test_grad_time_runs_and_writes_its_record(tmp_path):
    out = tmp_path / "record.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "grad_time.py"), "--repeats", "1", "--window", "0.02", "--sizes", "4096", "--out", str(out)],
                       capture_output=True, text=True, timeout=LIMIT_S)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    doc = json.loads(out.read_text())
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
