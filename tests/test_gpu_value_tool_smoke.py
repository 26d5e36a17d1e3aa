"""tools/value_time.py end to end at its smallest size: one repeat, a 20 ms window, 1 024 environments (--scale 0.001), its record compared in SHAPE — head keys,
summary keys, row fields — with the committed record of its full run, profiles/value_time.json.  No figure is compared: the tool runs a product path that
tests/test_gpu_value_mlp.py checks word for word, and this is about the tool still running and writing what it wrote."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 240


def without_population(key):
    return re.sub(r"(^|/)n\d+(?=/)", "", key)


def test_value_time_runs_and_writes_its_record(tmp_path):
    out = tmp_path / "record.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "value_time.py"), "--repeats", "1", "--window", "0.02", "--scale", "0.001", "--out", str(out)],
                       capture_output=True, text=True, timeout=LIMIT_S)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    doc = json.loads(out.read_text())
    with open(os.path.join(ROOT, "profiles", "value_time.json")) as f:
        ref = json.load(f)
    assert [k for k in doc if k != "summary"] == [k for k in ref if k != "summary"]
    assert {without_population(k) for k in doc["summary"]} == {without_population(k) for k in ref["summary"]}
    fields = {without_population(k): list(v) for k, v in ref["summary"].items()}
    for k, row in doc["summary"].items():
        assert list(row) == fields[without_population(k)]
    for name in ("ratios", "final_pass"):
        assert {without_population(k) for k in doc[name]} == {without_population(k) for k in ref[name]}
        assert all(list(v) == list(next(iter(ref[name].values()))) for v in doc[name].values())
