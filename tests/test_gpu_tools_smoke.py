"""Every timing tool end to end at its smallest size: one repeat, a 20 ms window, 1 024 environments per family (--scale 0.001, the least the tools' own
rounding allows), its record compared in SHAPE — head keys, summary keys, row fields — with the committed record of its full run.  No figure is compared:
the tools run product paths the suite checks elsewhere, and this is about the tools still running and writing what they wrote."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = ["mlp_policy_time", "mlp_sample_time", "mlp_gauss_time", "tanh_fast_time", "mlp2_time", "gae_time", "acrobot_time", "pendulum_time", "final_obs_time",
         "time_limit_bench"]
EXTRA = {"mlp_policy_time": ["--cases", "mlp,torch,linear"]}     # the cases of its committed record, which was taken before the table and uniform rows
LIMIT_S = 120
broken = []          # the tool whose run ended by signal or at the time limit: nothing more is started on the GPU after it


def load(name):
    with open(os.path.join(ROOT, "profiles", f"{name}.json")) as f:
        return json.load(f)


def without_population(key):
    return re.sub(r"(^|/)n\d+(?=/)", "", key)


def expected_shape(name):
    """(head keys, summary keys, row fields by summary key) the tool's record must have at this size, from the committed record of its full run"""
    ref = load("mlp_policy_time" if name == "mlp_sample_time" else name)       # mlp_sample_time has no committed record: mlp_policy_time's head and row fields
    head = [k for k in ref if k not in ("summary", "runs")]
    rows = {k: list(v) for k, v in ref["summary"].items()}
    if name == "mlp_policy_time":
        rows = {k: v for k, v in rows.items() if "/mlp_mfma/" not in k}        # rows of a build that was removed (the tool's docstring)
    if name == "mlp_sample_time":
        head[head.index("forms")] = "cases"                                    # the one head field it names differently
        fields = next(iter(rows.values()))
        rows = {f"{family}/{case}/H{H}/{act}": fields for family in ref["n_envs"] for case in ("sample", "mlp", "torch") for H in (32, 64) for act in ("relu", "tanh")}
    if name == "tanh_fast_time":
        head.insert(head.index("cases"), "lib")                                # its record was taken before --lib was recorded
    if name == "time_limit_bench":
        rows = {k: v for k, v in rows.items() if k.endswith("/new")}           # no --base here: this tree's library alone
    if name == "final_obs_time":                                               # no --base here: no parent row, and the reference row is `unset`
        rows = {k: ["unset", "set"] for k in rows}
    return head, {without_population(k) for k in rows}, {without_population(k): v for k, v in rows.items()}


@pytest.mark.parametrize("name", TOOLS)
def test_tool_runs_and_writes_its_record(name, tmp_path):
    if broken:
        pytest.skip(f"{broken[0]} ended by signal or at the time limit: nothing more is started on the GPU")
    out = tmp_path / "record.json"
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", f"{name}.py"), "--repeats", "1", "--window", "0.02", "--scale", "0.001", "--out", str(out)]
                           + EXTRA.get(name, []), capture_output=True, text=True, timeout=LIMIT_S)
    except subprocess.TimeoutExpired:
        broken.append(name)
        raise
    if r.returncode < 0 or re.search(r"failed with status -\d+", r.stderr):
        broken.append(name)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    doc = json.loads(out.read_text())
    head, keys, fields = expected_shape(name)
    assert [k for k in doc if k not in ("summary", "runs")] == head
    assert ("runs" in doc) == ("runs" in load("mlp_policy_time" if name == "mlp_sample_time" else name))
    assert {without_population(k) for k in doc["summary"]} == keys
    for k, row in doc["summary"].items():
        if name == "final_obs_time":
            committed = load(name)["summary"][k]["unset"]
            assert list(row) == fields[k]
            assert all(list(v) == [f.replace("vs_parent", "vs_unset") for f in committed] for v in row.values())
        else:
            assert list(row) == fields[without_population(k)]
