"""tools/timing.py, the one copy of the timing tools' scheme, and what the ten tools keep of their own: the committed records rewrite byte for byte through
the shared writers, the records that keep their runs are reproduced from those runs by their tool's record(), the window, rotation, scaling and summary
arithmetic on hand values, the fresh-child loop with plain python children (nothing here opens a device), and every tool's command line."""
import argparse
import importlib
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)

import timing  # noqa: E402

LINE_RECORDS = ["mlp_policy_time", "mlp_gauss_time", "tanh_fast_time", "mlp2_time", "gae_time"]        # written by write_record
RUN_RECORDS = ["acrobot_time", "pendulum_time", "final_obs_time", "time_limit_bench"]                  # written by write_json, runs kept
# the option strings of the parent commit's add_argument calls, --worker (private) left out
OPTIONS = {
    "mlp_policy_time": {"--repeats", "--window", "--scale", "--out", "--merge", "--K", "--families", "--cases"},
    "mlp_sample_time": {"--repeats", "--window", "--scale", "--out", "--K", "--families"},
    "mlp_gauss_time": {"--repeats", "--window", "--scale", "--out", "--K", "--families"},
    "tanh_fast_time": {"--repeats", "--window", "--scale", "--out", "--K", "--lib"},
    "mlp2_time": {"--repeats", "--window", "--scale", "--out", "--K", "--lib"},
    "gae_time": {"--repeats", "--window", "--scale", "--out"},
    "acrobot_time": {"--repeats", "--window", "--scale", "--out"},
    "pendulum_time": {"--repeats", "--window", "--scale", "--out"},
    "final_obs_time": {"--base", "--repeats", "--window", "--scale", "--out"},
    "time_limit_bench": {"--base", "--repeats", "--window", "--scale", "--out"},
}


def committed(name):
    with open(os.path.join(ROOT, "profiles", f"{name}.json")) as f:
        text = f.read()
    return text, json.loads(text)


@pytest.mark.parametrize("name", LINE_RECORDS)
def test_write_record_reproduces_the_committed_bytes(name, tmp_path):
    text, doc = committed(name)
    table = doc.pop("summary")
    timing.write_record(tmp_path / "out.json", doc, table)
    assert (tmp_path / "out.json").read_text() == text


@pytest.mark.parametrize("name", RUN_RECORDS)
def test_write_json_reproduces_the_committed_bytes(name, tmp_path):
    text, doc = committed(name)
    timing.write_json(tmp_path / "out.json", doc)
    assert (tmp_path / "out.json").read_text() == text


@pytest.mark.parametrize("name", RUN_RECORDS)
def test_record_replays_the_committed_runs(name, tmp_path):
    text, doc = committed(name)
    args = argparse.Namespace(window=doc["window_s"], repeats=doc["repeats"], scale=doc["scale"])
    again = importlib.import_module(name).record(doc["runs"], args)
    assert again["summary"] == doc["summary"]            # == on floats: exact
    assert list(again) == list(doc) and all(list(again["summary"][k]) == list(v) for k, v in doc["summary"].items())
    timing.write_json(tmp_path / "out.json", again)
    assert (tmp_path / "out.json").read_text() == text


def fake_timed(ms_per_launch, calls):
    def timed(count):
        calls.append(count)
        return ms_per_launch * count
    return timed


def test_window_of_warms_probes_and_sizes_the_window():
    calls = []
    ms, count = timing.window_of(fake_timed(0.25, calls), 0.3, 5, 7)
    assert calls == [5, 7, int(0.3 * 1000 / 0.25) + 1] and count == 1201 and ms == 0.25 * 1201
    calls = []
    assert timing.window_of(fake_timed(2.0, calls), 0.5, 2, 4) == (2.0 * 251, 251) and calls == [2, 4, 251]


def test_window_of_never_times_fewer_launches_than_the_probe():
    calls = []
    ms, count = timing.window_of(fake_timed(100.0, calls), 0.3, 30, 20)     # 0.3 s holds 3 launches of 100 ms
    assert calls == [30, 20, 20] and count == 20 and ms == 2000.0


def test_rotated():
    cases = ["a", "b", "c", "d", "e"]
    assert timing.rotated(cases, 0) == cases
    assert timing.rotated(cases, 2) == ["c", "d", "e", "a", "b"]
    assert timing.rotated(cases, 5) == cases
    assert timing.rotated(cases, 7 * 3) == ["b", "c", "d", "e", "a"]
    assert cases == ["a", "b", "c", "d", "e"]


def test_scaled():
    assert timing.scaled(1 << 20, 1.0) == 1 << 20
    assert timing.scaled(1 << 20, 0.001) == 1024           # 1048.576 -> 1048 -> one block of 1024
    assert timing.scaled(1 << 18, 0.001) == 1024           # 262 -> at least 1024
    assert timing.scaled(4096, 0.001) == 1024
    assert timing.scaled(1 << 20, 0.0035) == 3072          # 3670 -> 3 * 1024
    assert timing.scaled(4096, 1.0) == 4096


def test_summarise_in_both_repeats_forms():
    values = {"b/x": [4.0, 1.0, 2.0], "a/y": [0.1234567, 0.5]}
    rows = timing.summarise(values, "list")
    assert list(rows) == ["a/y", "b/x"]
    assert list(rows["b/x"]) == ["median", "min", "max", "spread", "env_steps_per_s", "repeats"]
    assert rows["b/x"] == dict(median=2.0, min=1.0, max=4.0, spread=1.5, env_steps_per_s=5e8, repeats=[4.0, 1.0, 2.0])
    assert rows["a/y"]["median"] == (0.1234567 + 0.5) / 2 and rows["a/y"]["repeats"] == [0.123457, 0.5]
    rows = timing.summarise(values, "count")
    assert list(rows["b/x"]) == ["median", "min", "max", "spread", "repeats"]
    assert rows["b/x"] == dict(median=2.0, min=1.0, max=4.0, spread=1.5, repeats=3) and rows["a/y"]["repeats"] == 2


def test_grouped_keeps_run_order():
    runs = [dict(case="x", ns_per_env_step=3.0), dict(case="y", ns_per_env_step=1.0), dict(case="x", ns_per_env_step=2.0)]
    assert timing.grouped(runs, lambda rec: rec["case"]) == {"x": [3.0, 2.0], "y": [1.0]}


def test_run_children_parses_the_result_line_and_attaches_the_repeat(capsys):
    code = "import sys, json; print('noise'); print('RESULT ' + json.dumps([dict(case=sys.argv[1], rep=int(sys.argv[2]))]))"
    runs = timing.run_children(lambda label, rep: ["-c", code, label, str(rep)], ["p", "q"], 2, 60)
    assert runs == [dict(case="p", rep=0, repeat=0), dict(case="q", rep=0, repeat=0), dict(case="p", rep=1, repeat=1), dict(case="q", rep=1, repeat=1)]
    assert capsys.readouterr().out.splitlines() == ["repeat 0 p: done", "repeat 0 q: done", "repeat 1 p: done", "repeat 1 q: done"]
    runs = timing.run_children(lambda label, rep: ["-c", code, "only", str(rep)], [None], 1, 60, fields=lambda label, rep, position: dict(row=position, repeat=rep))
    assert runs == [dict(case="only", rep=0, row=0, repeat=0)]
    assert capsys.readouterr().out.splitlines() == ["repeat 0: done"]


@pytest.mark.parametrize("ending, status", [("sys.exit(3)", 3), ("pass", 0)], ids=["exit_3", "no_result_line"])
def test_run_children_stops_at_the_first_bad_child(ending, status, tmp_path, capsys):
    counter = tmp_path / "started"
    good = "import sys, json; open(sys.argv[1], 'a').write('x'); print('RESULT ' + json.dumps([dict(v=1)]))"
    bad = f"import sys; open(sys.argv[1], 'a').write('x'); print('child said this'); print('and this on stderr', file=sys.stderr); {ending}"
    with pytest.raises(SystemExit) as failure:
        timing.run_children(lambda label, rep: ["-c", bad if (label, rep) == ("second", 1) else good, str(counter)], ["first", "second", "third"], 3, 60)
    assert str(failure.value) == f"worker second repeat 1 failed with status {status}"
    assert counter.read_text() == "x" * 5                  # three of repeat 0, first and second of repeat 1; third and repeat 2 never started
    err = capsys.readouterr().err
    assert "child said this" in err and "and this on stderr" in err


@pytest.mark.parametrize("name", sorted(OPTIONS))
def test_command_line(name):
    r = subprocess.run([sys.executable, os.path.join(TOOLS, f"{name}.py"), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    usage = r.stdout.split("options:")[0] if "options:" in r.stdout else r.stdout.split("optional arguments:")[0]
    assert set(re.findall(r"--[A-Za-z][\w-]*", usage)) - {"--help", "--worker"} == OPTIONS[name]


def test_no_tool_keeps_a_private_copy_of_the_scheme():
    for name in OPTIONS:
        with open(os.path.join(TOOLS, f"{name}.py")) as f:
            text = f.read()
        for piece in ("subprocess.run", "statistics.median", 'startswith("RESULT ")', "Event(enable_timing", "timer_start", "// 1024 * 1024"):
            assert piece not in text, (name, piece)
        assert not re.search(r"^\s*(from|import) \w+_(time|bench)\b", text, re.M), name
