"""No-GPU check of the episode time limit's kernel logic: the decision header modurl_gym_amd/csrc/time_limit.h and LunarLander's
per-env step / reset source compiled for the host (tests/native/time_limit_check.cpp), against the CPU oracle inside the Python
time-limit wrapper (tests/time_limit_ref.py) — every output word equal."""
import subprocess

import numpy as np
import pytest

import native_build
from oracle import oracle as ora
from time_limit_ref import TimeLimitRef
from words import same


@pytest.fixture(scope="module")
def exe():
    return native_build.program("time_limit_check.cpp")


@pytest.mark.parametrize("limit", [40, 100])
def test_lunar_lander_source_with_a_limit_equals_oracle_plus_wrapper(exe, limit, tmp_path):
    n, steps, seed = 256, 300, 11
    path = str(tmp_path / "ll.bin")
    r = subprocess.run([exe, "ll", str(n), str(limit), str(steps), str(seed), path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = np.fromfile(path, np.uint8)
    per_step = n * (4 + 32 + 4 + 1 + 1 + 4)
    assert raw.size == 32 * n + steps * per_step
    ref = TimeLimitRef(ora.OracleVec(ora.LUNARLANDER, n, seed=seed, enable_wind=True), limit, auto_reset=True, nthreads=8)
    assert same(raw[: 32 * n].view(np.float32).reshape(8, n), ref.reset())
    off = 32 * n
    for t in range(steps):
        rec = raw[off: off + per_step]; off += per_step
        act = rec[: 4 * n].view(np.uint32)
        obs = rec[4 * n: 36 * n].view(np.float32).reshape(8, n)
        rew = rec[36 * n: 40 * n].view(np.float32)
        done, trunc = rec[40 * n: 41 * n], rec[41 * n: 42 * n]
        elapsed = rec[42 * n: 46 * n].view(np.uint32)
        eo, er, ed, et = ref.step(act)
        for g, e, nm in zip((obs, rew, done, trunc), (eo, er, ed, et), ("obs", "reward", "done", "truncated")):
            assert same(g, e), f"limit {limit} step {t}: {nm}"
        assert np.array_equal(elapsed, ref.elapsed), f"limit {limit} step {t}: elapsed"
    # the window holds what it is meant to (a condition on the oracle side): no episode of this family ends within 40 steps, so limit 40
    # truncates every env seven times in 300 steps and nothing else; limit 100 sees episodes end by `done` and by the limit
    if limit == 40:
        assert ref.kinds == {"done_only": 0, "trunc_only": 7 * n, "both": 0}, ref.kinds
    else:
        assert ref.kinds["trunc_only"] > 0 and ref.kinds["done_only"] > 0, ref.kinds


def _rule(exe, limit, set_value, steps):
    out = subprocess.run([exe, "rule", str(limit), str(set_value), str(steps)], capture_output=True, text=True, check=True).stdout.split("\n")
    stored = int(out[0])
    rows = [tuple(map(int, l.split())) for l in out[1:] if l.strip()]
    return stored, [r[0] for r in rows], [r[1] for r in rows]


@pytest.mark.parametrize("limit,set_value,steps", [(7, 0, 20), (200, 150, 100), (65535, 65530, 10), (1, 0, 3), (0, 65530, 10), (100, 70000, 4), (65535, 0xFFFFFFFF, 3)])
def test_mountain_car_counter_rule(exe, limit, set_value, steps):
    """count, compare, saturate: truncated = elapsed >= limit (>=, not ==: it stays up past the limit), the 16-bit count saturates at
    65535 and never wraps, set_elapsed clamps.  The wrapper's rule with an unbounded count is the reference."""
    stored, trunc, elapsed = _rule(exe, limit, set_value, steps)
    assert stored == min(set_value, 65535)
    e = stored
    for t in range(steps):
        e += 1                                  # the wrapper's (unbounded) count
        assert trunc[t] == int(limit != 0 and e >= limit), (t, e)
        assert elapsed[t] == min(e, 65535), (t, e)
