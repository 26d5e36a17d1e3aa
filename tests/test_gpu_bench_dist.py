"""bench.py's torch.distributed (nccl = RCCL) path on ONE GPU, as the driver's 8-GPU launch would execute it on each rank: process group,
barriers, the MAX-over-ranks reductions, the mixed configs[4] section with its agreement all-reduce, the optional all-gather of observation
shards.  Run as a CHILD process (a fresh interpreter; never a re-exec of the test process).  The reference is single-threaded and `!Send`
(/root/reference src/box_2d/lunar_lander.rs:240-249): the split over GPUs is this build's to prove."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_rccl_path_runs_on_one_gpu_as_a_child_process():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MGYM_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", LOCAL_RANK="0", WORLD_SIZE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--full", "--no-cpu-baseline"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-2000:]          # the contract: ONE JSON line on stdout (RCCL's banner goes to stderr)
    line = json.loads(lines[0])
    assert line["n_gpus"] == 1 and line["value"] > 1e10 and line["scaling"] == "weak"
    ag = line["extra"]["all_gather_observations"]
    assert isinstance(ag["ms"], float) and ag["ms"] > 0 and ag["world"] == 1 and ag["bytes_per_rank"] == (1 << 20) * 16
    assert isinstance(ag["episodes_finished_all_ranks"], int) and ag["episodes_finished_all_ranks"] > 0
    mixed = line["extra"]["mixed_configs4_this_n"]
    assert "error" not in mixed and mixed["env_steps_per_s"] > 5e8 and mixed["n_gpus"] == 1


def test_plain_bench_run_times_the_steps_asked_for_and_dumps_the_same_outputs_twice(tmp_path):
    """`bench.py --gpus 1 --steps N --warmup W` without --full: the headline only (no cpu_baseline, extra or roofline.steady), and with
    --dump-outputs the last timed step's outputs — the same words from two runs with the same arguments."""
    import numpy as np

    lines = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "3",
                            "--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [l for l in r.stdout.splitlines() if l.strip()]
        assert len(out) == 1, r.stdout[-2000:]
        lines.append(json.loads(out[0]))
    for line in lines:
        assert line["steps"] == 7 and line["warmup"] == 3 and line["unit"] == "env-steps/s" and line["higher_is_better"] is True
        assert line["dtype"] == "f32" and line["ms_per_step"] > 0 and line["value"] > 0
        assert "extra" not in line and "cpu_baseline" not in line and "steady" not in line["roofline"]
    n = 1 << 20
    shapes = {"observation": (4, n), "reward": (n,), "done": (n,), "truncated": (n,)}
    assert sorted(f.name for f in (tmp_path / "a").iterdir()) == sorted(f"cartpole_{k}.npy" for k in shapes)
    for k, shape in shapes.items():
        a, b = np.load(tmp_path / "a" / f"cartpole_{k}.npy"), np.load(tmp_path / "b" / f"cartpole_{k}.npy")
        assert a.dtype == np.float32 and a.shape == shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), k
    assert 0 < np.load(tmp_path / "a" / "cartpole_reward.npy").sum() <= n
