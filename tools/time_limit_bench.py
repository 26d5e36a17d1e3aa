#!/usr/bin/env python3
"""What the episode time limit (mgym_config::max_episode_steps) costs: this tree's libmgym.so against another build of it — the parent
commit's — in the same run, alternating, several fresh processes each.

    python tools/time_limit_bench.py --base path/to/parent/libmgym.so --repeats 5 --out profiles/time_limit_bench.json

Cases (fused auto-reset on, a ring of 64 rows of uniform random actions, HIP-event timing on the handle's stream as bench.py does, a warm-up,
windows of at least --window seconds):
    MountainCar, MountainCarContinuous   1 048 576 envs   mgym_step, mgym_rollout K = 16
    LunarLander (wind)                     262 144 envs   mgym_step, mgym_rollout K = 16 and K = 64
each with limit 0 on both libraries, and on this tree's library also with a limit: 200 for MountainCar (the uniform policy practically never
reaches the goal, so every environment is truncated and reset in place every 200 steps) and 65535 for LunarLander, where the point is a window
in which NOTHING truncates, so that the work is word for word the limit-less one: a handle takes a few thousand steps in all, fewer than the
limit, so no count can reach it — the worker records the steps each handle took (`steps_per_env`) and the largest count left at the end, and
refuses to report a LunarLander limit case in which steps_per_env >= limit (`truncation_possible` must be false).  (A limit of 1000 does
truncate here: under uniform actions a growing share of landers rests on the ground for thousands of steps.)  Which handle of a case comes
first — limit 0 or the limit — alternates from repeat to repeat.  The other library knows no limit: the field is its unused last word.
The spread of the base library's own repeats is the noise figure every comparison is read against.  One JSON document: every repeat, and per case
median, min, max and spread (max - min over median)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [  # (family, n_envs, form, K)
    ("mountain_car", 1 << 20, "step", 1), ("mountain_car", 1 << 20, "rollout", 16),
    ("mountain_car_continuous", 1 << 20, "step", 1), ("mountain_car_continuous", 1 << 20, "rollout", 16),
    ("lunar_lander", 1 << 18, "step", 1), ("lunar_lander", 1 << 18, "rollout", 16), ("lunar_lander", 1 << 18, "rollout", 64),
]
RING = 64
LIMIT = {"mountain_car": 200, "mountain_car_continuous": 200, "lunar_lander": 65535}


def worker(lib_path, with_limit, window, scale, limit_first):
    os.environ["GPU_MAX_HW_QUEUES"] = "8"   # what the test suite pins (LunarLander's helper streams on queues of their own)
    sys.path.insert(0, ROOT)
    import numpy as np
    from modurl_gym_amd import _lib
    _lib.LIB_PATH = lib_path
    import ctypes
    try:                                    # (as _lib.load does: torch's HIP runtime first, so that both share one)
        import torch  # noqa: F401
    except Exception:
        pass
    probe = ctypes.CDLL(lib_path)
    for name in [k for k in list(_lib.PROTOTYPES) if not hasattr(probe, k)]:
        del _lib.PROTOTYPES[name]           # a base library from before the two elapsed-steps calls
    import modurl_gym_amd as mg
    kinds = {"mountain_car": mg.MOUNTAINCAR, "mountain_car_continuous": mg.MOUNTAINCAR_CONT, "lunar_lander": mg.LUNARLANDER}
    rng = np.random.default_rng(1)
    out = []
    for family, n, form, K in CASES:
        n = max(1024, int(n * scale)) // 1024 * 1024
        for limit in (([LIMIT[family], 0] if limit_first else [0, LIMIT[family]]) if with_limit else [0]):
            kw = dict(enable_wind=True) if family == "lunar_lander" else {}
            env = mg.VecEnv(kinds[family], n, seed=7, auto_reset=True, max_episode_steps=limit, **kw)
            if family == "mountain_car_continuous":   # a ring of RING action rows, taken K at a time (one row repeated for ever would be a constant policy)
                acts = (rng.random((RING, n), np.float32) * 2 - 1).astype(np.float32)
            else:
                acts = rng.integers(0, 4 if family == "lunar_lander" else 3, (RING, n)).astype(np.uint32)
            d_act = mg.DeviceArray.from_numpy(acts)
            turn = [0]

            def next_actions():
                p = d_act.ptr + (turn[0] % (RING // K)) * K * n * 4
                turn[0] += 1
                return p

            d_obs = mg.DeviceArray((K, env.obs_dim, n), np.float32)
            d_rew, d_done, d_trunc = mg.DeviceArray((K, n), np.float32), mg.DeviceArray((K, n), np.uint8), mg.DeviceArray((K, n), np.uint8)
            if form == "step":
                launch = lambda: env.step_device(next_actions(), d_obs, d_rew, d_done, d_trunc)
            else:
                launch = lambda: env.rollout_device(next_actions(), K, d_obs, d_rew, d_done, d_trunc)
            env.reset_device()
            env.sync()

            def timed(count):
                env.timer_start()
                for _ in range(count):
                    launch()
                ms = env.timer_stop()
                env.sync()   # (raises on a sticky device error)
                return ms

            timed(30)                                  # warm-up
            per = timed(20) / 20                       # ms per launch
            count = max(20, int(window * 1000.0 / per) + 1)
            ms = timed(count)
            steps_per_env = (30 + 20 + count) * K
            max_elapsed = int(env.elapsed_steps().max()) if limit else None
            if family == "lunar_lander" and limit and steps_per_env >= limit:
                raise SystemExit(f"{family} {form} K={K}: {steps_per_env} steps per env reach the limit {limit}: not a window without truncations")
            out.append(dict(steps_per_env=steps_per_env, truncation_possible=bool(limit and steps_per_env >= limit), max_elapsed_at_end=max_elapsed,
                            family=family, n_envs=n, form=form, K=K, limit=limit, launches=count, window_ms=ms,
                            ns_per_env_step=ms * 1e6 / (count * K * n), ms_per_launch=ms / count, episodes=env.episode_count()))
            env.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", help="the other build of libmgym.so (the parent commit's)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0, help="seconds of timed launches per case")
    ap.add_argument("--scale", type=float, default=1.0, help="population scale (smoke runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_limit_bench.json"))
    ap.add_argument("--worker", nargs=3, metavar=("LIB", "WITH_LIMIT", "LIMIT_FIRST"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker[0], args.worker[1] == "1", args.window, args.scale, args.worker[2] == "1")
    new_lib = os.path.join(ROOT, "modurl_gym_amd", "libmgym.so")
    libs = ([("base", os.path.abspath(args.base), "0")] if args.base else []) + [("new", new_lib, "1")]
    runs = []
    for rep in range(args.repeats):           # alternating: base, new, base, new, ...
        for tag, path, with_limit in libs:
            # a fresh child per repeat: one process holds one build of the library, and the parent never opens the GPU
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", path, with_limit, str(rep % 2), "--window", str(args.window), "--scale", str(args.scale)],
                               capture_output=True, text=True, timeout=900)
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
                raise SystemExit(f"worker {tag} repeat {rep} failed with status {r.returncode}")   # nothing more is started on the GPU
            for rec in json.loads(line[0][7:]):
                runs.append(dict(rec, lib=tag, repeat=rep, limit_handle_first=bool(rep % 2)))
            print(f"repeat {rep} {tag}: done", flush=True)
    summary = {}
    for rec in runs:
        key = f"{rec['family']}/{rec['form']}{rec['K'] if rec['form'] == 'rollout' else ''}/limit{rec['limit']}/{rec['lib']}"
        summary.setdefault(key, []).append(rec["ns_per_env_step"])
    table = {k: dict(median=statistics.median(v), min=min(v), max=max(v), spread=(max(v) - min(v)) / statistics.median(v), repeats=len(v))
             for k, v in sorted(summary.items())}
    doc = dict(unit="ns per env-step", window_s=args.window, repeats=args.repeats, scale=args.scale, summary=table, runs=runs)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for k, v in table.items():
        print(f"{k:62s} median {v['median']:.4f}  min {v['min']:.4f}  max {v['max']:.4f}  spread {100 * v['spread']:.2f} %")


if __name__ == "__main__":
    main()
