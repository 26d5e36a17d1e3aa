#!/usr/bin/env python3
"""What the episode time limit (mgym_config::max_episode_steps) costs: this tree's libmgym.so against another build of it — the parent
commit's — in the same run, alternating, several fresh processes each.

    python tools/time_limit_bench.py --base path/to/parent/libmgym.so --repeats 5 --out profiles/time_limit_bench.json

Cases (fused auto-reset on, a ring of 64 rows of uniform random actions; the timing is tools/timing.py's: the handle's timer, a warm-up of 30
launches and a probe of 20, a fresh process per library and repeat):
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
import os
import sys

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, PROBE = 30, 20   # launches before the window: they count towards the steps a handle has taken

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
        n = timing.scaled(n, scale)
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

            ms, count = timing.window_of(timing.engine_timed(env, launch), window, WARM, PROBE)
            steps_per_env = (WARM + PROBE + count) * K
            max_elapsed = int(env.elapsed_steps().max()) if limit else None
            if family == "lunar_lander" and limit and steps_per_env >= limit:
                raise SystemExit(f"{family} {form} K={K}: {steps_per_env} steps per env reach the limit {limit}: not a window without truncations")
            out.append(dict(steps_per_env=steps_per_env, truncation_possible=bool(limit and steps_per_env >= limit), max_elapsed_at_end=max_elapsed,
                            family=family, n_envs=n, form=form, K=K, limit=limit, launches=count, window_ms=ms,
                            ns_per_env_step=ms * 1e6 / (count * K * n), ms_per_launch=ms / count, episodes=env.episode_count()))
            env.close()
    timing.emit(out)


def record(runs, args):
    """the whole document, from the children's records and the command line alone"""
    table = timing.summarise(timing.grouped(runs, lambda rec: f"{rec['family']}/{rec['form']}{rec['K'] if rec['form'] == 'rollout' else ''}/limit{rec['limit']}/{rec['lib']}"),
                             "count")
    return dict(unit="ns per env-step", window_s=args.window, repeats=args.repeats, scale=args.scale, summary=table, runs=runs)


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
    libs = {"new": (new_lib, "1")}                                           # lib: (path, with the limit cases)
    if args.base:
        libs = {"base": (os.path.abspath(args.base), "0"), **libs}
    # alternating: base, new, base, new, ...; one process holds one build of the library
    runs = timing.run_children(lambda tag, rep: [os.path.abspath(__file__), "--worker", *libs[tag], str(rep % 2), "--window", str(args.window), "--scale", str(args.scale)],
                               list(libs), args.repeats, 900, fields=lambda tag, rep, position: dict(lib=tag, repeat=rep, limit_handle_first=bool(rep % 2)))
    doc = record(runs, args)
    timing.write_json(args.out, doc)
    for k, v in doc["summary"].items():
        print(f"{k:62s} median {v['median']:.4f}  min {v['min']:.4f}  max {v['max']:.4f}  spread {100 * v['spread']:.2f} %")


if __name__ == "__main__":
    main()
