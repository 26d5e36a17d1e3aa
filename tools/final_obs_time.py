#!/usr/bin/env python3
"""What the final-observation channel (mgym_set_final_obs_out) costs: the parent commit's libmgym.so, this tree's with the channel unset, and this
tree's with the channel set, in the same run, fresh processes, the order rotating.

    python tools/final_obs_time.py --base path/to/parent/libmgym.so --repeats 5 --out profiles/final_obs_time.json

Cases, all at 1 048 576 envs with fused auto-reset (HIP-event timing on the handle's stream as bench.py does, a warm-up, windows of at least
--window seconds):
    cartpole/step            mgym_step, a ring of 64 rows of uniform random actions
    cartpole/uniform16       mgym_rollout_uniform, K = 16
    mountain_car/uniform16   mgym_rollout_uniform, K = 16, max_episode_steps = 200
    pendulum/gauss16         mgym_rollout_mlp_gauss, K = 16, max_episode_steps = 200, 32 ReLU units, sigma = 0.5
Rows per case: `parent` (--base), `unset`, `set`.  A channel-unset handle launches the parent's kernels, so its row is expected within the spread of
the parent's own repeats, (max - min) / median; the channel-set row is recorded with the share of env-steps that finished in its window and the bytes
the channel wrote per env-step (4 obs_dim per finished env-step; at most 32 obs_dim where every 4-byte store dirties a 32-byte sector of its own).
One JSON document: every repeat, and per case and row median, min, max and spread."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RING, K, HIDDEN = 64, 16, 32
CASES = ["cartpole/step", "cartpole/uniform16", "mountain_car/uniform16", "pendulum/gauss16"]


def worker(lib_path, with_channel, window, scale):
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
        del _lib.PROTOTYPES[name]           # a base library from before mgym_set_final_obs_out
    import modurl_gym_amd as mg
    rng = np.random.default_rng(1)
    n = max(1024, int((1 << 20) * scale)) // 1024 * 1024
    out = []
    for case in CASES:
        family, form = case.split("/")
        kind = {"cartpole": mg.CARTPOLE, "mountain_car": mg.MOUNTAINCAR, "pendulum": mg.PENDULUM}[family]
        env = mg.VecEnv(kind, n, seed=7, auto_reset=True, max_episode_steps=0 if family == "cartpole" else 200)
        k = 1 if form == "step" else K
        d_act = mg.DeviceArray.from_numpy(rng.integers(0, 2, (RING, n)).astype(np.uint32)) if form == "step" else mg.DeviceArray((k, n), np.uint32)
        d_obs = mg.DeviceArray((k, env.obs_dim, n), np.float32)
        d_rew, d_done, d_trunc = mg.DeviceArray((k, n), np.float32), mg.DeviceArray((k, n), np.uint8), mg.DeviceArray((k, n), np.uint8)
        d_fin = None
        if with_channel:
            d_fin = mg.DeviceArray((k, env.obs_dim, n), np.float32)
            env.set_final_obs_out_device(d_fin, k)
        turn = [0]
        if form == "step":
            def launch():
                env.step_device(d_act.ptr + (turn[0] % RING) * n * 4, d_obs, d_rew, d_done, d_trunc)
                turn[0] += 1
        elif form == "uniform16":
            launch = lambda: env.rollout_uniform_device(11, k, d_act, d_obs, d_rew, d_done, d_trunc)
        else:
            D, A = env.mlp_dims()
            pol, _ = env.pack_mlp(rng.normal(0, 0.5, (HIDDEN, D)), rng.normal(0, 0.5, HIDDEN), rng.normal(0, 0.5, (A, HIDDEN)), rng.normal(0, 0.5, A))

            def launch():
                env.rollout_mlp_gauss_device(pol, HIDDEN, "relu", 0.5, 11, turn[0], k, d_act, d_obs, d_rew, d_done, d_trunc)
                turn[0] += 1
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
        before = env.episode_count()
        ms = timed(count)
        finished = env.episode_count() - before
        env_steps = count * k * n
        out.append(dict(case=case, n_envs=n, K=k, launches=count, window_ms=ms, ns_per_env_step=ms * 1e6 / env_steps, ms_per_launch=ms / count,
                        finished_share=finished / env_steps, final_bytes_per_env_step=4 * env.obs_dim * finished / env_steps if with_channel else 0.0,
                        final_sector_bytes_per_env_step_max=32 * env.obs_dim * finished / env_steps if with_channel else 0.0))
        if with_channel:
            env.set_final_obs_out_device(None)
        env.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", required=False, help="the parent commit's build of libmgym.so")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of timed launches per case")
    ap.add_argument("--scale", type=float, default=1.0, help="population scale (smoke runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "final_obs_time.json"))
    ap.add_argument("--worker", nargs=2, metavar=("LIB", "WITH_CHANNEL"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker[0], args.worker[1] == "1", args.window, args.scale)
    new_lib = os.path.join(ROOT, "modurl_gym_amd", "libmgym.so")
    rows = ([("parent", os.path.abspath(args.base), "0")] if args.base else []) + [("unset", new_lib, "0"), ("set", new_lib, "1")]
    runs = []
    for rep in range(args.repeats):
        order = rows[rep % len(rows):] + rows[:rep % len(rows)]   # the order rotates from repeat to repeat
        for tag, path, with_channel in order:
            # a fresh child per row and repeat: one process holds one build of the library, and the parent never opens the GPU
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", path, with_channel, "--window", str(args.window), "--scale", str(args.scale)],
                               capture_output=True, text=True, timeout=600)
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
                raise SystemExit(f"worker {tag} repeat {rep} failed with status {r.returncode}")   # nothing more is started on the GPU
            for rec in json.loads(line[0][7:]):
                runs.append(dict(rec, row=tag, repeat=rep, position=[t for t, _, _ in order].index(tag)))
            print(f"repeat {rep} {tag}: done", flush=True)
    summary = {}
    for case in CASES:
        per_row = {}
        for tag, _, _ in rows:
            recs = [r for r in runs if r["case"] == case and r["row"] == tag]
            v = [r["ns_per_env_step"] for r in recs]
            med = statistics.median(v)
            per_row[tag] = dict(median=med, min=min(v), max=max(v), spread=(max(v) - min(v)) / med, repeats=len(v),
                                finished_share=statistics.median(r["finished_share"] for r in recs),
                                final_bytes_per_env_step=statistics.median(r["final_bytes_per_env_step"] for r in recs),
                                final_sector_bytes_per_env_step_max=statistics.median(r["final_sector_bytes_per_env_step_max"] for r in recs))
        ref = per_row.get("parent", per_row["unset"])
        for tag in per_row:
            per_row[tag]["vs_" + ("parent" if "parent" in per_row else "unset")] = per_row[tag]["median"] / ref["median"] - 1.0
        if "parent" in per_row:
            per_row["unset_within_parent_spread"] = abs(per_row["unset"]["median"] - ref["median"]) <= ref["max"] - ref["min"]
        summary[case] = per_row
    doc = dict(unit="ns per env-step", window_s=args.window, repeats=args.repeats, scale=args.scale, hidden=HIDDEN, summary=summary, runs=runs)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for case, per_row in summary.items():
        for tag, v in per_row.items():
            if isinstance(v, dict):
                print(f"{case:24s} {tag:7s} median {v['median']:.4f}  min {v['min']:.4f}  max {v['max']:.4f}  spread {100 * v['spread']:.2f} %  finished {100 * v['finished_share']:.2f} %")
        if "unset_within_parent_spread" in per_row:
            print(f"{case:24s} unset within the parent's spread: {per_row['unset_within_parent_spread']}")


if __name__ == "__main__":
    main()
