#!/usr/bin/env python3
"""What the final-observation channel (mgym_set_final_obs_out) costs: the parent commit's libmgym.so, this tree's with the channel unset, and this
tree's with the channel set, in the same run, fresh processes, the order rotating.

    python tools/final_obs_time.py --base path/to/parent/libmgym.so --repeats 5 --out profiles/final_obs_time.json

Cases, all at 1 048 576 envs with fused auto-reset (the timing is tools/timing.py's: the handle's timer, a warm-up of 30 launches and a probe of 20, a
fresh process per row and repeat):
    cartpole/step            mgym_step, a ring of 64 rows of uniform random actions
    cartpole/uniform16       mgym_rollout_uniform, K = 16
    mountain_car/uniform16   mgym_rollout_uniform, K = 16, max_episode_steps = 200
    pendulum/gauss16         mgym_rollout_mlp_gauss, K = 16, max_episode_steps = 200, 32 ReLU units, sigma = 0.5
Rows per case: `parent` (--base), `unset`, `set`.  A channel-unset handle launches the parent's kernels, so its row is expected within the spread of
the parent's own repeats, (max - min) / median; the channel-set row is recorded with the share of env-steps that finished in its window and the bytes
the channel wrote per env-step (4 obs_dim per finished env-step; at most 32 obs_dim where every 4-byte store dirties a 32-byte sector of its own).
One JSON document: every repeat, and per case and row median, min, max and spread."""
import argparse
import os
import sys

import timing

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
    n = timing.scaled(1 << 20, scale)
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

        timed = timing.engine_timed(env, launch)
        count = timing.calibrate(timed, window, 30, 20)
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
    timing.emit(out)


def record(runs, args):
    """the whole document, from the children's records and the command line alone"""
    tags = [tag for tag in ("parent", "unset", "set") if any(r["row"] == tag for r in runs)]
    summary = {}
    for case in CASES:
        per_row = {}
        for tag in tags:
            recs = [r for r in runs if r["case"] == case and r["row"] == tag]
            per_row[tag] = timing.stats([r["ns_per_env_step"] for r in recs], "count")
            for field in ("finished_share", "final_bytes_per_env_step", "final_sector_bytes_per_env_step_max"):
                per_row[tag][field] = timing.median(r[field] for r in recs)
        ref = per_row.get("parent", per_row["unset"])
        for tag in per_row:
            per_row[tag]["vs_" + ("parent" if "parent" in per_row else "unset")] = per_row[tag]["median"] / ref["median"] - 1.0
        if "parent" in per_row:
            per_row["unset_within_parent_spread"] = abs(per_row["unset"]["median"] - ref["median"]) <= ref["max"] - ref["min"]
        summary[case] = per_row
    return dict(unit="ns per env-step", window_s=args.window, repeats=args.repeats, scale=args.scale, hidden=HIDDEN, summary=summary, runs=runs)


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
    rows = {"unset": (new_lib, "0"), "set": (new_lib, "1")}                  # row: (library, channel set)
    if args.base:
        rows = {"parent": (os.path.abspath(args.base), "0"), **rows}
    # one process holds one build of the library; the order of the rows rotates from repeat to repeat
    runs = timing.run_children(lambda tag, rep: [os.path.abspath(__file__), "--worker", *rows[tag], "--window", str(args.window), "--scale", str(args.scale)],
                               lambda rep: timing.rotated(list(rows), rep), args.repeats, 600,
                               fields=lambda tag, rep, position: dict(row=tag, repeat=rep, position=position))
    doc = record(runs, args)
    timing.write_json(args.out, doc)
    for case, per_row in doc["summary"].items():
        for tag, v in per_row.items():
            if isinstance(v, dict):
                print(f"{case:24s} {tag:7s} median {v['median']:.4f}  min {v['min']:.4f}  max {v['max']:.4f}  spread {100 * v['spread']:.2f} %  finished {100 * v['finished_share']:.2f} %")
        if "unset_within_parent_spread" in per_row:
            print(f"{case:24s} unset within the parent's spread: {per_row['unset_within_parent_spread']}")


if __name__ == "__main__":
    main()
