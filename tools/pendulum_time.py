#!/usr/bin/env python3
"""Pendulum-v1 beside MountainCarContinuous, the continuous-action family already in the tree, in the same process with the same timing method:

    python tools/pendulum_time.py --repeats 5 --out profiles/pendulum_time.json

Both families at 1 048 576 envs, fused auto-reset on, max_episode_steps = 200 (gymnasium's limit for both ids; Pendulum's only episode boundary); the timing
is tools/timing.py's (the handle's timer, a warm-up of 30 launches and a probe of 20, a fresh process per repeat).  Per family
    step         mgym_step from a ring of 64 rows of uniform random actions; obs_out NULL (the engine's columns are the observation), reward / done / truncated written
    rollout16    mgym_rollout, K = 16, the same ring, obs_out NULL
    mlp16        mgym_rollout_mlp, K = 16, 32 ReLU units, actions_out and obs_out NULL
The record holds, per case, ns per env-step (median / min / max / spread over the repeats), env-steps/s, the ALGORITHMIC bytes per env-step — what the
call must move, counted from its arguments below, not a counter reading — and that traffic at the median rate as a fraction of 8 TB/s.  It is a whole-call
rate over peak bandwidth, not a kernel's share of peak; mlp16 is bound by the policy's arithmetic, its fraction is given for completeness."""
import argparse
import os
import sys

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_BYTES_PER_S = 8e12
N, K, RING, LIMIT, HIDDEN = 1 << 20, 16, 64, 200, 32
# state words read + written per launch (the elapsed count included: 2 B each way), obs_dim
STATE = {"mountain_car_continuous": dict(read=8 + 2, write=8 + 2), "pendulum": dict(read=12 + 2, write=16 + 2)}   # step: Pendulum reads th, thdot, sin; writes cos, sin, thdot, th
ROLL_STATE = {"mountain_car_continuous": dict(read=8 + 2, write=8 + 2), "pendulum": dict(read=16 + 2, write=16 + 2)}  # a rollout loads all four Pendulum columns


def algorithmic_bytes(family, case):
    """bytes per env-step the call must move: per step action 4 R (not mlp16), reward 4 W, done 1 W, truncated 1 W; the state once per launch"""
    if case == "step":
        return STATE[family]["read"] + STATE[family]["write"] + 4 + 6
    per_launch = ROLL_STATE[family]["read"] + ROLL_STATE[family]["write"]
    return per_launch / K + (4 if case == "rollout16" else 0) + 6


def worker(window, rotate, scale):
    sys.path.insert(0, ROOT)
    import numpy as np
    import modurl_gym_amd as mg
    n = timing.scaled(N, scale)
    kinds = {"mountain_car_continuous": mg.MOUNTAINCAR_CONT, "pendulum": mg.PENDULUM}
    scale_a = {"mountain_car_continuous": 1.0, "pendulum": 2.0}
    cases = [(f, c) for f in kinds for c in ("step", "rollout16", "mlp16")]
    out = []
    for family, case in timing.rotated(cases, rotate):
        rng = np.random.default_rng(1)
        env = mg.VecEnv(kinds[family], n, seed=7, auto_reset=True, max_episode_steps=LIMIT)
        d_act = mg.DeviceArray.from_numpy(((rng.random((RING, n), np.float32) * 2 - 1) * scale_a[family]).astype(np.float32))
        k = 1 if case == "step" else K
        d_rew, d_done, d_trunc = mg.DeviceArray((k, n), np.float32), mg.DeviceArray((k, n), np.uint8), mg.DeviceArray((k, n), np.uint8)
        turn = [0]

        def next_actions():
            p = d_act.ptr + (turn[0] % (RING // k)) * k * n * 4
            turn[0] += 1
            return p

        if case == "step":
            launch = lambda: env.step_device(next_actions(), None, d_rew, d_done, d_trunc)
        elif case == "rollout16":
            launch = lambda: env.rollout_device(next_actions(), K, None, d_rew, d_done, d_trunc)
        else:
            D, A = env.mlp_dims()
            pol, H = env.pack_mlp(*timing.mlp_weights(D, A, HIDDEN))
            launch = lambda: env.rollout_mlp_device(pol, H, "relu", K, None, None, d_rew, d_done, d_trunc)
        env.reset_device()
        env.sync()

        ms, count = timing.window_of(timing.engine_timed(env, launch), window, 30, 20)
        out.append(dict(family=family, case=case, n_envs=n, K=k, launches=count, window_ms=ms, ns_per_env_step=ms * 1e6 / (count * k * n), episodes=env.episode_count()))
        env.close()
    timing.emit(out)


def record(runs, args):
    """the whole document, from the children's records and the command line alone"""
    table = timing.summarise(timing.grouped(runs, lambda rec: f"{rec['family']}/{rec['case']}"), "count")
    for key, row in table.items():
        b = algorithmic_bytes(*key.split("/"))
        row.update(env_steps_per_s=1e9 / row["median"], algorithmic_bytes_per_env_step=b, fraction_of_8TBps=b * 1e9 / row["median"] / PEAK_BYTES_PER_S)
    return dict(unit="ns per env-step", n_envs=timing.scaled(N, args.scale), K=K, hidden=HIDDEN, max_episode_steps=LIMIT, window_s=args.window,
                repeats=args.repeats, scale=args.scale, peak_bytes_per_s=PEAK_BYTES_PER_S,
                note="whole-call rates (HIP events round the launches of a window); the bytes are algorithmic, counted from the arguments; spread = (max - min) / median",
                summary=table, runs=runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0, help="seconds of timed launches per case")
    ap.add_argument("--scale", type=float, default=1.0, help="population scale (smoke runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pendulum_time.json"))
    ap.add_argument("--worker", nargs=1, metavar="ROTATE")
    args = ap.parse_args()
    if args.worker:
        return worker(args.window, int(args.worker[0]), args.scale)
    # both families in one child
    runs = timing.run_children(lambda _, rep: [os.path.abspath(__file__), "--worker", str(rep), "--window", str(args.window), "--scale", str(args.scale)],
                               [None], args.repeats, 900)
    doc = record(runs, args)
    timing.write_json(args.out, doc)
    for k_, v in doc["summary"].items():
        print(f"{k_:40s} median {v['median']:.5f} ns  spread {100 * v['spread']:.2f} %  {v['env_steps_per_s']:.3e} env-steps/s  {v['algorithmic_bytes_per_env_step']:.2f} B  "
              f"{100 * v['fraction_of_8TBps']:.1f} % of 8 TB/s")


if __name__ == "__main__":
    main()
