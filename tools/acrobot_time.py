#!/usr/bin/env python3
"""Acrobot-v1 beside CartPole, the yardstick in the tree, in the same process with the same timing method:

    python tools/acrobot_time.py --repeats 5 --out profiles/acrobot_time.json

Both families at 1 048 576 envs, fused auto-reset on, max_episode_steps = 500 (gymnasium's limit for both ids); the timing is tools/timing.py's (the
handle's timer, torch events for the torch rows, a warm-up of 2 launches and a probe of 4 — the engine rows after 20 launches more — and a fresh process
per repeat).  Per family
    step           mgym_step from a ring of 64 rows of uniform random actions; obs_out NULL (the engine's columns are the observation), reward / done / truncated written
    rollout16      mgym_rollout, K = 16, the same ring, obs_out NULL
    mlp32, mlp64   mgym_rollout_mlp, K = 16, 32 / 64 ReLU units, actions_out and obs_out NULL
    sample32       mgym_rollout_mlp_sample, K = 16, 32 ReLU units, a new call word per launch
    torch32, torch_sample32   the loop those replace: TorchVecEnv with AoS observations; per step two torch.addmm, relu, argmax (or multinomial over
                   softmax), TorchVecEnv.step
The record holds, per case, ns per env-step (median / min / max / spread over the repeats), env-steps/s and, for the engine's own rows, the ALGORITHMIC
bytes per env-step — what the call must move, counted from its arguments, not a counter reading — and that traffic at the median rate as a fraction of
8 TB/s: a whole-call rate over peak bandwidth, not a kernel's share of peak.  Acrobot's step is four derivative evaluations and eight f64 sincos
pairs per environment: which of arithmetic and traffic bounds it is read off that fraction beside CartPole's."""
import argparse
import os
import sys

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_BYTES_PER_S = 8e12
N, K, RING, LIMIT = 1 << 20, 16, 64, 500
# state bytes read + written per launch.  CartPole: 4 state columns and its step counter (the limit lives in the state); Acrobot: 8 columns and the u16 elapsed count
STATE = {"cartpole": 16 + 16 + 4 + 4, "acrobot": 32 + 32 + 2 + 2}
ENGINE_CASES = ("step", "rollout16", "mlp32", "mlp64", "sample32")


def algorithmic_bytes(family, case):
    """bytes per env-step the call must move: per step action 4 R (table sources only), reward 4 W, done 1 W, truncated 1 W; the state once per launch"""
    if case == "step":
        return STATE[family] + 4 + 6
    return STATE[family] / K + (4 if case == "rollout16" else 0) + 6


def worker(window, rotate, scale):
    sys.path.insert(0, ROOT)
    import numpy as np
    import modurl_gym_amd as mg
    n = timing.scaled(N, scale)
    kinds = {"cartpole": mg.CARTPOLE, "acrobot": mg.ACROBOT}
    n_act = {"cartpole": 2, "acrobot": 3}

    def weights(family, H):
        return timing.mlp_weights(mg.get_spec(kinds[family]).obs_dim, n_act[family], H)

    def engine(family, case):
        rng = np.random.default_rng(1)
        env = mg.VecEnv(kinds[family], n, seed=7, auto_reset=True, max_episode_steps=LIMIT)
        d_act = mg.DeviceArray.from_numpy(rng.integers(0, n_act[family], (RING, n)).astype(np.uint32))
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
            H = int(case[-2:])
            pol, H = env.pack_mlp(*weights(family, H))
            if case.startswith("sample"):
                def launch():
                    env.rollout_mlp_sample_device(pol, H, "relu", 9, turn[0], K, None, None, d_rew, d_done, d_trunc)
                    turn[0] += 1
            else:
                launch = lambda: env.rollout_mlp_device(pol, H, "relu", K, None, None, d_rew, d_done, d_trunc)
        env.reset_device()
        env.sync()

        timed = timing.engine_timed(env, launch)
        timed(20)
        ms, count = timing.window_of(timed, window, 2, 4)
        episodes = env.episode_count()
        env.close()
        return ms, count, k, episodes

    def torch_loop(family, case):
        env = mg.TorchVecEnv(kinds[family], n, seed=7, auto_reset=True, obs_layout="aos", max_episode_steps=LIMIT)
        head = timing.torch_heads()["greedy" if case == "torch32" else "sample"]
        ms, count = timing.window_of(timing.torch_policy_timed(env, weights(family, 32), "relu", head, K), window, 2, 4)
        return ms, count, K, None

    cases = [(f, c) for f in kinds for c in ENGINE_CASES + ("torch32", "torch_sample32")]
    out = []
    for family, case in timing.rotated(cases, rotate):
        ms, count, k, episodes = (torch_loop if case.startswith("torch") else engine)(family, case)
        out.append(dict(family=family, case=case, n_envs=n, K=k, launches=count, window_ms=ms, ns_per_env_step=ms * 1e6 / (count * k * n), episodes=episodes))
    timing.emit(out)


def record(runs, args):
    """the whole document, from the children's records and the command line alone"""
    table = timing.summarise(timing.grouped(runs, lambda rec: f"{rec['family']}/{rec['case']}"), "count")
    for key, row in table.items():
        family, case = key.split("/")
        row.update(env_steps_per_s=1e9 / row["median"])
        if case in ENGINE_CASES:
            b = algorithmic_bytes(family, case)
            row.update(algorithmic_bytes_per_env_step=b, fraction_of_8TBps=b * 1e9 / row["median"] / PEAK_BYTES_PER_S)
    return dict(unit="ns per env-step", n_envs=timing.scaled(N, args.scale), K=K, max_episode_steps=LIMIT, window_s=args.window,
                repeats=args.repeats, scale=args.scale, peak_bytes_per_s=PEAK_BYTES_PER_S,
                note="whole-call rates (events round the launches of a window); the bytes are algorithmic, counted from the arguments; spread = (max - min) / median",
                summary=table, runs=runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of timed work per case")
    ap.add_argument("--scale", type=float, default=1.0, help="population scale (smoke runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "acrobot_time.json"))
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
        extra = f"  {v['algorithmic_bytes_per_env_step']:.2f} B  {100 * v['fraction_of_8TBps']:.1f} % of 8 TB/s" if "fraction_of_8TBps" in v else ""
        print(f"{k_:32s} median {v['median']:.5f} ns  spread {100 * v['spread']:.2f} %  {v['env_steps_per_s']:.3e} env-steps/s{extra}")


if __name__ == "__main__":
    main()
