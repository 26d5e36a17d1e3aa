#!/usr/bin/env python3
"""What the hidden activation costs inside the hidden-layer policy rollouts: MGYM_ACT_TANH_FAST beside ReLU and the glibc-exact tanh of the same build, and
beside the torch loop (torch.tanh) the rollout replaces:

    python tools/tanh_fast_time.py --repeats 5 --out profiles/tanh_fast_time.json

1 048 576 envs, K = 16, fused auto-reset on; the timing is tools/timing.py's (a warm-up and a probe of 5 launches each, a fresh process per repeat with every
case in it).  Rows: CartPole through mgym_rollout_mlp and mgym_rollout_mlp_sample, MountainCarContinuous and Pendulum (max_episode_steps = 200, gymnasium's
registration) through mgym_rollout_mlp_gauss, each with 32 and 64 hidden units.  Columns, ns per env-step, all in one process:
    relu, tanh, tanh_fast   the fused rollout, one call per K steps (a new call word each where the entry point draws), actions not stored
    torch                   the loop a trainer would run instead: TorchVecEnv with AoS observations; per step two torch.addmm with torch.tanh between them,
                            then argmax / torch.multinomial of the softmax / mu + sigma * torch.randn, then TorchVecEnv.step
Not measured here: hardware counters, other populations or K, LunarLander, a training loop."""
import argparse
import os
import sys

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ENVS = 1 << 20
ROWS = [("cartpole", "mlp"), ("cartpole", "sample"), ("mountain_car_continuous", "gauss"), ("pendulum", "gauss")]
IN_SCALE = {"cartpole": (1.0, 1.0, 8.0, 1.0), "mountain_car_continuous": (2.0, 40.0), "pendulum": (1.0, 1.0, 0.3)}
LIMIT = {"cartpole": 0, "mountain_car_continuous": 0, "pendulum": 200}
ACTIVATIONS = ("relu", "tanh", "tanh_fast")
SIGMA = 0.5
TORCH_HEAD = {"mlp": "greedy", "sample": "sample", "gauss": "gauss"}


def worker(n, window, rotate, K, lib):
    sys.path.insert(0, ROOT)
    import numpy as np
    if lib:
        from modurl_gym_amd import _lib
        _lib.LIB_PATH = os.path.abspath(lib)   # before anything loads the library
    import modurl_gym_amd as mg
    kinds = {"cartpole": mg.CARTPOLE, "mountain_car_continuous": mg.MOUNTAINCAR_CONT, "pendulum": mg.PENDULUM}

    def weights(family, H):
        return timing.mlp_weights(mg.get_spec(kinds[family]).obs_dim, 2 if family == "cartpole" else 1, H, IN_SCALE[family])

    def fused(family, entry, H, act):
        w = weights(family, H)
        pol = np.concatenate([w[0].ravel(), w[1], w[2].ravel(), w[3]])   # nn.Linear order
        env = mg.VecEnv(kinds[family], n, seed=7, auto_reset=True, max_episode_steps=LIMIT[family])
        rew, done, trunc = mg.DeviceArray((K, n), np.float32), mg.DeviceArray((K, n), np.uint8), mg.DeviceArray((K, n), np.uint8)
        env.reset_device()
        env.sync()
        calls = [0]

        def launch():
            if entry == "mlp":
                env.rollout_mlp_device(pol, H, act, K, None, None, rew, done, trunc)
            elif entry == "sample":
                env.rollout_mlp_sample_device(pol, H, act, 9, calls[0], K, None, None, rew, done, trunc)
            else:
                env.rollout_mlp_gauss_device(pol, H, act, SIGMA, 9, calls[0], K, None, None, rew, done, trunc)
            calls[0] += 1

        out = timing.window_of(timing.engine_timed(env, launch), window, 5, 5)
        env.close()
        return out

    def torch_loop(family, entry, H):
        env = mg.TorchVecEnv(kinds[family], n, seed=7, auto_reset=True, obs_layout="aos", max_episode_steps=LIMIT[family])
        timed = timing.torch_policy_timed(env, weights(family, H), "tanh", timing.torch_heads(SIGMA)[TORCH_HEAD[entry]], K)
        return timing.window_of(timed, window, 5, 5)

    cases = []
    for family, entry in ROWS:
        for H in (32, 64):
            for act in ACTIVATIONS:
                cases.append((family, f"{entry}/H{H}/{act}", lambda f=family, e=entry, H=H, a=act: fused(f, e, H, a)))
            cases.append((family, f"{entry}/H{H}/torch", lambda f=family, e=entry, H=H: torch_loop(f, e, H)))
    out = []
    for family, name, run in timing.rotated(cases, rotate):
        ms, count = run()
        out.append(dict(family=family, n_envs=n, K=K, case=name, launches=count, window_ms=ms, ns_per_env_step=ms * 1e6 / (count * K * n)))
    timing.emit(out)


def record(runs, args):
    """(head, table) of the record, from the children's records and the command line alone"""
    table = timing.summarise(timing.grouped(runs, lambda rec: f"{rec['family']}/{rec['case']}"), "list")
    # each tanh_fast row against the tanh row and the torch loop of the same run
    ratios = {}
    for k, v in table.items():
        if k.endswith("/tanh_fast"):
            base = k[: -len("tanh_fast")]
            ratios[k] = dict(tanh_over_tanh_fast=table[base + "tanh"]["median"] / v["median"], torch_over_tanh_fast=table[base + "torch"]["median"] / v["median"],
                             relu_over_tanh_fast=table[base + "relu"]["median"] / v["median"])
    head = dict(unit="ns per env-step", K=args.K, window_s=args.window, repeats=args.repeats, scale=args.scale, sigma=SIGMA, n_envs=timing.scaled(N_ENVS, args.scale),
                max_episode_steps=LIMIT, lib=os.path.basename(args.lib) if args.lib else "the package's", cases="relu / tanh / tanh_fast: the fused rollout with that hidden activation; torch: addmm, torch.tanh, addmm, "
                "argmax | multinomial(softmax) | mu + sigma * randn, step; all of a repeat in one process",
                not_measured="hardware counters, other populations or K, LunarLander, a training loop", ratios=ratios)
    return head, table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of timed work per case")
    ap.add_argument("--scale", type=float, default=1.0, help="population scale (smoke runs)")
    ap.add_argument("--out", required=True, help="record file (the committed record of the full run: profiles/tanh_fast_time.json)")
    ap.add_argument("--K", type=int, default=16, help="steps per rollout call")
    ap.add_argument("--lib", default="", help="time this build of libmgym.so instead of the package's (an A/B of two builds on one machine)")
    ap.add_argument("--worker", nargs=2, metavar=("N", "ROTATE"))
    args = ap.parse_args()
    if args.worker:
        return worker(int(args.worker[0]), args.window, int(args.worker[1]), args.K, args.lib)
    n = timing.scaled(N_ENVS, args.scale)
    runs = timing.run_children(lambda _, rep: [os.path.abspath(__file__), "--worker", str(n), str(7 * rep), "--window", str(args.window), "--K", str(args.K),
                                               "--out", args.out, "--lib", args.lib], [None], args.repeats, 600)
    head, table = record(runs, args)
    timing.write_record(args.out, head, table)
    for k, v in table.items():
        print(f"{k:52s} median {v['median']:.4f}  min {v['min']:.4f}  max {v['max']:.4f}  spread {100 * v['spread']:.2f} %  {v['env_steps_per_s']:.3e} env-steps/s")
    for k, v in head["ratios"].items():
        print(f"{k:52s} tanh / tanh_fast {v['tanh_over_tanh_fast']:.2f}  torch / tanh_fast {v['torch_over_tanh_fast']:.2f}  relu / tanh_fast {v['relu_over_tanh_fast']:.2f}")


if __name__ == "__main__":
    main()
