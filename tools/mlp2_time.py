#!/usr/bin/env python3
"""What the second hidden layer costs inside the policy rollouts: mgym_rollout_mlp2 beside the one-hidden-layer call of the same build and beside the torch loop
it replaces:

    python tools/mlp2_time.py --repeats 5 --out profiles/mlp2_time.json

K = 16, fused auto-reset on; the timing is tools/timing.py's (a warm-up and a probe of 3 launches each, a fresh process per repeat with every case in it).
Rows: CartPole with the greedy and the sampling head, Pendulum (max_episode_steps = 200) with the Gaussian head; 1 048 576 and 4 096 envs; widths (32, 32) and
(64, 64); ReLU and tanh_fast.  Columns, ns per env-step, all in one process:
    mlp2    mgym_rollout_mlp2, one call per K steps (a new call word each where the head draws), actions not stored
    mlp1    the one-hidden-layer call with the same head at H = H1, for scale
    torch   the loop a trainer would run instead: TorchVecEnv with AoS observations; per step three torch.addmm with torch.relu / torch.tanh between them,
            then argmax / torch.multinomial of the softmax / mu + sigma * torch.randn, then TorchVecEnv.step
Not measured here: hardware counters, other sizes or K, LunarLander, a training loop."""
import argparse
import os
import sys

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ENVS = (1 << 20, 4096)
ROWS = [("cartpole", "greedy"), ("cartpole", "sample"), ("pendulum", "gauss")]
IN_SCALE = {"cartpole": (1.0, 1.0, 8.0, 1.0), "pendulum": (1.0, 1.0, 0.3)}
LIMIT = {"cartpole": 0, "pendulum": 200}
ACTIVATIONS = ("relu", "tanh_fast")
WIDTHS = (32, 64)
SIGMA = 0.5


def worker(scale, window, rotate, K, lib):
    sys.path.insert(0, ROOT)
    import numpy as np
    if lib:
        from modurl_gym_amd import _lib
        _lib.LIB_PATH = os.path.abspath(lib)   # before anything loads the library
    import modurl_gym_amd as mg
    kinds = {"cartpole": mg.CARTPOLE, "pendulum": mg.PENDULUM}

    def weights(family, H):
        D, A = mg.get_spec(kinds[family]).obs_dim, 2 if family == "cartpole" else 1
        rng = np.random.default_rng(100 + H)
        return ((rng.normal(0, 1, (H, D)) * np.array(IN_SCALE[family])).astype(np.float32), rng.normal(0, 0.5, H).astype(np.float32),
                (rng.normal(0, 1, (H, H)) / np.sqrt(H)).astype(np.float32), rng.normal(0, 0.5, H).astype(np.float32),
                (rng.normal(0, 1, (A, H)) / np.sqrt(H)).astype(np.float32), rng.normal(0, 0.1, A).astype(np.float32))

    def fused(family, head, n, H, act, layers):
        w = weights(family, H)
        env = mg.VecEnv(kinds[family], n, seed=7, auto_reset=True, max_episode_steps=LIMIT[family])
        pol2 = env.pack_mlp2(*w)[0]
        pol1 = env.pack_mlp(w[0], w[1], w[4], w[5])[0]
        rew, done, trunc = mg.DeviceArray((K, n), np.float32), mg.DeviceArray((K, n), np.uint8), mg.DeviceArray((K, n), np.uint8)
        env.reset_device()
        env.sync()
        calls = [0]

        def launch():
            if layers == 2:
                env.rollout_mlp2_device(pol2, H, H, act, head, SIGMA, 9, calls[0], K, None, None, rew, done, trunc)
            elif head == "greedy":
                env.rollout_mlp_device(pol1, H, act, K, None, None, rew, done, trunc)
            elif head == "sample":
                env.rollout_mlp_sample_device(pol1, H, act, 9, calls[0], K, None, None, rew, done, trunc)
            else:
                env.rollout_mlp_gauss_device(pol1, H, act, SIGMA, 9, calls[0], K, None, None, rew, done, trunc)
            calls[0] += 1

        out = timing.window_of(timing.engine_timed(env, launch), window, 3, 3)
        env.close()
        return out

    def torch_loop(family, head, n, H, act):
        env = mg.TorchVecEnv(kinds[family], n, seed=7, auto_reset=True, obs_layout="aos", max_episode_steps=LIMIT[family])
        return timing.window_of(timing.torch_policy_timed(env, weights(family, H), act, timing.torch_heads(SIGMA)[head], K), window, 3, 3)

    cases = []
    for family, head in ROWS:
        for n0 in N_ENVS:
            n = timing.scaled(n0, scale)
            for H in WIDTHS:
                for act in ACTIVATIONS:
                    name = f"{head}/n{n}/{H}x{H}/{act}"
                    cases.append((family, n, name + "/mlp2", lambda f=family, h=head, n=n, H=H, a=act: fused(f, h, n, H, a, 2)))
                    cases.append((family, n, name + "/mlp1", lambda f=family, h=head, n=n, H=H, a=act: fused(f, h, n, H, a, 1)))
                    cases.append((family, n, name + "/torch", lambda f=family, h=head, n=n, H=H, a=act: torch_loop(f, h, n, H, a)))
    out = []
    for family, n, name, run in timing.rotated(cases, rotate):
        ms, count = run()
        out.append(dict(family=family, n_envs=n, K=K, case=name, launches=count, window_ms=ms, ns_per_env_step=ms * 1e6 / (count * K * n)))
    timing.emit(out)


def record(runs, args):
    """(head, table) of the record, from the children's records and the command line alone"""
    table = timing.summarise(timing.grouped(runs, lambda rec: f"{rec['family']}/{rec['case']}"), "list")
    # each mlp2 row against the one-layer call and the torch loop of the same run
    ratios = {}
    for k, v in table.items():
        if k.endswith("/mlp2"):
            base = k[: -len("mlp2")]
            ratios[k] = dict(torch_over_mlp2=table[base + "torch"]["median"] / v["median"], mlp2_over_mlp1=v["median"] / table[base + "mlp1"]["median"])
    head = dict(unit="ns per env-step", K=args.K, window_s=args.window, repeats=args.repeats, scale=args.scale, sigma=SIGMA, n_envs=list(N_ENVS),
                max_episode_steps=LIMIT, lib=os.path.basename(args.lib) if args.lib else "the package's",
                cases="mlp2: mgym_rollout_mlp2; mlp1: the one-hidden-layer call with the same head at H = H1; torch: three addmm, two activations (torch.relu / torch.tanh), "
                "argmax | multinomial(softmax) | mu + sigma * randn, step; all of a repeat in one process",
                static_bound="157 TF / (2 x 4096 flop) = 1.9e10 env-steps/s at (64, 64)",
                not_measured="hardware counters, other sizes or K, LunarLander, a training loop", ratios=ratios)
    return head, table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of timed work per case")
    ap.add_argument("--scale", type=float, default=1.0, help="population scale (smoke runs)")
    ap.add_argument("--out", required=True, help="record file (the committed record of the full run: profiles/mlp2_time.json)")
    ap.add_argument("--K", type=int, default=16, help="steps per rollout call")
    ap.add_argument("--lib", default="", help="time this build of libmgym.so instead of the package's (an A/B of two builds on one machine)")
    ap.add_argument("--worker", nargs=2, metavar=("SCALE", "ROTATE"))
    args = ap.parse_args()
    if args.worker:
        return worker(float(args.worker[0]), args.window, int(args.worker[1]), args.K, args.lib)
    runs = timing.run_children(lambda _, rep: [os.path.abspath(__file__), "--worker", str(args.scale), str(7 * rep), "--window", str(args.window), "--K", str(args.K),
                                               "--out", args.out, "--lib", args.lib], [None], args.repeats, 900)
    head, table = record(runs, args)
    timing.write_record(args.out, head, table)
    for k, v in table.items():
        print(f"{k:52s} median {v['median']:.4f}  min {v['min']:.4f}  max {v['max']:.4f}  spread {100 * v['spread']:.2f} %  {v['env_steps_per_s']:.3e} env-steps/s")
    for k, v in head["ratios"].items():
        print(f"{k:52s} torch / mlp2 {v['torch_over_mlp2']:.2f}  mlp2 / mlp1 {v['mlp2_over_mlp1']:.2f}")


if __name__ == "__main__":
    main()
