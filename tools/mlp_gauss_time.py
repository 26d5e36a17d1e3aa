#!/usr/bin/env python3
"""What the Gaussian draw costs inside the continuous families' rollouts (mgym_rollout_mlp_gauss), beside the identity head of the same build and the torch
loop it replaces:

    python tools/mlp_gauss_time.py --repeats 5 --out profiles/mlp_gauss_time.json

MountainCarContinuous and Pendulum (max_episode_steps = 200, gymnasium's registration) at 1 048 576 envs, K = 16, fused auto-reset on; the timing is
tools/timing.py's (a warm-up and a probe of 5 launches each, a fresh process per family and repeat).  Per family, H in {32, 64} and activation, ns per
env-step of
    gauss/H../..   mgym_rollout_mlp_gauss with sigma = 0.5, one call per K steps with a new call word each, actions not stored
    mlp/H../..     mgym_rollout_mlp (the score itself as the action) of this build, in the same process: gauss - mlp is the cost of the draw
    torch/H../..   the loop a trainer would run instead: TorchVecEnv with AoS observations; per step two torch.addmm, the activation,
                   mu + sigma * torch.randn, TorchVecEnv.step"""
import argparse
import os
import sys

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = [("mountain_car_continuous", 1 << 20), ("pendulum", 1 << 20)]
IN_SCALE = {"mountain_car_continuous": (2.0, 40.0), "pendulum": (1.0, 1.0, 0.3)}
LIMIT = {"mountain_car_continuous": 0, "pendulum": 200}
SIGMA = 0.5


def worker(family, n, window, rotate, K):
    sys.path.insert(0, ROOT)
    import numpy as np
    import modurl_gym_amd as mg
    kind = {"mountain_car_continuous": mg.MOUNTAINCAR_CONT, "pendulum": mg.PENDULUM}[family]
    kw = dict(max_episode_steps=LIMIT[family])
    D = mg.get_spec(kind).obs_dim

    def fused(call):
        env = mg.VecEnv(kind, n, seed=7, auto_reset=True, **kw)
        rew, done, trunc = mg.DeviceArray((K, n), np.float32), mg.DeviceArray((K, n), np.uint8), mg.DeviceArray((K, n), np.uint8)
        env.reset_device()
        env.sync()
        calls = [0]

        def launch():
            call(env, calls[0], rew, done, trunc)
            calls[0] += 1

        out = timing.window_of(timing.engine_timed(env, launch), window, 5, 5)
        env.close()
        return out

    def torch_loop(H, act):
        env = mg.TorchVecEnv(kind, n, seed=7, auto_reset=True, obs_layout="aos", **kw)
        timed = timing.torch_policy_timed(env, timing.mlp_weights(D, 1, H, IN_SCALE[family]), act, timing.torch_heads(SIGMA)["gauss"], K)
        return timing.window_of(timed, window, 5, 5)

    cases = []
    for H in (32, 64):
        for act in ("relu", "tanh"):
            w = timing.mlp_weights(D, 1, H, IN_SCALE[family])
            pol = np.concatenate([w[0].ravel(), w[1], w[2].ravel(), w[3]])   # nn.Linear order: W1[H][D], b1[H], W2[1][H], b2[1]
            cases.append((f"gauss/H{H}/{act}", lambda pol=pol, H=H, act=act: fused(lambda env, c, r, d, t: env.rollout_mlp_gauss_device(pol, H, act, SIGMA, 9, c, K, None, None, r, d, t))))
            cases.append((f"mlp/H{H}/{act}", lambda pol=pol, H=H, act=act: fused(lambda env, c, r, d, t: env.rollout_mlp_device(pol, H, act, K, None, None, r, d, t))))
            cases.append((f"torch/H{H}/{act}", lambda H=H, act=act: torch_loop(H, act)))
    out = []
    for name, run in timing.rotated(cases, rotate):
        ms, count = run()
        out.append(dict(family=family, n_envs=n, K=K, case=name, launches=count, window_ms=ms, ns_per_env_step=ms * 1e6 / (count * K * n)))
    timing.emit(out)


def populations(args):
    return {f: timing.scaled(n, args.scale) for f, n in FAMILIES if f in args.families.split(",")}


def record(runs, args):
    """(head, table) of the record, from the children's records and the command line alone"""
    table = timing.summarise(timing.grouped(runs, lambda rec: f"{rec['family']}/{rec['case']}"), "list")
    sizes = populations(args)
    head = dict(unit="ns per env-step", K=args.K, window_s=args.window, repeats=args.repeats, scale=args.scale, sigma=SIGMA, n_envs=sizes,
                max_episode_steps={f: LIMIT[f] for f in sizes},
                cases="gauss: mgym_rollout_mlp_gauss; mlp: mgym_rollout_mlp (identity head) of the same build; torch: addmm, activation, addmm, mu + sigma * randn, step")
    return head, table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of timed work per case")
    ap.add_argument("--scale", type=float, default=1.0, help="population scale (smoke runs)")
    ap.add_argument("--out", required=True, help="record file (the committed record of the full run: profiles/mlp_gauss_time.json)")
    ap.add_argument("--K", type=int, default=16, help="steps per rollout call")
    ap.add_argument("--families", default=",".join(f for f, _ in FAMILIES), help="comma-separated subset of the families")
    ap.add_argument("--worker", nargs=3, metavar=("FAMILY", "N", "ROTATE"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker[0], int(args.worker[1]), args.window, int(args.worker[2]), args.K)
    sizes = populations(args)
    runs = timing.run_children(lambda family, rep: [os.path.abspath(__file__), "--worker", family, str(sizes[family]), str(5 * rep), "--window", str(args.window),
                                                    "--K", str(args.K), "--out", args.out], list(sizes), args.repeats, 600)
    head, table = record(runs, args)
    timing.write_record(args.out, head, table)
    for k, v in table.items():
        print(f"{k:44s} median {v['median']:.4f}  min {v['min']:.4f}  max {v['max']:.4f}  spread {100 * v['spread']:.2f} %  {v['env_steps_per_s']:.3e} env-steps/s")


if __name__ == "__main__":
    main()
