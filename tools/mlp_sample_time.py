#!/usr/bin/env python3
"""What the softmax draw costs inside the rollouts (mgym_rollout_mlp_sample), beside the argmax form of the same build and the torch loop it replaces:

    python tools/mlp_sample_time.py --repeats 5 --out profiles/mlp_sample_time.json

CartPole and MountainCar at 1 048 576 envs, LunarLander with wind at 262 144, K = 16, fused auto-reset on; the timing is tools/timing.py's (a warm-up and a
probe of 5 launches each, a fresh process per family and repeat).  Per family, H in {32, 64} and activation, ns per env-step of
    sample/H../..  mgym_rollout_mlp_sample, one call per K steps with a new call word each, actions not stored
    mlp/H../..     mgym_rollout_mlp (argmax) of this build: sample - mlp is the cost of the draw, and these rows against profiles/mlp_policy_time.json show
                   that the existing path has not moved
    torch/H../..   the loop a trainer would run instead: TorchVecEnv with AoS observations; per step two torch.addmm, the activation,
                   torch.multinomial over torch.softmax, TorchVecEnv.step"""
import argparse
import os
import sys

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = [("cartpole", 1 << 20), ("mountain_car", 1 << 20), ("lunar_lander", 1 << 18)]
IN_SCALE = {"cartpole": (2.0, 1.0, 8.0, 1.0), "mountain_car": (2.0, 40.0), "lunar_lander": (2.0, 2.0, 2.0, 2.0, 3.0, 2.0, 2.0, 2.0)}


def worker(family, n, window, rotate, K):
    sys.path.insert(0, ROOT)
    import numpy as np
    import modurl_gym_amd as mg
    kind = {"cartpole": mg.CARTPOLE, "mountain_car": mg.MOUNTAINCAR, "lunar_lander": mg.LUNARLANDER}[family]
    kw = dict(enable_wind=True) if family == "lunar_lander" else {}
    spec = mg.get_spec(kind)
    D, A = spec.obs_dim, spec.n_actions

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
        timed = timing.torch_policy_timed(env, timing.mlp_weights(D, A, H, IN_SCALE[family]), act, timing.torch_heads()["sample"], K)
        return timing.window_of(timed, window, 5, 5)

    cases = []
    for H in (32, 64):
        for act in ("relu", "tanh"):
            w = timing.mlp_weights(D, A, H, IN_SCALE[family])
            pol = np.concatenate([w[0].ravel(), w[1], w[2].ravel(), w[3]])   # nn.Linear order: W1[H][D], b1[H], W2[A][H], b2[A]
            cases.append((f"sample/H{H}/{act}", lambda pol=pol, H=H, act=act: fused(lambda env, c, r, d, t: env.rollout_mlp_sample_device(pol, H, act, 9, c, K, None, None, r, d, t))))
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
    head = dict(unit="ns per env-step", K=args.K, window_s=args.window, repeats=args.repeats, scale=args.scale, n_envs=populations(args),
                cases="sample: mgym_rollout_mlp_sample; mlp: mgym_rollout_mlp (argmax) of the same build; torch: addmm, activation, addmm, softmax, multinomial, step")
    return head, table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of timed work per case")
    ap.add_argument("--scale", type=float, default=1.0, help="population scale (smoke runs)")
    ap.add_argument("--out", required=True, help="record file (a full run's would be profiles/mlp_sample_time.json: none has been taken)")
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
        print(f"{k:34s} median {v['median']:.4f}  min {v['min']:.4f}  max {v['max']:.4f}  spread {100 * v['spread']:.2f} %  {v['env_steps_per_s']:.3e} env-steps/s")


if __name__ == "__main__":
    main()
