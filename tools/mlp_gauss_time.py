#!/usr/bin/env python3
"""What the Gaussian draw costs inside the continuous families' rollouts (mgym_rollout_mlp_gauss), beside the identity head of the same build and the torch
loop it replaces:

    python tools/mlp_gauss_time.py --repeats 5 --out profiles/mlp_gauss_time.json

The timing scheme is that of tools/mlp_sample_time.py (K = 16, fused auto-reset on, a fresh process per family and repeat, the cases of a process in an
order that rotates with the repeat, median / min / max / spread over the repeats).  MountainCarContinuous and Pendulum (max_episode_steps = 200, gymnasium's
registration) at 1 048 576 envs.  Per family, H in {32, 64} and activation, ns per env-step of
    gauss/H../..   mgym_rollout_mlp_gauss with sigma = 0.5, one call per K steps with a new call word each, actions not stored
    mlp/H../..     mgym_rollout_mlp (the score itself as the action) of this build, in the same process: gauss - mlp is the cost of the draw
    torch/H../..   the loop a trainer would run instead: TorchVecEnv with AoS observations; per step two torch.addmm, the activation,
                   mu + sigma * torch.randn, TorchVecEnv.step"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mlp_policy_time import write_record  # noqa: E402

FAMILIES = [("mountain_car_continuous", 1 << 20), ("pendulum", 1 << 20)]
IN_SCALE = {"mountain_car_continuous": (2.0, 40.0), "pendulum": (1.0, 1.0, 0.3)}
LIMIT = {"mountain_car_continuous": 0, "pendulum": 200}
SIGMA = 0.5


def worker(family, n, window, rotate, K):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import modurl_gym_amd as mg
    kind = {"mountain_car_continuous": mg.MOUNTAINCAR_CONT, "pendulum": mg.PENDULUM}[family]
    kw = dict(max_episode_steps=LIMIT[family])
    D = mg.get_spec(kind).obs_dim

    def weights(H):
        rng = np.random.default_rng(100 + H)
        return ((rng.normal(0, 1, (H, D)) * np.array(IN_SCALE[family])).astype(np.float32), rng.normal(0, 0.5, H).astype(np.float32),
                (rng.normal(0, 1, (1, H)) / np.sqrt(H)).astype(np.float32), rng.normal(0, 0.1, 1).astype(np.float32))

    def window_of(timed):
        timed(5)                                        # warm-up
        per = timed(5) / 5                              # ms per launch of K steps
        count = max(5, int(window * 1000.0 / per) + 1)
        return timed(count), count

    def fused(call):
        env = mg.VecEnv(kind, n, seed=7, auto_reset=True, **kw)
        rew, done, trunc = mg.DeviceArray((K, n), np.float32), mg.DeviceArray((K, n), np.uint8), mg.DeviceArray((K, n), np.uint8)
        env.reset_device()
        env.sync()
        calls = [0]

        def timed(count):
            env.timer_start()
            for _ in range(count):
                call(env, calls[0], rew, done, trunc)
                calls[0] += 1
            ms = env.timer_stop()
            env.sync()                                  # (raises on a sticky device error)
            return ms

        ms, count = window_of(timed)
        env.close()
        return ms, count

    def torch_loop(H, act):
        env = mg.TorchVecEnv(kind, n, seed=7, auto_reset=True, obs_layout="aos", **kw)
        w1, b1, w2, b2 = (torch.from_numpy(x).cuda() for x in weights(H))
        w1t, w2t = w1.t().contiguous(), w2.t().contiguous()
        fn = torch.relu if act == "relu" else torch.tanh
        state = [env.reset()]

        def timed(count):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            obs = state[0]
            e0.record()
            for _ in range(count * K):
                h = fn(torch.addmm(b1, obs, w1t))
                mu = torch.addmm(b2, h, w2t).squeeze(1)
                a = mu + SIGMA * torch.randn(n, device=mu.device, dtype=torch.float32)
                obs = env.step(a)[0]
            e1.record()
            e1.synchronize()
            env.check()
            state[0] = obs
            return e0.elapsed_time(e1)

        return window_of(timed)

    cases = []
    for H in (32, 64):
        for act in ("relu", "tanh"):
            w = weights(H)
            pol = np.concatenate([w[0].ravel(), w[1], w[2].ravel(), w[3]])   # nn.Linear order: W1[H][D], b1[H], W2[1][H], b2[1]
            cases.append((f"gauss/H{H}/{act}", lambda pol=pol, H=H, act=act: fused(lambda env, c, r, d, t: env.rollout_mlp_gauss_device(pol, H, act, SIGMA, 9, c, K, None, None, r, d, t))))
            cases.append((f"mlp/H{H}/{act}", lambda pol=pol, H=H, act=act: fused(lambda env, c, r, d, t: env.rollout_mlp_device(pol, H, act, K, None, None, r, d, t))))
            cases.append((f"torch/H{H}/{act}", lambda H=H, act=act: torch_loop(H, act)))
    cases = cases[rotate % len(cases):] + cases[: rotate % len(cases)]
    out = []
    for name, run in cases:
        ms, count = run()
        out.append(dict(family=family, n_envs=n, K=K, case=name, launches=count, window_ms=ms, ns_per_env_step=ms * 1e6 / (count * K * n)))
    print("RESULT " + json.dumps(out), flush=True)


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
    families = [(f, n) for f, n in FAMILIES if f in args.families.split(",")]
    runs = []
    for rep in range(args.repeats):
        for family, n in families:
            n = max(1024, int(n * args.scale)) // 1024 * 1024
            # a fresh child per family and repeat; the parent never opens the GPU
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", family, str(n), str(5 * rep), "--window", str(args.window), "--K", str(args.K),
                                "--out", args.out], capture_output=True, text=True, timeout=600)
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
                raise SystemExit(f"worker {family} repeat {rep} failed with status {r.returncode}")   # nothing more is started on the GPU
            runs += [dict(rec, repeat=rep) for rec in json.loads(line[0][7:])]
            print(f"repeat {rep} {family}: done", flush=True)
    summary = {}
    for rec in runs:
        summary.setdefault(f"{rec['family']}/{rec['case']}", []).append(rec["ns_per_env_step"])
    table = {k: dict(median=statistics.median(v), min=min(v), max=max(v), spread=(max(v) - min(v)) / statistics.median(v),
                     env_steps_per_s=1e9 / statistics.median(v), repeats=[round(x, 6) for x in v]) for k, v in sorted(summary.items())}
    head = dict(unit="ns per env-step", K=args.K, window_s=args.window, repeats=args.repeats, scale=args.scale, sigma=SIGMA,
                n_envs={f: max(1024, int(n * args.scale)) // 1024 * 1024 for f, n in families}, max_episode_steps={f: LIMIT[f] for f, _ in families},
                cases="gauss: mgym_rollout_mlp_gauss; mlp: mgym_rollout_mlp (identity head) of the same build; torch: addmm, activation, addmm, mu + sigma * randn, step")
    write_record(args.out, head, table)
    for k, v in table.items():
        print(f"{k:44s} median {v['median']:.4f}  min {v['min']:.4f}  max {v['max']:.4f}  spread {100 * v['spread']:.2f} %  {v['env_steps_per_s']:.3e} env-steps/s")


if __name__ == "__main__":
    main()
