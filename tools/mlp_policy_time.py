#!/usr/bin/env python3
"""What the hidden-layer policy costs inside the rollout kernels (mgym_rollout_mlp), beside the loop it replaces and the linear policy:

    python tools/mlp_policy_time.py --repeats 5 --out profiles/mlp_policy_time.json

Per family — CartPole and MountainCar at 1 048 576 envs, LunarLander (wind) at 262 144 envs, K = 16, fused auto-reset on — ns per env-step of
    (a) mlp/H{32,64}/{relu,tanh}   mgym_rollout_mlp, one call per K steps, actions not stored (the packed-VALU form, the one that ships; the record
                                   profiles/mlp_policy_time.json also holds mlp_mfma/... rows of CartPole, taken in the same processes on a build that
                                   had the hidden layer on the matrix pipe behind a knob: it was slower and was removed)
    (b) torch/H{32,64}/{relu,tanh} the loop it replaces: TorchVecEnv with AoS observations [n, D]; per step torch.addmm(b1, obs, W1^T), the activation,
                                   torch.addmm(b2, h, W2^T), argmax, TorchVecEnv.step — eager kernels, the [n, H] activation through memory
    (c) linear                     mgym_rollout_linear, for scale
    (d) table, uniform             mgym_rollout (random actions from a device table) and mgym_rollout_uniform: the rows a change to the shared rollout
                                   kernels must not move
--K sets the steps per call (default 16), --families and --cases take comma-separated subsets (e.g. --families lunar_lander --K 64).  A run that is not
the full default one must name its --out: the default file is the committed record of the full run.  One run is one K on one library; a record that
compares libraries or Ks is put together from the runs' files:

    python tools/mlp_policy_time.py --merge parent=a16.json after=b16.json parent=a64.json after=b64.json --out profiles/ll_mlp_rollout_time.json

(rows "K<K>/<case>/<label>", the families' prefix dropped when every file holds one family).
The timing is tools/timing.py's: the handle's own timer for (a), (c) and (d), torch events for (b), a warm-up and a probe of 5 launches each, a fresh
process per family and repeat."""
import argparse
import json
import os
import sys

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = [("cartpole", 1 << 20), ("mountain_car", 1 << 20), ("lunar_lander", 1 << 18)]
IN_SCALE = {"cartpole": (2.0, 1.0, 8.0, 1.0), "mountain_car": (2.0, 40.0), "lunar_lander": (2.0, 2.0, 2.0, 2.0, 3.0, 2.0, 2.0, 2.0)}


def worker(family, n, window, rotate, K, only):
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
        ms, count = timing.window_of(timing.engine_timed(env, lambda: call(env, rew, done, trunc)), window, 5, 5)
        info = env.info()
        env.close()
        return ms, count, info

    def torch_loop(H, act):
        env = mg.TorchVecEnv(kind, n, seed=7, auto_reset=True, obs_layout="aos", **kw)
        timed = timing.torch_policy_timed(env, timing.mlp_weights(D, A, H, IN_SCALE[family]), act, timing.torch_heads()["greedy"], K)
        return timing.window_of(timed, window, 5, 5) + ({},)

    cases = []
    for H in (32, 64):
        for act in ("relu", "tanh"):
            w = timing.mlp_weights(D, A, H, IN_SCALE[family])
            pol = np.concatenate([w[0].ravel(), w[1], w[2].ravel(), w[3]])   # nn.Linear order: W1[H][D], b1[H], W2[A][H], b2[A]
            cases.append((f"mlp/H{H}/{act}", lambda pol=pol, H=H, act=act: fused(lambda env, r, d, t: env.rollout_mlp_device(pol, H, act, K, None, None, r, d, t))))
            cases.append((f"torch/H{H}/{act}", lambda H=H, act=act: torch_loop(H, act)))
    lin = np.random.default_rng(3).normal(0, 1, (1 if family == "cartpole" else A) * (D + 1)).astype(np.float32)
    cases.append(("linear", lambda: fused(lambda env, r, d, t: env.rollout_linear_device(lin, K, None, None, r, d, t))))
    tab = mg.DeviceArray.from_numpy(np.random.default_rng(5).integers(0, A, (K, n)).astype(np.uint32))
    cases.append(("table", lambda: fused(lambda env, r, d, t: env.rollout_device(tab, K, None, r, d, t))))
    cases.append(("uniform", lambda: fused(lambda env, r, d, t: env.rollout_uniform_device(9, K, None, None, r, d, t))))
    if only:
        cases = [c for c in cases if c[0].split("/")[0] in only]
    out = []
    for name, run in timing.rotated(cases, rotate):
        ms, count, info = run()
        out.append(dict(family=family, n_envs=n, K=K, case=name, launches=count, window_ms=ms, ns_per_env_step=ms * 1e6 / (count * K * n),
                        env_steps_per_s=count * K * n / (ms * 1e-3), rollout_form=info.get("rollout"), persistent_launches=info.get("rollout_persistent_launches")))
    timing.emit(out)


def merge(pairs, out):
    rows, heads = {}, []
    for pair in pairs:
        label, path = pair.split("=", 1)
        rec = json.load(open(path))
        heads.append(dict(label=label, K=rec["K"], repeats=rec["repeats"], window_s=rec["window_s"], n_envs=rec["n_envs"]))
        one = len(rec["n_envs"]) == 1
        for k, v in rec["summary"].items():
            rows[f"K{rec['K']}/{k.split('/', 1)[1] if one else k}/{label}"] = v
    timing.write_record(out, dict(unit="ns per env-step", runs=heads), dict(sorted(rows.items())))


def populations(args):
    return {f: timing.scaled(n, args.scale) for f, n in FAMILIES if f in args.families.split(",")}


def record(runs, args):
    """(head, table) of the record, from the children's records and the command line alone"""
    table = timing.summarise(timing.grouped(runs, lambda rec: f"{rec['family']}/{rec['case']}"), "list")
    head = dict(unit="ns per env-step", K=args.K, window_s=args.window, repeats=args.repeats, scale=args.scale,
                n_envs=populations(args), forms="mlp: the packed-VALU form (v_pk_fma_f32 chains, weights as scalar operands)")
    return head, table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of timed work per case")
    ap.add_argument("--scale", type=float, default=1.0, help="population scale (smoke runs)")
    ap.add_argument("--out", default=None, help="record file (default, full runs only: profiles/mlp_policy_time.json)")
    ap.add_argument("--merge", nargs="+", metavar="LABEL=FILE", help="put the records of several runs into one file (--out) and exit")
    ap.add_argument("--K", type=int, default=16, help="steps per rollout call")
    ap.add_argument("--families", default=",".join(f for f, _ in FAMILIES), help="comma-separated subset of the families")
    ap.add_argument("--cases", default="", help="comma-separated subset of mlp,torch,linear,table,uniform (default: all)")
    ap.add_argument("--worker", nargs=3, metavar=("FAMILY", "N", "ROTATE"))
    args = ap.parse_args()
    K = args.K
    only = [c for c in args.cases.split(",") if c]
    if set(only) - {"mlp", "torch", "linear", "table", "uniform"}:
        raise SystemExit(f"--cases: unknown case in {args.cases!r} (mlp, torch, linear, table, uniform)")
    full = K == 16 and not only and args.families == ap.get_default("families") and args.scale == 1.0
    if args.out is None and not args.worker:
        if args.merge or not full:
            raise SystemExit("--out is required for a merge and for a run with --K, --families, --cases or --scale: the default file is the full run's record")
        args.out = os.path.join(ROOT, "profiles", "mlp_policy_time.json")
    if args.merge:
        return merge(args.merge, args.out)
    if args.worker:
        return worker(args.worker[0], int(args.worker[1]), args.window, int(args.worker[2]), K, only)
    sizes = populations(args)
    runs = timing.run_children(lambda family, rep: [os.path.abspath(__file__), "--worker", family, str(sizes[family]), str(3 * rep), "--window", str(args.window),
                                                    "--K", str(K), "--cases", args.cases], list(sizes), args.repeats, 600)
    head, table = record(runs, args)
    timing.write_record(args.out, head, table)
    for k, v in table.items():
        print(f"{k:34s} median {v['median']:.4f}  min {v['min']:.4f}  max {v['max']:.4f}  spread {100 * v['spread']:.2f} %  {v['env_steps_per_s']:.3e} env-steps/s")


if __name__ == "__main__":
    main()
