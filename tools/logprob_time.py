#!/usr/bin/env python3
"""What mgym_logprob_mlp costs beside the torch pass it replaces in a collector, beside mgym_value_mlp's dense pass of the same widths, and beside the rollout
launch of the same network: the actor's log-probabilities over a rollout's buffers.

    python tools/logprob_time.py --repeats 5 --out profiles/logprob_time.json

The timing is tools/timing.py's (device events around a window of back-to-back calls, a warm-up and a probe of 3 calls each, a fresh process per repeat with
every case in it).  Rows: 1 048 576 and 4 096 environments, K = 16, CartPole (the sample head, A = 2) and Pendulum (the Gaussian head, sigma = 0.5), actors (32),
(64), (32, 32), (64, 64), ReLU and tanh_fast.  Inputs of the three passes are synthetic device tensors (observations uniform inside the family's bounds, actions
uniform over the two actions or standard normal), every output preallocated.  Columns, ns per env-step (K x n of them), all in one process:
    logp      mgym_logprob_mlp: K n evaluations of the actor and the head
    torch     the pass it replaces: torch.baddbmm (the batched addmm) / activation over cat(obs_first, obs[:-1]) — the [K, H, n] activations through memory —
              then log_softmax + gather, or the Gaussian log-density
    value     mgym_value_mlp without the final arguments with a critic of the same widths: (K + 1) n evaluations with one output and no head
    rollout   the launch that drew the actions: mgym_rollout_mlp_sample / _mlp_gauss (one hidden layer) or mgym_rollout_mlp2 (two) of the same network on a
              stepping handle with fused auto-reset (Pendulum: max_episode_steps = 200), as tools/mlp2_time.py times them, a new call word each
The record's ratios: torch / logp with faster_beyond_spread (the slowest fused repeat beats the fastest torch repeat); logp / value; and logp / rollout, the
call's cost as a share of the rollout launch of the same network — what the choice of a separate pass over emitting from inside the rollout kernels rests on.
Not measured here: hardware counters, other sizes or K, LunarLander, a training loop."""
import argparse
import os
import sys

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ENVS = (1 << 20, 4096)
K = 16
FAMILIES = {"cartpole": ((-4.8, -5.0, -0.42, -5.0), (4.8, 5.0, 0.42, 5.0)), "pendulum": ((-1.0, -1.0, -8.0), (1.0, 1.0, 8.0))}
HEAD = {"cartpole": "sample", "pendulum": "gauss"}
OUTPUTS = {"cartpole": 2, "pendulum": 1}
LIMIT = {"cartpole": 0, "pendulum": 200}
NETS = ((32,), (64,), (32, 32), (64, 64))
ACTIVATIONS = ("relu", "tanh_fast")
COLUMNS = ("logp", "torch", "value", "rollout")
SIGMA = 0.5


def worker(sizes, window, rotate):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import modurl_gym_amd as mg
    kinds = {"cartpole": mg.CARTPOLE, "pendulum": mg.PENDULUM}

    def window_of(body):
        return timing.window_of(timing.torch_timed(body), window, 3, 3)

    def weights(family, widths, outputs):
        lo, hi = FAMILIES[family]
        rng = np.random.default_rng(100 + sum(widths))
        dims = (len(lo), *widths, outputs)
        out = []
        for k, (fan_in, fan_out) in enumerate(zip(dims[:-1], dims[1:])):
            scale_in = 1.0 / np.array(hi) if k == 0 else 1.0 / np.sqrt(fan_in)
            out += [(rng.normal(0, 1, (fan_out, fan_in)) * scale_in).astype(np.float32), rng.normal(0, 0.5, fan_out).astype(np.float32)]
        return out

    def inputs(family, n):
        lo, hi = (torch.tensor(x, device="cuda")[:, None] for x in FAMILIES[family])
        g = torch.Generator(device="cuda").manual_seed(77)
        box = lambda *lead: lo + (hi - lo) * torch.rand(*lead, len(FAMILIES[family][0]), n, device="cuda", generator=g)
        if family == "cartpole":
            acts = torch.randint(0, 2, (K, n), device="cuda", generator=g, dtype=torch.int32)
        else:
            acts = torch.randn(K, n, device="cuda", generator=g)
        return dict(first=box(), obs=box(K), acts=acts)

    def logp(family, n, widths, act):
        x, w = inputs(family, n), weights(family, widths, OUTPUTS[family])
        env = mg.TorchVecEnv(kinds[family], n)
        env._bind_stream()
        policy, h1, h2 = (*env.env.pack_mlp(*w), 0) if len(widths) == 1 else env.env.pack_mlp2(*w)
        out = torch.empty((K, n), device="cuda")
        res = window_of(lambda: env.env.logprob_mlp_device(policy, h1, h2, act, HEAD[family], SIGMA, K, x["first"], x["obs"], x["acts"], out))
        env.check()
        env.close()
        return res

    def value(family, n, widths, act):
        x, w = inputs(family, n), weights(family, widths, 1)
        env = mg.TorchVecEnv(kinds[family], n)
        env._bind_stream()
        critic, h1, h2 = env.env.pack_critic(w)
        val, last = torch.empty((K, n), device="cuda"), torch.empty(n, device="cuda")
        res = window_of(lambda: env.env.value_mlp_device(critic, h1, h2, act, K, x["first"], x["obs"], None, None, None, val, last, None))
        env.check()
        env.close()
        return res

    def torch_expr(family, n, widths, act):
        x = inputs(family, n)
        w = [torch.from_numpy(a).cuda() for a in weights(family, widths, OUTPUTS[family])]
        fn = torch.relu if act == "relu" else torch.tanh
        index = x["acts"].long()[:, None, :] if family == "cartpole" else None   # (the learner's own int64 actions: not part of the pass)
        const = -float(np.log(SIGMA)) - 0.91893853320467274

        def body():
            h = torch.cat([x["first"][None], x["obs"][:-1]])   # [K, D, n]
            for k in range(0, len(w), 2):
                h = torch.baddbmm(w[k + 1][None, :, None], w[k].expand(h.shape[0], *w[k].shape), h)
                if k + 2 < len(w):
                    h = fn(h)
            if index is not None:
                return torch.log_softmax(h, 1).gather(1, index)[:, 0]
            z = (x["acts"] - h[:, 0]) / SIGMA
            return const - 0.5 * z * z
        return window_of(body)

    def rollout(family, n, widths, act):
        w = weights(family, widths, OUTPUTS[family])
        env = mg.VecEnv(kinds[family], n, seed=7, auto_reset=True, max_episode_steps=LIMIT[family])
        rew, done, trunc = mg.DeviceArray((K, n), np.float32), mg.DeviceArray((K, n), np.uint8), mg.DeviceArray((K, n), np.uint8)
        acts, obs = mg.DeviceArray((K, n), np.uint32), mg.DeviceArray((K, len(FAMILIES[family][0]), n), np.float32)   # a collector keeps both for this call
        env.reset_device()
        env.sync()
        calls = [0]
        if len(widths) == 1:
            pol, H = env.pack_mlp(*w)
        else:
            pol, H1, H2 = env.pack_mlp2(*w)

        def launch():
            if len(widths) == 2:
                env.rollout_mlp2_device(pol, H1, H2, act, HEAD[family], SIGMA, 9, calls[0], K, acts, obs, rew, done, trunc)
            elif family == "cartpole":
                env.rollout_mlp_sample_device(pol, H, act, 9, calls[0], K, acts, obs, rew, done, trunc)
            else:
                env.rollout_mlp_gauss_device(pol, H, act, SIGMA, 9, calls[0], K, acts, obs, rew, done, trunc)
            calls[0] += 1

        res = timing.window_of(timing.engine_timed(env, launch), window, 3, 3)
        env.close()
        return res

    runners = dict(logp=logp, torch=torch_expr, value=value, rollout=rollout)
    cases = []
    for n in sizes:
        for family in FAMILIES:
            for widths in NETS:
                for act in ACTIVATIONS:
                    for column in COLUMNS:
                        cases.append((n, family, widths, act, column, lambda run=runners[column], a=(family, n, widths, act): run(*a)))
    out = []
    for n, family, widths, act, column, run in timing.rotated(cases, rotate):
        ms, count = run()
        out.append(dict(n_envs=n, family=family, net="x".join(map(str, widths)), activation=act, case=column, calls=count, window_ms=ms,
                        ns_per_env_step=ms * 1e6 / (count * K * n)))
    timing.emit(out)


def record(runs, args, sizes):
    """(head, table) of the record, from the children's records and the command line alone"""
    table = timing.summarise(timing.grouped(runs, lambda r: f"{r['family']}/n{r['n_envs']}/{r['net']}/{r['activation']}/{r['case']}"), "list")
    ratios = {}
    for k, v in table.items():
        row, case = k.rsplit("/", 1)
        if case != "logp":
            continue
        t, val, roll = (table[f"{row}/{c}"] for c in ("torch", "value", "rollout"))
        ratios[row] = dict(torch_over_logp=t["median"] / v["median"], faster_beyond_spread=v["max"] < t["min"], logp_over_value=v["median"] / val["median"],
                           logp_share_of_rollout=v["median"] / roll["median"])
    head = dict(unit="ns per env-step (K x n per call)", window_s=args.window, repeats=args.repeats, n_envs=list(sizes), K=K, families=list(FAMILIES), heads=HEAD,
                sigma=SIGMA, nets=["x".join(map(str, c)) for c in NETS], activations=list(ACTIVATIONS), max_episode_steps=LIMIT,
                cases="logp: mgym_logprob_mlp; torch: baddbmm / activation over cat(obs_first, obs[:-1]), then log_softmax + gather or the Gaussian log-density; value: "
                      "mgym_value_mlp without the final arguments, a critic of the same widths; rollout: mgym_rollout_mlp_sample / _mlp_gauss / _mlp2 of the same network "
                      "with every output stored; all of a repeat in one process, device events around a window of back-to-back calls",
                ratios_of="torch / logp with faster_beyond_spread (the slowest logp repeat beats the fastest torch repeat); logp / value; logp / rollout, the call's cost "
                          "as a share of the rollout launch of the same network",
                not_measured="hardware counters, other sizes or K, LunarLander, a training loop", ratios=ratios)
    return head, table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of timed work per case")
    ap.add_argument("--sizes", default=",".join(map(str, N_ENVS)), help="populations, comma separated (a smoke run: 4096)")
    ap.add_argument("--out", required=True, help="record file (the committed record of the full run: profiles/logprob_time.json)")
    ap.add_argument("--worker", metavar="ROTATE", type=int)
    args = ap.parse_args()
    sizes = tuple(int(s) for s in args.sizes.split(","))
    if args.worker is not None:
        return worker(sizes, args.window, args.worker)
    runs = timing.run_children(lambda _, rep: [os.path.abspath(__file__), "--worker", str(7 * rep), "--window", str(args.window), "--sizes", args.sizes, "--out", args.out],
                               [None], args.repeats, 900)
    head, table = record(runs, args, sizes)
    timing.write_record(args.out, head, table)
    for k, v in table.items():
        print(f"{k:48s} median {v['median']:.5f}  min {v['min']:.5f}  max {v['max']:.5f}  spread {100 * v['spread']:.2f} %  {v['env_steps_per_s']:.3e} env-steps/s")
    for k, v in head["ratios"].items():
        print(f"{k:40s} torch / logp {v['torch_over_logp']:.2f}  beyond the spread: {v['faster_beyond_spread']}  logp / value {v['logp_over_value']:.2f}  "
              f"logp / rollout {v['logp_share_of_rollout']:.3f}")


if __name__ == "__main__":
    main()
