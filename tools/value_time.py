#!/usr/bin/env python3
"""What mgym_value_mlp costs beside the torch expression it replaces in a collector: a critic's values over a rollout's buffers.

    python tools/value_time.py --repeats 5 --out profiles/value_time.json

The timing is tools/timing.py's (torch events around a window of back-to-back calls, a warm-up and a probe of 3 calls each, a fresh process per repeat with
every case in it).  Rows: 1 048 576 and 4 096 environments, K = 16, CartPole (D = 4) and Pendulum (D = 3), critics (32), (64), (32, 32), (64, 64), ReLU and
tanh_fast.  Inputs are synthetic device tensors (observations uniform inside the family's bounds, trunc at the column's rate, done NULL so that the rate is the
selection rate), every output preallocated.  Columns, ns per env-step (K x n of them), all in one process:
    value         mgym_value_mlp without the final arguments: the dense pass alone, (K + 1) n evaluations
    value_p005    ... with final_obs, trunc and final_value_out at a selection rate of 0.005: the dense pass and the final pass
    value_p05     ... at a selection rate of 0.05
    torch_dense   torch.baddbmm, activation, ... over cat(obs_first, obs[:-1]) and over obs[-1]: two passes, what `value` replaces
    torch         those two and the same network over the whole final_obs: three passes, what a caller of mgym_gae wrote before
The record's ratios: torch / value_p005, torch / value_p05 and torch_dense / value with faster_beyond_spread (the slowest fused repeat beats the fastest torch
repeat); the final pass's added time, value_pXXX - value, per env-step and per selected env-step, and added(0.05) / added(0.005) — 10 if it follows the selected
count, 1 if it follows K x n; and the dense pass beside the same-width mgym_rollout_mlp / _mlp2 row of profiles/mlp2_time.json (greedy head for CartPole, Gaussian
for Pendulum: a rollout also steps the environment, so it is the nearest existing figure for the same arithmetic, not the same work).
Not measured here: hardware counters, other sizes or K, a training loop."""
import argparse
import json
import os
import sys

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ENVS = (1 << 20, 4096)
K = 16
FAMILIES = {"cartpole": ((-4.8, -5.0, -0.42, -5.0), (4.8, 5.0, 0.42, 5.0)), "pendulum": ((-1.0, -1.0, -8.0), (1.0, 1.0, 8.0))}
CRITICS = ((32,), (64,), (32, 32), (64, 64))
ACTIVATIONS = ("relu", "tanh_fast")
RATES = {"value_p005": 0.005, "value_p05": 0.05}
COLUMNS = ("value", "value_p005", "value_p05", "torch_dense", "torch")
MLP2_ROW = {"cartpole": "greedy", "pendulum": "gauss"}


def worker(scale, window, rotate):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import modurl_gym_amd as mg
    kinds = {"cartpole": mg.CARTPOLE, "pendulum": mg.PENDULUM}

    def window_of(body):
        return timing.window_of(timing.torch_timed(body), window, 3, 3)

    def weights(family, widths):
        lo, hi = FAMILIES[family]
        rng = np.random.default_rng(100 + sum(widths))
        dims = (len(lo), *widths, 1)
        out = []
        for k, (fan_in, fan_out) in enumerate(zip(dims[:-1], dims[1:])):
            scale_in = 1.0 / np.array(hi) if k == 0 else 1.0 / np.sqrt(fan_in)
            out += [(rng.normal(0, 1, (fan_out, fan_in)) * scale_in).astype(np.float32), rng.normal(0, 0.5, fan_out).astype(np.float32)]
        return out

    def inputs(family, n):
        lo, hi = (torch.tensor(x, device="cuda")[:, None] for x in FAMILIES[family])
        g = torch.Generator(device="cuda").manual_seed(77)
        u01 = lambda *s: torch.rand(*s, device="cuda", generator=g)
        box = lambda *lead: lo + (hi - lo) * u01(*lead, len(FAMILIES[family][0]), n)
        return dict(first=box(), obs=box(K), final=box(K), u=u01(K, n))

    def fused(family, n, widths, act, column):
        x, w = inputs(family, n), weights(family, widths)
        env = mg.TorchVecEnv(kinds[family], n)
        env._bind_stream()
        critic, h1, h2 = env.env.pack_critic(w)
        value, last = torch.empty((K, n), device="cuda"), torch.empty(n, device="cuda")
        fo = u = fv = None
        if column != "value":
            fo, u, fv = x["final"], (x["u"] < RATES[column]).to(torch.uint8), torch.zeros((K, n), device="cuda")
        out = window_of(lambda: env.env.value_mlp_device(critic, h1, h2, act, K, x["first"], x["obs"], fo, None, u, value, last, fv))
        env.check()
        env.close()
        return out

    def torch_expr(family, n, widths, act, column):
        x = inputs(family, n)
        w = [torch.from_numpy(a).cuda() for a in weights(family, widths)]
        fn = torch.relu if act == "relu" else torch.tanh

        def value(o):   # [R, D, n] -> [R, n]
            h = o
            for k in range(0, len(w), 2):
                h = torch.baddbmm(w[k + 1][None, :, None], w[k].expand(h.shape[0], *w[k].shape), h)
                if k + 2 < len(w):
                    h = fn(h)
            return h[:, 0]

        def body():
            value(torch.cat([x["first"][None], x["obs"][:-1]]))
            value(x["obs"][-1:])
            if column == "torch":
                value(x["final"])
        return window_of(body)

    cases = []
    for n0 in N_ENVS:
        n = timing.scaled(n0, scale)
        for family in FAMILIES:
            for widths in CRITICS:
                for act in ACTIVATIONS:
                    for column in COLUMNS:
                        run = torch_expr if column.startswith("torch") else fused
                        cases.append((n, family, widths, act, column, lambda run=run, a=(family, n, widths, act, column): run(*a)))
    out = []
    for n, family, widths, act, column, run in timing.rotated(cases, rotate):
        ms, count = run()
        out.append(dict(n_envs=n, family=family, critic="x".join(map(str, widths)), activation=act, case=column, calls=count, window_ms=ms,
                        ns_per_env_step=ms * 1e6 / (count * K * n)))
    timing.emit(out)


def record(runs, args):
    """(head, table) of the record, from the children's records, the command line and profiles/mlp2_time.json alone"""
    table = timing.summarise(timing.grouped(runs, lambda r: f"{r['family']}/n{r['n_envs']}/{r['critic']}/{r['activation']}/{r['case']}"), "list")
    with open(os.path.join(ROOT, "profiles", "mlp2_time.json")) as f:
        mlp2 = json.load(f)["summary"]
    ratios, final_pass, beside = {}, {}, {}
    for k, v in table.items():
        row, case = k.rsplit("/", 1)
        if case.startswith("torch"):
            continue
        t = table[f"{row}/{'torch_dense' if case == 'value' else 'torch'}"]
        ratios[k] = dict(torch_over_fused=t["median"] / v["median"], faster_beyond_spread=v["max"] < t["min"])
        if case == "value":
            added = {c: table[f"{row}/{c}"]["median"] - v["median"] for c in RATES}
            final_pass[row] = dict(added_ns_per_env_step=added, added_ns_per_selected_env_step={c: added[c] / RATES[c] for c in RATES},
                                   added_p05_over_p005=added["value_p05"] / added["value_p005"] if added["value_p005"] > 0 else None,
                                   added_share_of_dense={c: added[c] / v["median"] for c in RATES})
            family, n, critic, act = row.split("/")
            h = critic.split("x")
            ref = mlp2.get(f"{family}/{MLP2_ROW[family]}/{n}/{h[0]}x{h[0]}/{act}/{'mlp1' if len(h) == 1 else 'mlp2'}")
            if ref:
                beside[row] = dict(rollout_ns_per_env_step=ref["median"], value_ns_per_evaluation=v["median"] * K / (K + 1),
                                   rollout_over_value_evaluation=ref["median"] / (v["median"] * K / (K + 1)))
    head = dict(unit="ns per env-step (K x n per call)", window_s=args.window, repeats=args.repeats, scale=args.scale, n_envs=list(N_ENVS), K=K,
                families=list(FAMILIES), critics=["x".join(map(str, c)) for c in CRITICS], activations=list(ACTIVATIONS), selection_rates=RATES,
                cases="value: mgym_value_mlp without the final arguments; value_p005 / value_p05: with final_obs, trunc (done NULL) and final_value_out at that "
                      "selection rate; torch_dense: baddbmm / activation over cat(obs_first, obs[:-1]) and obs[-1]; torch: those and the whole final_obs; all of a "
                      "repeat in one process, device events around a window of back-to-back calls",
                ratios_against="value against torch_dense, value_p005 and value_p05 against torch",
                final_pass_claim="added_p05_over_p005 is 10 where the final pass's time follows the selected count and 1 where it follows K x n",
                beside_mlp2_time="the same-width mgym_rollout_mlp (mlp1) / mgym_rollout_mlp2 row of profiles/mlp2_time.json, which also steps the environment; "
                                 "value_ns_per_evaluation is the dense pass per (K + 1) n evaluations",
                not_measured="hardware counters, other sizes or K, a training loop", ratios=ratios, final_pass=final_pass, beside_rollouts=beside)
    return head, table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of timed work per case")
    ap.add_argument("--scale", type=float, default=1.0, help="population scale (smoke runs)")
    ap.add_argument("--out", required=True, help="record file (the committed record of the full run: profiles/value_time.json)")
    ap.add_argument("--worker", nargs=2, metavar=("SCALE", "ROTATE"))
    args = ap.parse_args()
    if args.worker:
        return worker(float(args.worker[0]), args.window, int(args.worker[1]))
    runs = timing.run_children(lambda _, rep: [os.path.abspath(__file__), "--worker", str(args.scale), str(7 * rep), "--window", str(args.window), "--out", args.out],
                               [None], args.repeats, 900)
    head, table = record(runs, args)
    timing.write_record(args.out, head, table)
    for k, v in table.items():
        print(f"{k:48s} median {v['median']:.5f}  min {v['min']:.5f}  max {v['max']:.5f}  spread {100 * v['spread']:.2f} %  {v['env_steps_per_s']:.3e} env-steps/s")
    for k, v in head["ratios"].items():
        print(f"{k:48s} torch / fused {v['torch_over_fused']:.2f}  faster beyond the spread: {v['faster_beyond_spread']}")
    for k, v in head["final_pass"].items():
        print(f"{k:40s} final pass added ns/env-step {v['added_ns_per_env_step']}  p05 / p005 {v['added_p05_over_p005']}")


if __name__ == "__main__":
    main()
