#!/usr/bin/env python3
"""What mgym_ppo_grad_mlp and mgym_value_grad_mlp cost beside the torch update they replace and beside mgym_logprob_mlp, the forward arithmetic of the same net.

    python tools/grad_time.py --repeats 5 --window 0.1 --out profiles/grad_time.json
    python tools/grad_time.py --repeats 3 --window 0.1 --columns ppo,value --lib OTHER/libmgym.so --out FILE     (an A/B of two builds on one machine)

The timing is tools/timing.py's (device events around a window of back-to-back calls, a warm-up and a probe of 3 calls each, a fresh process per repeat with
every case in it).  Rows: 1 048 576 and 4 096 environments, K = 16, CartPole (the sample head, A = 2) and Pendulum (the Gaussian head, sigma = 0.5), H = 32 and
64, ReLU and tanh_fast.  Inputs are synthetic device tensors (observations uniform inside the family's bounds, actions uniform over the two actions or standard
normal, logp_old the device's own mgym_logprob_mlp plus noise of 0.1, adv and ret standard normal), every output and the workspace (best_bytes) preallocated.
Columns, ns per env-step (K x n of them), all in one process:
    ppo       mgym_ppo_grad_mlp over the full range: both launches
    ppo4      the same batch as 4 calls on 4 contiguous slices of the environments (four minibatches)
    value     mgym_value_grad_mlp with a critic of the same width
    logp      mgym_logprob_mlp of the same actor: the forward arithmetic alone
    torch     the path ppo replaces: addmm / activation over the [K n, D] batch, log_softmax + gather or the Gaussian log-density, the clipped surrogate with
              the entropy bonus, backward(), the gradients flattened into one tensor
The record's ratios: torch / ppo with faster_beyond_spread (the slowest fused repeat beats the fastest torch repeat); ppo4 / ppo; ppo / logp; and the
algorithmic bytes of a ppo env-step, D + 3 words, over its time as a share of 8 TB/s.
--hidden2 H2 (default 0: everything above, unchanged) times the two-layer calls instead — mgym_ppo_grad_mlp2, mgym_value_grad_mlp2 and mgym_logprob_mlp at
hidden2 = H2 — against the torch update of the same two-layer net, H2 = -1 meaning the first width again ((32, 32) and (64, 64)); the rows are then named
"32x32" and the record says hidden2.
Not measured here: hardware counters, other sizes or K, LunarLander, the one-per-lane kernels, a full training loop."""
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
WIDTHS = (32, 64)
ACTIVATIONS = ("relu", "tanh_fast")
COLUMNS = ("ppo", "ppo4", "value", "logp", "torch")
SIGMA, CLIP, ENT_COEF = 0.5, 0.2, 0.01
PEAK_BYTES_PER_S = 8e12


def worker(sizes, window, rotate, columns, lib, hidden2=0):
    sys.path.insert(0, ROOT)
    if lib:
        from modurl_gym_amd import _lib
        _lib.LIB_PATH = os.path.abspath(lib)   # before anything loads the library
    import numpy as np
    import torch
    import modurl_gym_amd as mg
    kinds = {"cartpole": mg.CARTPOLE, "pendulum": mg.PENDULUM}

    def window_of(body):
        return timing.window_of(timing.torch_timed(body), window, 3, 3)

    def second(H):
        return H if hidden2 < 0 else hidden2

    def weights(family, H, outputs):
        lo, hi = FAMILIES[family]
        rng = np.random.default_rng(100 + H)
        w = [(rng.normal(0, 1, (H, len(lo))) / np.array(hi)).astype(np.float32), rng.normal(0, 0.5, H).astype(np.float32)]
        if hidden2:
            w += [(rng.normal(0, 1.5, (second(H), H)) / np.sqrt(H)).astype(np.float32), rng.normal(0, 0.5, second(H)).astype(np.float32)]
            H = second(H)
        return w + [(rng.normal(0, 1, (outputs, H)) / np.sqrt(H)).astype(np.float32), rng.normal(0, 0.5, outputs).astype(np.float32)]

    def inputs(family, n, env, policy, H, act):
        lo, hi = (torch.tensor(x, device="cuda")[:, None] for x in FAMILIES[family])
        g = torch.Generator(device="cuda").manual_seed(77)
        box = lambda *lead: lo + (hi - lo) * torch.rand(*lead, len(FAMILIES[family][0]), n, device="cuda", generator=g)
        x = dict(first=box(), obs=box(K))
        x["acts"] = torch.randint(0, 2, (K, n), device="cuda", generator=g, dtype=torch.int32) if family == "cartpole" else torch.randn(K, n, device="cuda", generator=g)
        x["old"] = torch.empty((K, n), device="cuda")
        if policy is not None:
            env.env.logprob_mlp_device(policy, H, second(H) if hidden2 else 0, act, HEAD[family], SIGMA, K, x["first"], x["obs"], x["acts"], x["old"])
            x["old"] += 0.1 * torch.randn(K, n, device="cuda", generator=g)
        x["adv"], x["ret"] = torch.randn(K, n, device="cuda", generator=g), torch.randn(K, n, device="cuda", generator=g)
        return x

    def fused(family, n, H, act, column):
        outputs = 1 if column == "value" else OUTPUTS[family]
        w = weights(family, H, outputs)
        env = mg.TorchVecEnv(kinds[family], n)
        env._bind_stream()
        policy = env.env.pack_critic(w)[0] if column == "value" else (env.env.pack_mlp2(*w)[0] if hidden2 else env.env.pack_mlp(*w)[0])
        H2 = second(H) if hidden2 else 0
        x = inputs(family, n, env, None if column == "value" else policy, H, act)
        nbytes = env.env.grad_workspace_bytes2(H, H2)[1] if H2 else env.env.grad_workspace_bytes(H)[1]
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
        grad, stats, logp = torch.empty(len(policy) + 1, device="cuda"), torch.empty(8, device="cuda"), torch.empty((K, n), device="cuda")
        e = env.env

        def ppo(first, count):
            if H2:
                return e.ppo_grad_mlp2_device(policy, H, H2, act, HEAD[family], SIGMA, K, first, count, x["first"], x["obs"], x["acts"], x["old"], x["adv"], CLIP, ENT_COEF,
                                              ws, nbytes, grad, stats)
            e.ppo_grad_mlp_device(policy, H, act, HEAD[family], SIGMA, K, first, count, x["first"], x["obs"], x["acts"], x["old"], x["adv"], CLIP, ENT_COEF, ws, nbytes,
                                  grad, stats)

        def value():
            if H2:
                return e.value_grad_mlp2_device(policy, H, H2, act, K, 0, n, x["first"], x["obs"], x["ret"], ws, nbytes, grad, stats)
            e.value_grad_mlp_device(policy, H, act, K, 0, n, x["first"], x["obs"], x["ret"], ws, nbytes, grad, stats)
        body = {"ppo": lambda: ppo(0, n), "ppo4": lambda: [ppo(k * (n // 4), n // 4) for k in range(4)], "value": value,
                "logp": lambda: e.logprob_mlp_device(policy, H, H2, act, HEAD[family], SIGMA, K, x["first"], x["obs"], x["acts"], logp)}[column]
        res = window_of(body)
        env.check()
        assert bool(torch.isfinite(grad).all()) or column == "logp"
        env.close()
        return res

    def torch_update(family, n, H, act, column):
        env = mg.TorchVecEnv(kinds[family], n)
        env._bind_stream()
        w = weights(family, H, OUTPUTS[family])
        x = inputs(family, n, env, (env.env.pack_mlp2(*w) if hidden2 else env.env.pack_mlp(*w))[0], H, act)
        env.close()
        params = [torch.from_numpy(a).cuda().requires_grad_(True) for a in w] + [torch.tensor([float(np.log(SIGMA))], device="cuda", requires_grad=True)]
        fn = torch.relu if act == "relu" else torch.tanh
        rows = torch.cat([x["first"][None], x["obs"][:-1]]).transpose(1, 2).reshape(K * n, -1).contiguous()   # the learner's own [B, D] batch: not part of the pass
        index = x["acts"].long().reshape(-1, 1) if family == "cartpole" else None
        acts, old, adv = x["acts"].reshape(-1), x["old"].reshape(-1), x["adv"].reshape(-1)

        def body():
            for p in params:
                p.grad = None
            s, ls = rows, params[-1]
            for k in range(0, len(params) - 3, 2):
                s = fn(torch.addmm(params[k + 1], s, params[k].T))
            s = torch.addmm(params[-2], s, params[-3].T)
            if index is not None:
                lsm = torch.log_softmax(s, 1)
                logp, ent = lsm.gather(1, index)[:, 0], -(lsm.exp() * lsm).sum(1).mean()
            else:
                dist = torch.distributions.Normal(s[:, 0], ls.exp(), validate_args=False)
                logp, ent = dist.log_prob(acts), dist.entropy().mean()
            r = (logp - old).exp()
            loss = -torch.min(r * adv, torch.clamp(r, 1 - CLIP, 1 + CLIP) * adv).mean() - ENT_COEF * ent
            loss.backward()
            return torch.cat([p.grad.reshape(-1) for p in params if p.grad is not None])
        return window_of(body)

    cases = []
    for n in sizes:
        for family in FAMILIES:
            for H in WIDTHS:
                for act in ACTIVATIONS:
                    for column in columns:
                        run = torch_update if column == "torch" else fused
                        cases.append((n, family, H, act, column, lambda run=run, a=(family, n, H, act, column): run(*a)))
    out = []
    for n, family, H, act, column, run in timing.rotated(cases, rotate):
        ms, count = run()
        out.append(dict(n_envs=n, family=family, net=net_name(H, hidden2), activation=act, case=column, calls=count, window_ms=ms, ns_per_env_step=ms * 1e6 / (count * K * n)))
    timing.emit(out)


def net_name(H, hidden2):
    return str(H) if not hidden2 else f"{H}x{H if hidden2 < 0 else hidden2}"


def record(runs, args, sizes):
    """(head, table) of the record, from the children's records and the command line alone"""
    table = timing.summarise(timing.grouped(runs, lambda r: f"{r['family']}/n{r['n_envs']}/{r['net']}/{r['activation']}/{r['case']}"), "list")
    ratios = {}
    for k, v in table.items():
        row, case = k.rsplit("/", 1)
        if case != "ppo" or any(f"{row}/{c}" not in table for c in ("torch", "ppo4", "logp")):   # (a run of some columns has no ratios)
            continue
        t, four, logp = (table[f"{row}/{c}"] for c in ("torch", "ppo4", "logp"))
        words = len(FAMILIES[row.split("/")[0]][0]) + 3
        ratios[row] = dict(torch_over_ppo=t["median"] / v["median"], faster_beyond_spread=v["max"] < t["min"], ppo4_over_ppo=four["median"] / v["median"],
                           ppo_over_logp=v["median"] / logp["median"], share_of_8_tb_s=4 * words / (v["median"] * 1e-9) / PEAK_BYTES_PER_S)
    head = dict(unit="ns per env-step (K x n per call)", window_s=args.window, repeats=args.repeats, n_envs=list(sizes), K=K, families=list(FAMILIES), heads=HEAD,
                sigma=SIGMA, clip=CLIP, ent_coef=ENT_COEF, nets=[net_name(h, args.hidden2) for h in WIDTHS], activations=list(ACTIVATIONS),
                cases="ppo: mgym_ppo_grad_mlp over the full range; ppo4: the same batch as 4 calls on 4 slices of the environments; value: mgym_value_grad_mlp, a critic "
                      "of the same width; logp: mgym_logprob_mlp of the same actor; torch: addmm / activation, log_softmax + gather or the Gaussian log-density, the "
                      "clipped surrogate with the entropy bonus, backward(), the gradients flattened; all of a repeat in one process, device events around a window of "
                      "back-to-back calls",
                ratios_of="torch / ppo with faster_beyond_spread (the slowest ppo repeat beats the fastest torch repeat); ppo4 / ppo; ppo / logp; the algorithmic "
                          "bytes of a ppo env-step (D + 3 words) over its time as a share of 8 TB/s",
                not_measured="hardware counters, other sizes or K, LunarLander, the one-per-lane kernels, a full training loop", ratios=ratios)
    if args.lib or tuple(args.columns) != COLUMNS:   # an A/B run names its build and its columns; the full run's record keeps its keys
        head.update(lib=os.path.basename(args.lib) if args.lib else "the package's", columns=list(args.columns))
    if args.hidden2:   # the two-layer run names itself; the one-layer record keeps its keys
        head.update(hidden2=args.hidden2, two_layers="ppo, ppo4 and value are mgym_ppo_grad_mlp2 / mgym_value_grad_mlp2, logp is mgym_logprob_mlp at hidden2, torch is "
                                                    "the update of the same two-layer net")
    return head, table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of timed work per case")
    ap.add_argument("--sizes", default=",".join(map(str, N_ENVS)), help="populations, comma separated (a smoke run: 4096)")
    ap.add_argument("--out", required=True, help="record file (the committed record of the full run: profiles/grad_time.json)")
    ap.add_argument("--columns", default=",".join(COLUMNS), help="the columns to time, comma separated (the ratios need all of them)")
    ap.add_argument("--lib", default="", help="time this build of libmgym.so instead of the package's (an A/B of two builds on one machine)")
    ap.add_argument("--hidden2", type=int, default=0, help="0: one hidden layer; H2: the two-layer calls at (H, H2); -1: at (H, H)")
    ap.add_argument("--worker", metavar="ROTATE", type=int)
    args = ap.parse_args()
    sizes = tuple(int(s) for s in args.sizes.split(","))
    args.columns = tuple(args.columns.split(","))
    assert set(args.columns) <= set(COLUMNS), args.columns
    if args.worker is not None:
        return worker(sizes, args.window, args.worker, args.columns, args.lib, args.hidden2)
    runs = timing.run_children(lambda _, rep: [os.path.abspath(__file__), "--worker", str(7 * rep), "--window", str(args.window), "--sizes", args.sizes, "--out", args.out,
                                                "--columns", ",".join(args.columns), "--lib", args.lib, "--hidden2", str(args.hidden2)],
                               [None], args.repeats, 900)
    head, table = record(runs, args, sizes)
    timing.write_record(args.out, head, table)
    for k, v in table.items():
        print(f"{k:48s} median {v['median']:.5f}  min {v['min']:.5f}  max {v['max']:.5f}  spread {100 * v['spread']:.2f} %  {v['env_steps_per_s']:.3e} env-steps/s")
    for k, v in head["ratios"].items():
        print(f"{k:40s} torch / ppo {v['torch_over_ppo']:.2f}  beyond the spread: {v['faster_beyond_spread']}  ppo4 / ppo {v['ppo4_over_ppo']:.2f}  "
              f"ppo / logp {v['ppo_over_logp']:.2f}  share of 8 TB/s {100 * v['share_of_8_tb_s']:.2f} %")


if __name__ == "__main__":
    main()
