#!/usr/bin/env python3
"""What the fused advantage and episode-return scans cost beside the torch loops they replace:

    python tools/gae_time.py --repeats 5 --out profiles/gae_time.json

The timing is tools/timing.py's (torch events around a window of back-to-back calls, a warm-up and a probe of 3 calls each, a fresh process per repeat with
every case in it).  Rows: 1 048 576 and 4 096 environments, K = 16 and 128.  Inputs are synthetic device tensors (rewards in [-16, 1], values in +-100, done
and truncated at a rate of 0.02 each), every output preallocated.  Columns, ns per env-step, all in one process:
    gae            mgym_gae with done, trunc and final_value, both outputs
    returns        mgym_episode_returns with done and trunc, both outputs
    torch_gae      the reverse loop of INTEGRATION.md section 3 written with torch.where (the same selections), K iterations
    torch_returns  the forward loop with a per-environment carry, K iterations
share_of_8TBps is the whole-call rate of the algorithmic bytes (GAE: 18 + 8 / K per env-step — reward 4, value 4, two flag bytes, two outputs of 4, last_value
and nothing for the sparse final_value; returns: 6 + 16 / K, plus nothing for the sparse outputs) against 8 TB/s.  It is not a kernel's share of peak: the window
holds launch gaps too.
Not measured here: hardware counters, other sizes, a training loop."""
import argparse
import os
import sys

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ENVS = (1 << 20, 4096)
KS = (16, 128)
GAMMA, LAM, RATE = 0.99, 0.95, 0.02
PEAK_BYTES_PER_S = 8e12


def algorithmic_bytes(case, K):
    return 18 + 8 / K if case.endswith("gae") else 6 + 16 / K


def worker(scale, window, rotate):
    sys.path.insert(0, ROOT)
    import torch
    import modurl_gym_amd as mg

    def window_of(body):
        return timing.window_of(timing.torch_timed(body), window, 3, 3)

    def inputs(n, K):
        g = torch.Generator(device="cuda").manual_seed(1234 + K)
        u01 = lambda *s: torch.rand(*s, device="cuda", generator=g)
        rew, val, fv = u01(K, n) * 17 - 16, u01(K, n) * 200 - 100, u01(K, n) * 200 - 100
        return dict(rew=rew, val=val, fv=fv, last=u01(n) * 200 - 100, done=u01(K, n) < RATE, trunc=u01(K, n) < RATE)

    def fused(what, n, K):
        x = inputs(n, K)
        env = mg.TorchVecEnv(mg.CARTPOLE, n)
        env._bind_stream()
        d8, u8 = x["done"].view(torch.uint8), x["trunc"].view(torch.uint8)
        if what == "gae":
            adv, ret = torch.empty_like(x["rew"]), torch.empty_like(x["rew"])
            body = lambda: env.env.gae_device(K, x["rew"], d8, u8, x["val"], x["last"], x["fv"], GAMMA, LAM, adv, ret)
        else:
            acc, ln = torch.zeros(n, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
            ro, lo = torch.zeros_like(x["rew"]), torch.zeros((K, n), dtype=torch.int32, device="cuda")
            body = lambda: env.env.episode_returns_device(K, x["rew"], d8, u8, acc, ln, ro, lo)
        out = window_of(body)
        env.check()
        env.close()
        return out

    def torch_gae(n, K):
        x = inputs(n, K)
        adv, ret = torch.empty_like(x["rew"]), torch.empty_like(x["rew"])
        zero, gl = torch.zeros(n, device="cuda"), GAMMA * LAM

        def body():
            carry, nxt = zero, x["last"]
            for t in range(K - 1, -1, -1):
                d, fin, v = x["done"][t], x["done"][t] | x["trunc"][t], x["val"][t]
                nv = torch.where(fin, torch.where(d, zero, x["fv"][t]), nxt)
                c = torch.where(fin, zero, carry)
                a = torch.add(torch.add(x["rew"][t], nv, alpha=GAMMA) - v, c, alpha=gl)
                adv[t] = a
                torch.add(a, v, out=ret[t])
                carry, nxt = a, v
        return window_of(body)

    def torch_returns(n, K):
        x = inputs(n, K)
        ro, lo = torch.zeros_like(x["rew"]), torch.zeros((K, n), dtype=torch.int32, device="cuda")
        zero, izero = torch.zeros(n, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
        carry = [zero.clone(), izero.clone()]

        def body():
            acc, ln = carry
            for t in range(K):
                fin = x["done"][t] | x["trunc"][t]
                acc, ln = acc + x["rew"][t], ln + 1
                torch.where(fin, acc, zero, out=ro[t])
                torch.where(fin, ln, izero, out=lo[t])
                acc, ln = torch.where(fin, zero, acc), torch.where(fin, izero, ln)
            carry[0], carry[1] = acc, ln
        return window_of(body)

    cases = []
    for n0 in N_ENVS:
        n = timing.scaled(n0, scale)
        for K in KS:
            cases.append((n, K, "gae", lambda n=n, K=K: fused("gae", n, K)))
            cases.append((n, K, "returns", lambda n=n, K=K: fused("returns", n, K)))
            cases.append((n, K, "torch_gae", lambda n=n, K=K: torch_gae(n, K)))
            cases.append((n, K, "torch_returns", lambda n=n, K=K: torch_returns(n, K)))
    out = []
    for n, K, name, run in timing.rotated(cases, rotate):
        ms, count = run()
        out.append(dict(n_envs=n, K=K, case=name, calls=count, window_ms=ms, ns_per_env_step=ms * 1e6 / (count * K * n)))
    timing.emit(out)


def record(runs, args):
    """(head, table) of the record, from the children's records and the command line alone"""
    table = timing.summarise(timing.grouped(runs, lambda rec: f"n{rec['n_envs']}/K{rec['K']}/{rec['case']}"), "list")
    for k, v in table.items():
        if not k.split("/")[2].startswith("torch"):
            v["share_of_8TBps"] = algorithmic_bytes(k, int(k.split("/")[1][1:])) / (v["median"] * 1e-9) / PEAK_BYTES_PER_S
    ratios = {}
    for k, v in table.items():
        row, case = k.rsplit("/", 1)
        if not case.startswith("torch"):
            t = table[f"{row}/torch_{case}"]
            # faster by more than the spread: the slowest fused repeat still beats the fastest torch repeat
            ratios[k] = dict(torch_over_fused=t["median"] / v["median"], faster_beyond_spread=v["max"] < t["min"])
    head = dict(unit="ns per env-step", window_s=args.window, repeats=args.repeats, scale=args.scale, n_envs=list(N_ENVS), K=list(KS), gamma=GAMMA, lam=LAM,
                flag_rate=RATE,
                cases="gae: mgym_gae (done, trunc, final_value, both outputs); returns: mgym_episode_returns (done, trunc, both outputs); torch_gae / torch_returns: "
                      "the K-iteration torch.where loops they replace; all of a repeat in one process, device events around a window of back-to-back calls",
                algorithmic_bytes_per_env_step="gae 18 + 8 / K, returns 6 + 16 / K (sparse final_value reads and return_out / length_out writes not counted)",
                share_of_8TBps="algorithmic bytes over whole-call time over 8e12 B/s: an end-to-end figure, launch gaps included, not a kernel's share of peak",
                not_measured="hardware counters, other sizes, a training loop", ratios=ratios)
    return head, table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of timed work per case")
    ap.add_argument("--scale", type=float, default=1.0, help="population scale (smoke runs)")
    ap.add_argument("--out", required=True, help="record file (the committed record of the full run: profiles/gae_time.json)")
    ap.add_argument("--worker", nargs=2, metavar=("SCALE", "ROTATE"))
    args = ap.parse_args()
    if args.worker:
        return worker(float(args.worker[0]), args.window, int(args.worker[1]))
    runs = timing.run_children(lambda _, rep: [os.path.abspath(__file__), "--worker", str(args.scale), str(5 * rep), "--window", str(args.window), "--out", args.out],
                               [None], args.repeats, 600)
    head, table = record(runs, args)
    timing.write_record(args.out, head, table)
    for k, v in table.items():
        share = f"  {100 * v['share_of_8TBps']:.1f} % of 8 TB/s" if "share_of_8TBps" in v else ""
        print(f"{k:36s} median {v['median']:.5f}  min {v['min']:.5f}  max {v['max']:.5f}  spread {100 * v['spread']:.2f} %  {v['env_steps_per_s']:.3e} env-steps/s{share}")
    for k, v in head["ratios"].items():
        print(f"{k:36s} torch / fused {v['torch_over_fused']:.1f}  faster beyond the spread: {v['faster_beyond_spread']}")


if __name__ == "__main__":
    main()
