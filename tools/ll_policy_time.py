"""LunarLander rollouts by action source, timed with device events in one process (GPU box): the table rollout (mgym_rollout), the in-kernel
linear policy (mgym_rollout_linear) and the in-kernel uniform policy (mgym_rollout_uniform) at K = 16 and 64, interleaved, beside the loop a
user has without them — K x (torch scores + argmax, mgym_step through TorchVecEnv).  ms per step-equivalent, median and range of the repetitions.

    python tools/ll_policy_time.py [n_envs] [reps] > profiles/<file>.json
"""
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import modurl_gym_amd as mg  # noqa: E402

W = np.zeros((4, 9), np.float32)   # the weights of tests/test_gpu_lunar_policy.py: all four actions, contacts, finished episodes
W[0, 6] = 2.0; W[0, 7] = 2.0
W[1, 4] = 3.0; W[1, 5] = 1.5; W[1, 8] = -0.1
W[2, 1] = -0.5; W[2, 3] = -4.0; W[2, 8] = -0.6
W[3, 4] = -3.0; W[3, 5] = -1.5; W[3, 8] = -0.1


def main():
    import torch
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    env = mg.VecEnv(mg.LUNARLANDER, n, seed=1, enable_wind=True, auto_reset=True)
    env.reset()
    kmax = 64
    act = mg.DeviceArray((kmax, n), np.uint32)
    obs = mg.DeviceArray((kmax, 8, n), np.float32)
    rew = mg.DeviceArray((kmax, n), np.float32)
    done, trunc = mg.DeviceArray((kmax, n), np.uint8), mg.DeviceArray((kmax, n), np.uint8)
    table = np.random.default_rng(0).integers(0, 4, (kmax, n)).astype(np.uint32)
    tab = mg.DeviceArray.from_numpy(table)
    pol = W.ravel()
    te = mg.TorchVecEnv(mg.LUNARLANDER, n, seed=1, enable_wind=True, auto_reset=True)
    wt = torch.from_numpy(W[:, :8].copy()).cuda()
    bt = torch.from_numpy(W[:, 8].copy()).cuda()[:, None]
    o = te.reset()
    seed = [0]

    def run(kind, K):
        nonlocal o
        if kind == "torch_loop":
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(K):
                a = (wt @ o + bt).argmax(dim=0).to(torch.int32)
                o = te.step(a)[0]
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)
        env.timer_start()
        if kind == "table":
            env.rollout_device(tab, K, obs, rew, done, trunc)
        elif kind == "linear":
            env.rollout_linear_device(pol, K, act, obs, rew, done, trunc)
        else:
            seed[0] += 1
            env.rollout_uniform_device(seed[0], K, act, obs, rew, done, trunc)
        ms = env.timer_stop()
        env.sync()
        return ms

    kinds = ("table", "linear", "uniform", "torch_loop")
    for K in (16, kmax):   # warm-up
        for kind in kinds:
            run(kind, K)
    res = {K: {kind: [] for kind in kinds} for K in (16, kmax)}
    for _ in range(reps):
        for K in (16, kmax):
            for kind in kinds:
                res[K][kind].append(run(kind, K) / K)
    out = {"n_envs": n, "wind": True, "auto_reset": True, "reps": reps, "unit": "ms per step-equivalent (device events)", "by_K": {}}
    for K, r in res.items():
        med = {kind: statistics.median(v) for kind, v in r.items()}
        out["by_K"][str(K)] = {kind: {"median": round(med[kind], 4), "min": round(min(v), 4), "max": round(max(v), 4)} for kind, v in r.items()}
        out["by_K"][str(K)]["linear_over_table"] = round(med["linear"] / med["table"], 4)
        out["by_K"][str(K)]["uniform_over_table"] = round(med["uniform"] / med["table"], 4)
        out["by_K"][str(K)]["torch_loop_over_linear"] = round(med["torch_loop"] / med["linear"], 4)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
