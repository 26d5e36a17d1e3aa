"""The checker of the episode time limit (mgym_config::max_episode_steps, include/mgym.h): the unchanged CPU oracle inside a small
TimeLimit wrapper — gymnasium's rule.  After every oracle step elapsed += 1 and truncated = elapsed >= limit (0: off); `done` is not
touched; with auto-reset the environments with either flag are reset through the oracle, their reset observations merged into the
step's and their counts zeroed.  Helper module of tests/test_time_limit_host.py and tests/test_gpu_time_limit.py."""
import numpy as np


class TimeLimitRef:
    def __init__(self, ref, limit, auto_reset, nthreads=1, own_truncation=False):
        """own_truncation: the oracle truncates by itself (CartPole at 500 steps) and its flag is OR-ed in; otherwise it is asserted absent"""
        self.ref, self.limit, self.auto_reset, self.nthreads, self.own_truncation = ref, int(limit), bool(auto_reset), nthreads, own_truncation
        self.elapsed = np.zeros(ref.n, np.int64)
        self.finished = 0                     # steps with either flag (what mgym_episode_count counts)
        self.kinds = {"done_only": 0, "trunc_only": 0, "both": 0}

    def reset(self, mask=None):
        obs = self.ref.reset(mask, nthreads=self.nthreads)
        if mask is None:
            self.elapsed[:] = 0
        else:
            self.elapsed[np.asarray(mask).astype(bool)] = 0
        return obs

    def step(self, actions):
        obs, rew, done, own = self.ref.step(actions, nthreads=self.nthreads)
        assert self.own_truncation or not own.any()   # the oracle itself (the reference's rule) never truncates the other families
        self.elapsed += 1
        trunc = ((self.elapsed >= self.limit) & (self.limit != 0)).astype(np.uint8) | own
        d, t = done.astype(bool), trunc.astype(bool)
        self.kinds["done_only"] += int((d & ~t).sum())
        self.kinds["trunc_only"] += int((~d & t).sum())
        self.kinds["both"] += int((d & t).sum())
        fin = (d | t)
        self.final_obs = obs                  # the step's own observation, before any reset observation is merged in
        self.finished += int(fin.sum())
        if self.auto_reset and fin.any():
            ro = self.ref.reset(fin.astype(np.uint8), nthreads=self.nthreads)
            obs = np.where(fin[None, :], ro, obs)
            self.elapsed[fin] = 0
        return obs, rew, done, trunc
