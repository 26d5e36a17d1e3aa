"""References for Pendulum-v1 (MGYM_PENDULUM), shared by test_pendulum_ref.py, test_pendulum_host.py and test_gpu_pendulum.py.  No test here.

 * PendulumRef — the word-exact reference: the text of include/mgym.h restated on numpy float32 arrays, one rounded operation per line.  sinf, cosf,
   fmodf are glibc's over whole arrays (tests/glibc_f32.py: numpy's own f32 sin is not glibc's); the hidden-layer policy is tests/mlp_ref.py's; the
   reset draw and the uniform policy use the Philox4x32-10 of tests/philox_ref.py.
 * step_f64 — gymnasium's step in float64 (the text of gymnasium/envs/classic_control/pendulum.py: gymnasium is not a dependency), angle_normalize with
   Python's % and the true pi.
 * the build of tests/native/pendulum_check.cpp — modurl_gym_amd/csrc/pendulum_step.h compiled for the host — as a shared object and as a program.
"""
import ctypes as C
import functools
import math

import numpy as np

import mlp_ref as M
import native_build
from glibc_f32 import cosf, fmodf, sinf
from mlp_ref import RELU, TANH
from philox_ref import SLOT_POLICY, env_draw, own_word, uniform_f64_to_f32
from words import same_words, words_of

SRC = "pendulum_check.cpp"
F = np.float32
PI_F, TWO_PI_F = F(3.14159274), F(6.28318548)
POL_TABLE, POL_LINEAR, POL_UNIFORM, POL_MLP_RELU, POL_MLP_TANH = range(5)
REWARD_MIN = -16.2736044   # -(pi^2 + 0.1 * 8^2 + 0.001 * 2^2)
BIG_TH = (1e6, -1e6, 12345.678, 3.1415927, -3.1415927, -0.0)   # imported angles: beyond the fast range reduction, at the wrap, and -0


class PdRun(C.Structure):
    _fields_ = [("n", C.c_uint64), ("steps", C.c_int32), ("seed", C.c_uint64), ("env_id_base", C.c_uint64), ("g", C.c_float), ("limit", C.c_uint32),
                ("auto_reset", C.c_int32), ("policy", C.c_int32), ("weights", C.c_void_p), ("hidden", C.c_int32), ("policy_seed", C.c_uint64),
                ("call", C.c_uint32), ("actions_in", C.c_void_p), ("state_in", C.c_void_p), ("actions_out", C.c_void_p), ("obs0", C.c_void_p),
                ("obs", C.c_void_p), ("reward", C.c_void_p), ("trunc", C.c_void_p), ("elapsed_out", C.c_void_p), ("state_out", C.c_void_p),
                ("finished", C.c_uint64), ("bad", C.c_int32), ("flush", C.c_int32)]


@functools.lru_cache(maxsize=None)
def check_lib():
    lib = C.CDLL(native_build.shared(SRC))
    lib.pendulum_run.restype, lib.pendulum_run.argtypes = C.c_int, [C.POINTER(PdRun)]
    return lib


def check_program():
    return native_build.program(SRC)


# ---- the text of include/mgym.h ----
def clamp(v, lo, hi):
    """v < lo ? lo : (v > hi ? hi : v): a NaN passes through"""
    return np.where(v < F(lo), F(lo), np.where(v > F(hi), F(hi), v)).astype(F)


def step_words(th, thdot, a, c_g):
    """One step of the header text on float32 arrays -> (th', thdot', reward, nan): where a is NaN the state comes back untouched with reward 0"""
    th, thdot, a = (np.ascontiguousarray(v, F) for v in (th, thdot, a))
    c_g = F(c_g)
    with np.errstate(all="ignore"):
        nan = np.isnan(a)
        u = clamp(a, -2.0, 2.0)
        x = th + PI_F
        r = fmodf(x, TWO_PI_F)
        r = np.where(r < F(0), r + TWO_PI_F, r).astype(F)
        an = r - PI_F
        t0 = an * an
        t1 = thdot * thdot
        t2 = F(0.1) * t1
        t3 = t0 + t2
        t4 = u * u
        t5 = F(0.001) * t4
        cost = t3 + t5
        s = sinf(th)
        p0 = c_g * s
        p1 = F(3.0) * u
        acc = p0 + p1
        d0 = acc * F(0.05)
        d1 = thdot + d0
        thdot2 = clamp(d1, -8.0, 8.0)
        e0 = thdot2 * F(0.05)
        th2 = th + e0
        reward = -cost
    return (np.where(nan, th, th2).astype(F), np.where(nan, thdot, thdot2).astype(F), np.where(nan, F(0), reward).astype(F), nan)


def reset_draw(seed, gid, episode):
    """-> (th, thdot) of the reset of env gid's episode number `episode`"""
    w = env_draw(seed, gid, episode)
    return uniform_f64_to_f32(-math.pi, math.pi, w[0], w[1]), uniform_f64_to_f32(-1.0, 1.0, w[2], w[3])


def uniform_actions(policy_seed, call, gid, t):
    """mgym_rollout_uniform's torque of env gid at step t of the handle's uniform call number `call`"""
    word = own_word(policy_seed, call, gid, SLOT_POLICY + int(t))
    return ((word >> np.uint32(8)).astype(F) * F(2.0 ** -22) - F(2.0)).astype(F)


def linear_actions(policy, obs):
    w = np.asarray(policy, F)
    with np.errstate(all="ignore"):
        return (((w[0] * obs[0] + w[1] * obs[1]) + w[2] * obs[2]) + w[3]).astype(F)


class PendulumRef:
    """n environments of the word-exact reference with the engine's surface: reset / set_state / step, the time limit and the fused auto-reset"""

    def __init__(self, n, seed=0, env_id_base=0, g=10.0, limit=0, auto_reset=False):
        self.n, self.seed, self.limit, self.auto_reset = n, seed, int(limit), auto_reset
        self.gid = np.uint64(env_id_base) + np.arange(n, dtype=np.uint64)
        self.c_g = F(1.5) * F(g)
        self.th, self.thdot = np.zeros(n, F), np.zeros(n, F)
        self.episode, self.elapsed = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        self.finished, self.bad, self.uniform_calls = 0, False, 0

    def obs(self):
        return np.stack([cosf(self.th), sinf(self.th), self.thdot])

    def _reset_where(self, m):
        th, thdot = reset_draw(self.seed, self.gid, self.episode)
        self.th, self.thdot = np.where(m, th, self.th).astype(F), np.where(m, thdot, self.thdot).astype(F)
        self.episode = np.where(m, self.episode + np.uint32(1), self.episode).astype(np.uint32)
        self.elapsed = np.where(m, 0, self.elapsed).astype(np.uint32)

    def reset(self, mask=None):
        self._reset_where(np.ones(self.n, bool) if mask is None else np.asarray(mask).astype(bool))
        return self.obs()

    def reset_deterministic(self):
        self.th[:], self.thdot[:], self.elapsed[:] = 0, 0, 0
        return self.obs()

    def get_state(self):
        return np.stack([words_of(self.th), words_of(self.thdot), self.episode])

    def set_state(self, blob):
        b = np.ascontiguousarray(blob, np.uint32)
        self.th, self.thdot, self.episode = b[0].view(F).copy(), b[1].view(F).copy(), b[2].copy()
        self.elapsed[:] = 0

    def step(self, actions):
        """-> (obs [3, n], reward, done, truncated)"""
        a = np.ascontiguousarray(actions, F)
        self.th, self.thdot, reward, nan = step_words(self.th, self.thdot, a, self.c_g)
        self.bad |= bool(nan.any())
        trunc = np.zeros(self.n, np.uint8)
        if self.limit:
            self.elapsed = np.minimum(self.elapsed + np.uint32(1), np.uint32(65535)).astype(np.uint32)
            trunc = (self.elapsed >= self.limit).astype(np.uint8)
            self.finished += int(trunc.sum())
            if self.auto_reset and trunc.any():
                self._reset_where(trunc.astype(bool))
        return self.obs(), reward, np.zeros(self.n, np.uint8), trunc

    def rollout(self, K, policy):
        """K steps; policy(t, obs before the step) -> actions.  -> (actions [K, n], obs [K, 3, n], reward, done, trunc)"""
        out = [[] for _ in range(5)]
        o = self.obs()
        for t in range(K):
            a = np.ascontiguousarray(policy(t, o), F)
            o, r, d, tr = self.step(a)
            for lst, v in zip(out, (a, o, r, d, tr)):
                lst.append(v)
        return tuple(np.stack(v) for v in out)

    def rollout_uniform(self, policy_seed, K):
        call = self.uniform_calls
        self.uniform_calls += 1
        return self.rollout(K, lambda t, o: uniform_actions(policy_seed, call, self.gid, t))

    def rollout_linear(self, policy, K):
        return self.rollout(K, lambda t, o: linear_actions(policy, o))

    def rollout_mlp(self, policy, H, act, K):
        return self.rollout(K, lambda t, o: M.scores(policy, 3, 1, H, o, act)[0])


# ---- gymnasium's step in float64 ----
def angle_normalize(x):
    return ((x + math.pi) % (2 * math.pi)) - math.pi


def step_f64(th, thdot, a, g):
    """gymnasium PendulumEnv.step with m = l = 1, dt = 0.05, max_speed = 8, max_torque = 2, on Python floats -> (th', thdot', cos, sin, reward)"""
    m, l, dt = 1.0, 1.0, 0.05
    u = min(max(a, -2.0), 2.0)
    costs = angle_normalize(th) ** 2 + 0.1 * thdot ** 2 + 0.001 * (u ** 2)
    newthdot = thdot + (3 * g / (2 * l) * math.sin(th) + 3.0 / (m * l ** 2) * u) * dt
    newthdot = min(max(newthdot, -8.0), 8.0)
    newth = th + newthdot * dt
    return newth, newthdot, math.cos(newth), math.sin(newth), -costs


# ---- the host-compiled header ----
def header_run(n, steps, seed=0, env_id_base=0, g=10.0, limit=0, auto_reset=False, policy=POL_TABLE, weights=None, hidden=0, policy_seed=0, call=0,
               actions=None, state=None, flush=False):
    """pendulum_run of tests/native/pendulum_check.cpp -> dict(actions, obs0, obs, reward, trunc, elapsed, state, finished, bad); flush: with denormals flushed to zero (x86)"""
    lib = check_lib()
    w = np.ascontiguousarray(weights if weights is not None else np.zeros(4), F)
    acts = np.ascontiguousarray(actions if actions is not None else np.zeros((steps, n)), F)
    st = None if state is None else np.ascontiguousarray(state, np.uint32)
    assert acts.shape == (steps, n) and (st is None or st.shape == (3, n))
    out = dict(actions=np.zeros((steps, n), F), obs0=np.zeros((3, n), F), obs=np.zeros((steps, 3, n), F), reward=np.zeros((steps, n), F),
               trunc=np.zeros((steps, n), np.uint8), elapsed=np.zeros(n, np.uint32), state=np.zeros((3, n), np.uint32))
    p = PdRun(n, steps, int(seed), int(env_id_base), float(g), int(limit), int(auto_reset), int(policy), w.ctypes.data, int(hidden), int(policy_seed), int(call),
              acts.ctypes.data, None if st is None else st.ctypes.data, out["actions"].ctypes.data, out["obs0"].ctypes.data, out["obs"].ctypes.data,
              out["reward"].ctypes.data, out["trunc"].ctypes.data, out["elapsed"].ctypes.data, out["state"].ctypes.data, 0, 0, int(flush))
    assert lib.pendulum_run(C.byref(p)) == 0
    out["finished"], out["bad"] = int(p.finished), bool(p.bad)
    return out


def ref_run(n, steps, seed=0, env_id_base=0, g=10.0, limit=0, auto_reset=False, policy=POL_TABLE, weights=None, hidden=0, policy_seed=0, call=0,
            actions=None, state=None):
    """the same run through PendulumRef, in header_run's output form"""
    ref = PendulumRef(n, seed, env_id_base, g, limit, auto_reset)
    if state is None:
        obs0 = ref.reset()
    else:
        ref.set_state(state)
        obs0 = ref.obs()
    ref.uniform_calls = call
    if policy == POL_TABLE:
        a, o, r, d, tr = ref.rollout(steps, lambda t, obs: actions[t])
    elif policy == POL_UNIFORM:
        a, o, r, d, tr = ref.rollout_uniform(policy_seed, steps)
    elif policy == POL_LINEAR:
        a, o, r, d, tr = ref.rollout_linear(weights, steps)
    else:
        a, o, r, d, tr = ref.rollout_mlp(weights, hidden, TANH if policy == POL_MLP_TANH else RELU, steps)
    return dict(actions=a, obs0=obs0, obs=o, reward=r, trunc=tr, elapsed=ref.elapsed, state=ref.get_state(), finished=ref.finished, bad=ref.bad)


def assert_same_run(got, exp, what=""):
    for k in ("actions", "obs0", "obs", "reward"):
        assert same_words(got[k], exp[k]), f"{what}: {k} differs"
    for k in ("trunc", "elapsed", "state"):
        assert np.array_equal(got[k], exp[k]), f"{what}: {k} differs"
    assert (got["finished"], got["bad"]) == (exp["finished"], exp["bad"]), what
