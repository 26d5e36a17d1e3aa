"""References for Acrobot-v1 (MGYM_ACROBOT), shared by test_acrobot_ref.py, test_acrobot_host.py and test_gpu_acrobot.py.  No test here.

 * AcrobotRef — the word-exact reference: the text of include/mgym.h restated on numpy float32 arrays, one rounded operation per line.  sinf, cosf,
   fmodf are glibc's over whole arrays (tests/glibc_f32.py); the hidden-layer policy is tests/mlp_ref.py's, Philox and the reset's 53-bit uniform
   tests/philox_ref.py's, the categorical draw tests/mlp_sample_ref.py's.
 * step_f64 — gymnasium's step in float64 (the text of gymnasium/envs/classic_control/acrobot.py with book_or_nips = "book" and torque_noise_max = 0:
   gymnasium is not a dependency): rk4, wrap with its while loops, bound, the book dynamics with cos(x - pi/2).
 * the build of tests/native/acrobot_check.cpp — modurl_gym_amd/csrc/acrobot_step.h compiled for the host — as a shared object and as a program.
"""
import ctypes as C
import functools
import math

import numpy as np

import mlp_ref as M
import mlp_sample_ref as S
import native_build
from glibc_f32 import cosf, fmodf, sinf
from mlp_ref import RELU, TANH, argmax_words
from pendulum_ref import clamp
from philox_ref import SLOT_POLICY, env_draw, own_word, uniform_f64_to_f32
from words import same_words, words_of

SRC = "acrobot_check.cpp"
F = np.float32
PI_F, TWO_PI_F = F(3.14159274), F(6.28318548)
V1, V2 = F(4 * math.pi), F(9 * math.pi)
H_F, DT_F = F(0.1), F(0.2)
DT6 = F(F(0.2) / F(6.0))
POL_TABLE, POL_LINEAR, POL_UNIFORM, POL_MLP_RELU, POL_MLP_TANH, POL_MLP_RELU_SAMPLE, POL_MLP_TANH_SAMPLE = range(7)
D, A, _ = M.FAMILIES["acrobot"]


class AbRun(C.Structure):
    _fields_ = [("n", C.c_uint64), ("steps", C.c_int32), ("seed", C.c_uint64), ("env_id_base", C.c_uint64), ("limit", C.c_uint32),
                ("auto_reset", C.c_int32), ("policy", C.c_int32), ("weights", C.c_void_p), ("hidden", C.c_int32), ("policy_seed", C.c_uint64),
                ("call", C.c_uint32), ("actions_in", C.c_void_p), ("state_in", C.c_void_p), ("actions_out", C.c_void_p), ("obs0", C.c_void_p),
                ("obs", C.c_void_p), ("reward", C.c_void_p), ("done", C.c_void_p), ("trunc", C.c_void_p), ("elapsed_out", C.c_void_p),
                ("state_out", C.c_void_p), ("finished", C.c_uint64), ("bad", C.c_int32), ("flush", C.c_int32)]


@functools.lru_cache(maxsize=None)
def check_lib():
    lib = C.CDLL(native_build.shared(SRC))
    lib.acrobot_run.restype, lib.acrobot_run.argtypes = C.c_int, [C.POINTER(AbRun)]
    return lib


def check_program():
    return native_build.program(SRC)


# ---- the text of include/mgym.h ----
def deriv_words(th1, th2, w1, w2, tau):
    """deriv() on float32 arrays -> (dd1, dd2); the first two components of the derivative are w1 and w2 themselves"""
    s1, c1, s2, c2 = sinf(th1), cosf(th1), sinf(th2), cosf(th2)
    t0 = s1 * c2
    t1 = c1 * s2
    s12 = t0 + t1
    d1 = F(3.5) + c2
    t2 = F(0.5) * c2
    d2 = F(1.25) + t2
    phi2 = F(4.9) * s12
    p0 = w2 * w2
    p1 = F(0.5) * p0
    p2 = -p1
    p3 = p2 * s2
    q0 = w2 * w1
    q1 = q0 * s2
    x0 = p3 - q1
    x1 = F(14.7) * s1
    x2 = x0 + x1
    phi1 = x2 + phi2
    r0 = d2 / d1
    r1 = r0 * phi1
    n0 = tau + r1
    m0 = w1 * w1
    m1 = F(0.5) * m0
    m2 = m1 * s2
    n1 = n0 - m2
    n2 = n1 - phi2
    e0 = d2 * d2
    e1 = e0 / d1
    den = F(1.25) - e1
    dd2 = n2 / den
    z0 = d2 * dd2
    z1 = z0 + phi1
    z2 = z1 / d1
    dd1 = -z2
    return dd1.astype(F), dd2.astype(F)


def wrap_words(x):
    r = fmodf(x + PI_F, TWO_PI_F)
    r = np.where(r < F(0), r + TWO_PI_F, r).astype(F)
    return np.where((x > PI_F) | (x < -PI_F), r - PI_F, x).astype(F)


def _rk_sum(k1, k2, k3, k4):
    t0 = F(2.0) * k2
    t1 = k1 + t0
    t2 = F(2.0) * k3
    t3 = t1 + t2
    return t3 + k4


def step_words(th1, th2, w1, w2, a):
    """One step of the header text on float32 state arrays and uint32 actions -> (th1', th2', w1', w2', reward, done, bad): where a > 2 the state
    comes back untouched with reward 0 and done 0"""
    th1, th2, w1, w2 = (np.ascontiguousarray(v, F) for v in (th1, th2, w1, w2))
    a = np.ascontiguousarray(a, np.uint32)
    bad = a > np.uint32(2)
    with np.errstate(all="ignore"):
        tau = np.where(bad, np.uint32(1), a).astype(F) - F(1.0)
        a1, b1 = deriv_words(th1, th2, w1, w2, tau)
        u2, v2 = w1 + H_F * a1, w2 + H_F * b1
        a2, b2 = deriv_words(th1 + H_F * w1, th2 + H_F * w2, u2, v2, tau)
        u3, v3 = w1 + H_F * a2, w2 + H_F * b2
        a3, b3 = deriv_words(th1 + H_F * u2, th2 + H_F * v2, u3, v3, tau)
        u4, v4 = w1 + DT_F * a3, w2 + DT_F * b3
        a4, b4 = deriv_words(th1 + DT_F * u3, th2 + DT_F * v3, u4, v4, tau)
        n_th1 = th1 + DT6 * _rk_sum(w1, u2, u3, u4)
        n_th2 = th2 + DT6 * _rk_sum(w2, v2, v3, v4)
        n_w1 = w1 + DT6 * _rk_sum(a1, a2, a3, a4)
        n_w2 = w2 + DT6 * _rk_sum(b1, b2, b3, b4)
        n_th1, n_th2 = wrap_words(n_th1), wrap_words(n_th2)
        n_w1, n_w2 = clamp(n_w1, -V1, V1), clamp(n_w2, -V2, V2)
        c1, s1, c2, s2 = cosf(n_th1), sinf(n_th1), cosf(n_th2), sinf(n_th2)
        g0 = c1 * c2
        g1 = s1 * s2
        g2 = g0 - g1
        g3 = -c1
        done = ((g3 - g2) > F(1.0)) & ~bad
    keep = lambda old, new: np.where(bad, old, new).astype(F)
    reward = np.where(bad | done, F(0), F(-1)).astype(F)
    return keep(th1, n_th1), keep(th2, n_th2), keep(w1, n_w1), keep(w2, n_w2), reward, done.astype(np.uint8), bad


def reset_draw(seed, gid, episode):
    """-> (th1, th2, w1, w2) of the reset of env gid's episode number `episode`"""
    a, b = env_draw(seed, gid, episode, 0), env_draw(seed, gid, episode, 1)
    u = lambda hi, lo: uniform_f64_to_f32(-0.1, 0.1, hi, lo)
    return u(a[0], a[1]), u(a[2], a[3]), u(b[0], b[1]), u(b[2], b[3])


def uniform_actions(policy_seed, call, gid, t):
    """mgym_rollout_uniform's action of env gid at step t of the handle's uniform call number `call` (MountainCar's Discrete(3) draw)"""
    word = own_word(policy_seed, call, gid, SLOT_POLICY + int(t) // 2)
    h = (word >> np.uint32(16)) if int(t) & 1 else (word & np.uint32(0xFFFF))
    return ((h * np.uint32(3)) >> np.uint32(16)).astype(np.uint32)


def linear_scores(policy, obs):
    w = np.asarray(policy, F).reshape(3, 7)
    out = []
    with np.errstate(all="ignore"):
        for j in range(3):
            s = w[j, 0] * obs[0]
            for q in range(1, 6):
                s = s + w[j, q] * obs[q]
            out.append((s + w[j, 6]).astype(F))
    return np.stack(out)


class AcrobotRef:
    """n environments of the word-exact reference with the engine's surface: reset / set_state / step, the time limit and the fused auto-reset"""

    def __init__(self, n, seed=0, env_id_base=0, limit=0, auto_reset=False):
        self.n, self.seed, self.limit, self.auto_reset = n, seed, int(limit), auto_reset
        self.gid = np.uint64(env_id_base) + np.arange(n, dtype=np.uint64)
        self.s = [np.zeros(n, F) for _ in range(4)]   # th1, th2, w1, w2
        self.episode, self.elapsed = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        self.finished, self.bad, self.uniform_calls = 0, False, 0
        self.final = None   # the observation before the fused reset, where the last step finished an episode

    def obs(self):
        th1, th2, w1, w2 = self.s
        return np.stack([cosf(th1), sinf(th1), cosf(th2), sinf(th2), w1, w2])

    def _reset_where(self, m):
        new = reset_draw(self.seed, self.gid, self.episode)
        self.s = [np.where(m, v, old).astype(F) for v, old in zip(new, self.s)]
        self.episode = np.where(m, self.episode + np.uint32(1), self.episode).astype(np.uint32)
        self.elapsed = np.where(m, 0, self.elapsed).astype(np.uint32)

    def reset(self, mask=None):
        self._reset_where(np.ones(self.n, bool) if mask is None else np.asarray(mask).astype(bool))
        return self.obs()

    def reset_deterministic(self):
        self.s = [np.zeros(self.n, F) for _ in range(4)]
        self.elapsed[:] = 0
        return self.obs()

    def get_state(self):
        return np.stack([words_of(v) for v in self.s] + [self.episode])

    def set_state(self, blob):
        b = np.ascontiguousarray(blob, np.uint32)
        self.s = [b[k].view(F).copy() for k in range(4)]
        self.episode = b[4].copy()
        self.elapsed[:] = 0

    def step(self, actions):
        """-> (obs [6, n], reward, done, truncated)"""
        *self.s, reward, done, bad = step_words(*self.s, actions)
        self.bad |= bool(bad.any())
        trunc = np.zeros(self.n, np.uint8)
        if self.limit:
            self.elapsed = np.minimum(self.elapsed + np.uint32(1), np.uint32(65535)).astype(np.uint32)
            trunc = (self.elapsed >= self.limit).astype(np.uint8)
        fin = (done | trunc).astype(bool)
        self.finished += int(fin.sum())
        self.final = self.obs()
        if self.auto_reset and fin.any():
            self._reset_where(fin)
        return self.obs(), reward, done, trunc

    def rollout(self, K, policy):
        """K steps; policy(t, obs before the step) -> actions.  -> (actions [K, n], obs [K, 6, n], reward, done, trunc); self.finals [K, 6, n]"""
        out = [[] for _ in range(5)]
        finals = []
        o = self.obs()
        for t in range(K):
            a = np.ascontiguousarray(policy(t, o), np.uint32)
            o, r, d, tr = self.step(a)
            finals.append(self.final)
            for lst, v in zip(out, (a, o, r, d, tr)):
                lst.append(v)
        self.finals = np.stack(finals)
        return tuple(np.stack(v) for v in out)

    def rollout_uniform(self, policy_seed, K):
        call = self.uniform_calls
        self.uniform_calls += 1
        return self.rollout(K, lambda t, o: uniform_actions(policy_seed, call, self.gid, t))

    def rollout_linear(self, policy, K):
        return self.rollout(K, lambda t, o: argmax_words(linear_scores(policy, o)))

    def rollout_mlp(self, policy, H, act, K):
        return self.rollout(K, lambda t, o: argmax_words(M.scores(policy, D, A, H, o, act)))

    def rollout_mlp_sample(self, policy, H, act, seed, call, K):
        return self.rollout(K, lambda t, o: S.draw(M.scores(policy, D, A, H, o, act), S.words(seed, call, self.gid, t))[0])


# ---- gymnasium's step in float64 ----
def wrap64(x, m, M):
    x = np.array(x, np.float64)
    diff = M - m
    while (x > M).any():
        x = np.where(x > M, x - diff, x)
    while (x < m).any():
        x = np.where(x < m, x + diff, x)
    return x


def bound64(x, m, M):
    return np.minimum(np.maximum(x, m), M)


def dsdt64(s):
    m1 = m2 = l1 = 1.0
    lc1 = lc2 = 0.5
    I1 = I2 = 1.0
    g = 9.8
    theta1, theta2, dtheta1, dtheta2, a = s
    d1 = m1 * lc1 ** 2 + m2 * (l1 ** 2 + lc2 ** 2 + 2 * l1 * lc2 * np.cos(theta2)) + I1 + I2
    d2 = m2 * (lc2 ** 2 + l1 * lc2 * np.cos(theta2)) + I2
    phi2 = m2 * lc2 * g * np.cos(theta1 + theta2 - np.pi / 2.0)
    phi1 = (-m2 * l1 * lc2 * dtheta2 ** 2 * np.sin(theta2) - 2 * m2 * l1 * lc2 * dtheta2 * dtheta1 * np.sin(theta2)
            + (m1 * lc1 + m2 * l1) * g * np.cos(theta1 - np.pi / 2) + phi2)
    ddtheta2 = (a + d2 / d1 * phi1 - m2 * l1 * lc2 * dtheta1 ** 2 * np.sin(theta2) - phi2) / (m2 * lc2 ** 2 + I2 - d2 ** 2 / d1)
    ddtheta1 = -(d2 * ddtheta2 + phi1) / d1
    return np.stack([dtheta1, dtheta2, ddtheta1, ddtheta2, np.zeros_like(a)])


def step_f64(th1, th2, w1, w2, a):
    """gymnasium AcrobotEnv.step ("book", no noise) on float64 arrays (finite states only: its wrap loops) -> (th1', th2', w1', w2', terminated, margin),
    margin = -cos th1' - cos(th1' + th2') - 1 (terminated = margin > 0)"""
    dt = 0.2
    y0 = np.stack([np.asarray(v, np.float64) for v in (th1, th2, w1, w2)] + [np.asarray(a, np.float64) - 1.0])
    dt2 = dt / 2.0
    k1 = dsdt64(y0)
    k2 = dsdt64(y0 + dt2 * k1)
    k3 = dsdt64(y0 + dt2 * k2)
    k4 = dsdt64(y0 + dt * k3)
    ns = y0 + dt / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)
    n1, n2 = wrap64(ns[0], -np.pi, np.pi), wrap64(ns[1], -np.pi, np.pi)
    n3, n4 = bound64(ns[2], -4 * np.pi, 4 * np.pi), bound64(ns[3], -9 * np.pi, 9 * np.pi)
    margin = -np.cos(n1) - np.cos(n2 + n1) - 1.0
    return n1, n2, n3, n4, margin > 0.0, margin


# ---- the host-compiled header ----
def header_run(n, steps, seed=0, env_id_base=0, limit=0, auto_reset=False, policy=POL_TABLE, weights=None, hidden=0, policy_seed=0, call=0,
               actions=None, state=None, flush=False):
    """acrobot_run of tests/native/acrobot_check.cpp -> dict(actions, obs0, obs, reward, done, trunc, elapsed, state, finished, bad); flush: with denormals flushed to zero (x86)"""
    lib = check_lib()
    w = np.ascontiguousarray(weights if weights is not None else np.zeros(21), F)
    acts = np.ascontiguousarray(actions if actions is not None else np.zeros((steps, n)), np.uint32)
    st = None if state is None else np.ascontiguousarray(state, np.uint32)
    assert acts.shape == (steps, n) and (st is None or st.shape == (5, n))
    out = dict(actions=np.zeros((steps, n), np.uint32), obs0=np.zeros((6, n), F), obs=np.zeros((steps, 6, n), F), reward=np.zeros((steps, n), F),
               done=np.zeros((steps, n), np.uint8), trunc=np.zeros((steps, n), np.uint8), elapsed=np.zeros(n, np.uint32), state=np.zeros((5, n), np.uint32))
    p = AbRun(n, steps, int(seed), int(env_id_base), int(limit), int(auto_reset), int(policy), w.ctypes.data, int(hidden), int(policy_seed), int(call),
              acts.ctypes.data, None if st is None else st.ctypes.data, out["actions"].ctypes.data, out["obs0"].ctypes.data, out["obs"].ctypes.data,
              out["reward"].ctypes.data, out["done"].ctypes.data, out["trunc"].ctypes.data, out["elapsed"].ctypes.data, out["state"].ctypes.data, 0, 0, int(flush))
    assert lib.acrobot_run(C.byref(p)) == 0
    out["finished"], out["bad"] = int(p.finished), bool(p.bad)
    return out


def ref_rollout(ref, steps, policy=POL_TABLE, weights=None, hidden=0, policy_seed=0, call=0, actions=None):
    """`steps` steps of an AcrobotRef under one of the action sources -> (actions, obs, reward, done, trunc)"""
    if policy == POL_TABLE:
        return ref.rollout(steps, lambda t, obs: actions[t])
    if policy == POL_UNIFORM:
        ref.uniform_calls = call
        return ref.rollout_uniform(policy_seed, steps)
    if policy == POL_LINEAR:
        return ref.rollout_linear(weights, steps)
    act = TANH if policy in (POL_MLP_TANH, POL_MLP_TANH_SAMPLE) else RELU
    if policy in (POL_MLP_RELU_SAMPLE, POL_MLP_TANH_SAMPLE):
        return ref.rollout_mlp_sample(weights, hidden, act, policy_seed, call, steps)
    return ref.rollout_mlp(weights, hidden, act, steps)


def ref_run(n, steps, seed=0, env_id_base=0, limit=0, auto_reset=False, policy=POL_TABLE, weights=None, hidden=0, policy_seed=0, call=0,
            actions=None, state=None):
    """the same run through AcrobotRef, in header_run's output form"""
    ref = AcrobotRef(n, seed, env_id_base, limit, auto_reset)
    if state is None:
        obs0 = ref.reset()
    else:
        ref.set_state(state)
        obs0 = ref.obs()
    a, o, r, d, tr = ref_rollout(ref, steps, policy, weights, hidden, policy_seed, call, actions)
    return dict(actions=a, obs0=obs0, obs=o, reward=r, done=d, trunc=tr, elapsed=ref.elapsed, state=ref.get_state(), finished=ref.finished, bad=ref.bad)


def same_state(got, exp):
    """state blobs [5, n]: the four f32 columns as words (NaNs equal as a class), the episode column exactly"""
    g, e = np.ascontiguousarray(got, np.uint32), np.ascontiguousarray(exp, np.uint32)
    return same_words(g[:4].view(F), e[:4].view(F)) and np.array_equal(g[4], e[4])


def assert_same_run(got, exp, what=""):
    for k in ("obs0", "obs", "reward"):
        assert same_words(got[k], exp[k]), f"{what}: {k} differs"
    for k in ("actions", "done", "trunc", "elapsed"):
        assert np.array_equal(got[k], exp[k]), f"{what}: {k} differs"
    assert same_state(got["state"], exp["state"]), f"{what}: state differs"
    assert (got["finished"], got["bad"]) == (exp["finished"], exp["bad"]), what
