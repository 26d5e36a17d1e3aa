"""mgym_rollout_linear / mgym_rollout_uniform for LunarLanderV3 (include/mgym.h): the in-kernel policies of the persistent rollout launch
(ll_roll.h, action source LINEAR / UNIFORM) and of the K-step form (ll_policy_kernel + step()), each against a loop that computes the same
actions on the host and calls mgym_step, and against the CPU oracle driven by those actions — every word of every output.  Wind on throughout."""
import numpy as np
import pytest

import modurl_gym_amd as mg
from oracle import oracle as ora
from words import same

pytestmark = pytest.mark.gpu

# obs: x y vx vy angle angular-velocity leg0 leg1; actions: 0 nothing, 1 left engine, 2 main engine, 3 right engine.  Chosen against the
# oracle: all four actions, leg contacts and thousands of finished episodes within 160 steps of 4096 envs.
W = np.zeros((4, 9), np.float32)
W[0, 6] = 2.0; W[0, 7] = 2.0
W[1, 4] = 3.0; W[1, 5] = 1.5; W[1, 8] = -0.1
W[2, 1] = -0.5; W[2, 3] = -4.0; W[2, 8] = -0.6
W[3, 4] = -3.0; W[3, 5] = -1.5; W[3, 8] = -0.1
POL = W.ravel()


def lin_actions(w, obs):
    """the documented score (f32, each operation rounded, in order) and the sequential strict argmax"""
    w = np.asarray(w, np.float32).reshape(4, 9)
    a = np.zeros(obs.shape[1], np.uint32)
    best = None
    for j in range(4):
        s = w[j, 0] * obs[0]
        for q in range(1, 8):
            s = s + w[j, q] * obs[q]
        s = s + w[j, 8]
        if j == 0:
            best = s
        else:
            m = s > best
            best = np.where(m, s, best)
            a[m] = j
    return a


def uni_actions(seed, call, t, n, base=0):
    """Philox4x32-10(key = seed; counter = (g & ~3, call, 0x40000000 + t / 16)), word g % 4, bits 2 (t % 16) .. + 1"""
    a = np.zeros(n, np.uint32)
    for g0 in range(0, n, 4):
        gid = base + g0
        w = ora.philox([gid & 0xFFFFFFFF, gid >> 32, call, 0x40000000 + t // 16], [seed & 0xFFFFFFFF, seed >> 32])
        for k in range(min(4, n - g0)):
            a[g0 + k] = (int(w[k]) >> (2 * (t % 16))) & 3
    return a


MODES = {"persistent": {"MGYM_LL_ROLLOUT_MIN_K": "8"}, "k_steps_small_k": {"MGYM_LL_ROLLOUT_MIN_K": "8"}, "k_steps_disabled": {"MGYM_LL_ROLLOUT": "0"}}


def make(monkeypatch, mode, n, seed, auto_reset):
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    env = mg.VecEnv(mg.LUNARLANDER, n, seed=seed, enable_wind=True, auto_reset=auto_reset)
    for k in MODES[mode]:
        monkeypatch.delenv(k)
    info = env.info()
    assert info["rollout"] == ("k_steps" if mode == "k_steps_disabled" else "persistent_launch")
    return env


class Ref:
    """the stepping loop (mgym_step on a second handle) and the oracle, driven by the same actions"""

    def __init__(self, n, seed, auto_reset):
        self.loop = mg.VecEnv(mg.LUNARLANDER, n, seed=seed, enable_wind=True, auto_reset=auto_reset)
        self.ora = ora.OracleVec(ora.LUNARLANDER, n, seed=seed, enable_wind=True)
        self.auto_reset = auto_reset
        self.obs = self.loop.reset()
        assert same(self.ora.reset(nthreads=8), self.obs)

    def step(self, a):
        o, r, d, tr = self.loop.step(a)
        eo, er, ed, et = self.ora.step(a, nthreads=8)
        if self.auto_reset:
            m = (ed | et).astype(np.uint8)
            if m.any():
                ro = self.ora.reset(m, nthreads=8)
                eo = np.where(m.astype(bool)[None, :], ro, eo)
        for g, x, nm in zip((o, r, d, tr), (eo, er, ed, et), ("obs", "reward", "done", "truncated")):
            assert same(g, x), f"stepping loop vs oracle: {nm}"
        self.obs = o
        return o, r, d, tr


def check_outputs(got, ref, acts_fn, K, what):
    acts, gobs, grew, gdone, gtrunc = got
    for t in range(K):
        a = acts_fn(t, ref.obs)
        assert np.array_equal(acts[t], a), f"{what} step {t}: actions"
        o, r, d, tr = ref.step(a)
        for g, e, nm in zip((gobs[t], grew[t], gdone[t], gtrunc[t]), (o, r, d, tr), ("obs", "reward", "done", "truncated")):
            assert same(g, e), f"{what} step {t}: {nm}"


@pytest.mark.parametrize("mode,n,auto_reset", [("persistent", 4096, True), ("persistent", 97, True), ("persistent", 1, True), ("persistent", 97, False),
                                               ("k_steps_small_k", 4096, True), ("k_steps_small_k", 97, False), ("k_steps_small_k", 1, True),
                                               ("k_steps_disabled", 97, True), ("k_steps_disabled", 1, False)])
def test_linear_rollout_equals_step_loop_and_oracle(monkeypatch, mode, n, auto_reset):
    K, calls = (40, 4) if mode != "k_steps_small_k" else (5, 32)   # 160 steps either way
    env = make(monkeypatch, mode, n, 11, auto_reset)
    ref = Ref(n, 11, auto_reset)
    assert same(env.reset(), ref.obs)
    acts_all, legs, finished = [], 0, 0
    for c in range(calls):
        got = env.rollout_linear(POL, K)
        check_outputs(got, ref, lambda t, obs: lin_actions(POL, obs), K, f"call {c}")
        acts_all.append(got[0])
        legs += int((got[1][:, 6, :] > 0).sum())
        finished += int(got[3].sum())
    assert same(env.get_state(), ref.loop.get_state())
    if n == 4096:   # the weights reach every part of the step: all four actions, leg contacts, finished episodes
        acts = np.concatenate(acts_all)
        assert all(int((acts == j).sum()) > 0 for j in range(4))
        assert legs > 0 and finished > 100


@pytest.mark.parametrize("mode,n", [("persistent", 4096), ("persistent", 97), ("k_steps_small_k", 97), ("k_steps_disabled", 97)])
def test_uniform_rollout_equals_oracle_driven_by_the_documented_bits(monkeypatch, mode, n):
    K, seed = (24 if mode == "persistent" else 5), 0xFEEDC0DE12345
    env = make(monkeypatch, mode, n, 13, True)
    ref = Ref(n, 13, True)
    assert same(env.reset(), ref.obs)
    for call in range(3):   # consecutive calls advance the counter
        got = env.rollout_uniform(seed, K)
        check_outputs(got, ref, lambda t, obs: uni_actions(seed, call, t, n), K, f"call {call}")
    assert all(0.2 < float((got[0] == j).mean()) < 0.3 for j in range(4)) or n < 1000


def test_uniform_rollout_across_the_launch_split(monkeypatch):
    """K = 250 runs as launches of 240 and 10 steps; t counts on across them"""
    n, K, seed = 97, 250, 77
    env = make(monkeypatch, "persistent", n, 17, True)
    ref = Ref(n, 17, True)
    assert same(env.reset(), ref.obs)
    check_outputs(env.rollout_uniform(seed, K), ref, lambda t, obs: uni_actions(seed, 0, t, n), K, "K = 250")


def test_linear_rollout_large_population_equals_steps():
    n, K = 262144, 16
    env = mg.VecEnv(mg.LUNARLANDER, n, seed=3, enable_wind=True, auto_reset=True)
    loop = mg.VecEnv(mg.LUNARLANDER, n, seed=3, enable_wind=True, auto_reset=True)
    assert env.info()["rollout"] == "persistent_launch"
    obs = loop.reset()
    assert same(env.reset(), obs)
    for c in range(2):
        acts, gobs, grew, gdone, gtrunc = env.rollout_linear(POL, K)
        for t in range(K):
            a = lin_actions(POL, obs)
            assert np.array_equal(acts[t], a), f"call {c} step {t}: actions"
            o, r, d, tr = loop.step(a)
            for g, e, nm in zip((gobs[t], grew[t], gdone[t], gtrunc[t]), (o, r, d, tr), ("obs", "reward", "done", "truncated")):
                assert same(g, e), f"call {c} step {t}: {nm}"
            obs = o
    assert same(env.get_state(), loop.get_state())


def test_policy_rollouts_interleave_with_table_rollouts_steps_resets_and_set_state(monkeypatch):
    n, seed = 4096, 23
    env = make(monkeypatch, "persistent", n, seed, True)
    loop = mg.VecEnv(mg.LUNARLANDER, n, seed=seed, enable_wind=True, auto_reset=True)
    rng = np.random.default_rng(1)
    obs = loop.reset()
    assert same(env.reset(), obs)

    def loop_steps(acts_fn, K):
        nonlocal obs
        for t in range(K):
            obs = loop.step(acts_fn(t, obs))[0]
        assert same(env.get_state(), loop.get_state())

    env.rollout_linear(POL, 16); loop_steps(lambda t, o: lin_actions(POL, o), 16)
    tab = rng.integers(0, 4, (12, n)).astype(np.uint32)
    env.rollout(tab); loop_steps(lambda t, o: tab[t], 12)
    env.rollout_uniform(5, 16); loop_steps(lambda t, o: uni_actions(5, 0, t, n), 16)
    a = rng.integers(0, 4, n).astype(np.uint32)
    env.step(a); obs = loop.step(a)[0]
    m = (rng.random(n) < 0.3).astype(np.uint8)
    env.reset(m); loop.reset(m); obs = loop.observation()
    assert same(env.get_state(), loop.get_state())
    env.rollout_linear(POL, 9); loop_steps(lambda t, o: lin_actions(POL, o), 9)
    st = loop.get_state()
    env.set_state(st); loop.set_state(st); obs = loop.observation()
    assert same(env.observation(), obs)
    env.rollout_uniform(5, 16); loop_steps(lambda t, o: uni_actions(5, 1, t, n), 16)
    env.rollout_linear(POL, 20); loop_steps(lambda t, o: lin_actions(POL, o), 20)
    assert same(env.get_state(), loop.get_state())
    assert same(env.observation(), obs)


def test_captured_linear_rollout_equals_the_eager_call():
    n, K = 512, 16
    cap = mg.VecEnv(mg.LUNARLANDER, n, seed=29, enable_wind=True, auto_reset=True)
    eag = mg.VecEnv(mg.LUNARLANDER, n, seed=29, enable_wind=True, auto_reset=True)
    assert same(cap.reset(), eag.reset())
    bufs = [mg.DeviceArray((K, n), np.uint32), mg.DeviceArray((K, 8, n), np.float32), mg.DeviceArray((K, n), np.float32),
            mg.DeviceArray((K, n), np.uint8), mg.DeviceArray((K, n), np.uint8)]
    g = cap.graph_capture(lambda: cap.rollout_linear_device(POL, K, *bufs))
    try:
        cap.graph_launch(g)
        cap.sync()
    finally:
        cap.graph_destroy(g)
    exp = eag.rollout_linear(POL, K)
    for b, e, nm in zip(bufs, exp, ("actions", "obs", "reward", "done", "truncated")):
        assert same(b.numpy().reshape(-1)[: e.size].reshape(e.shape), e), nm
    assert same(cap.get_state(), eag.get_state())


def test_errors():
    env = mg.VecEnv(mg.LUNARLANDER, 8)
    with pytest.raises(mg.MgymError) as e1:
        env.rollout_linear(np.zeros(9, np.float32), 4)
    assert isinstance(e1.value, ValueError) and e1.value.status == mg.envs.L.ERR_BAD_ARG
    with pytest.raises(mg.NotResetError):
        env.rollout_linear(POL, 4)
    with pytest.raises(mg.NotResetError):
        env.rollout_uniform(1, 4)
    env.close()


def test_torch_rollout_linear_equals_vecenv():
    torch = pytest.importorskip("torch")
    n, K = 1024, 16
    te = mg.TorchVecEnv(mg.LUNARLANDER, n, seed=31, enable_wind=True, auto_reset=True)
    ve = mg.VecEnv(mg.LUNARLANDER, n, seed=31, enable_wind=True, auto_reset=True)
    te.reset()
    ve.reset()
    for c in range(2):
        got = te.rollout_linear(torch.from_numpy(POL), K)
        torch.cuda.synchronize()
        exp = ve.rollout_linear(POL, K)
        for g, e, nm in zip(got, exp, ("actions", "obs", "reward", "done", "truncated")):
            g = g.cpu().numpy()
            g = g.view(np.uint32) if g.dtype == np.int32 else g.astype(np.uint8) if g.dtype == np.bool_ else g
            assert same(g, e), f"call {c}: {nm}"
        gu = te.rollout_uniform(9, K)
        eu = ve.rollout_uniform(9, K)
        torch.cuda.synchronize()
        assert same(gu[0].cpu().numpy().view(np.uint32), eu[0]) and same(gu[1].cpu().numpy(), eu[1])
