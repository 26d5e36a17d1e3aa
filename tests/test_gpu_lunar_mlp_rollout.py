"""mgym_rollout_mlp for LunarLanderV3 through the persistent rollout launch (ll_roll.h, action sources MLP_RELU / MLP_TANH).  The reference for the
actions is modurl_gym_amd/csrc/mlp_policy.h compiled for the host (policy_header.header_actions) on the observation each environment holds before
the step; the reference for everything else is a second handle stepped with mgym_step.  Whole words, no tolerance, wind on.  Which form ran is read
from mgym_get_info's rollout_persistent_launches (the words are the same either way).  The handles of these tests set MGYM_LL_ROLLOUT_MLP=1, so both
activations go through the launch whatever the default is; test_default_form_of_each_activation checks the default (PERSISTENT_BY_DEFAULT)."""
import numpy as np
import pytest

import modurl_gym_amd as mg
from mlp_policy_ref import FAMILIES, RELU, TANH
from policy_header import GREEDY, check_lib, header_actions
from mlp_ref import normal_weights, packed
from words import same

pytestmark = pytest.mark.gpu

ACT_NAME = {RELU: "relu", TANH: "tanh"}
# the weight recipe and seeds of test_gpu_mlp_policy.py (chosen on the CPU for the first 300 environments of seed 11; every environment draws from
# (seed, global id), so they are the first 300 of a larger handle too)
IN_SCALE = (2.0, 2.0, 2.0, 2.0, 3.0, 2.0, 2.0, 2.0)
SEEDS = {(1, RELU): 87, (1, TANH): 12, (7, RELU): 3, (7, TANH): 0, (64, RELU): 0, (64, TANH): 0}
D, A, _ = FAMILIES["lunar_lander"]
ENV_SEED = 11
MODES = {"persistent": {"MGYM_LL_ROLLOUT_MIN_K": "8", "MGYM_LL_ROLLOUT_MLP": "1"}, "default_mlp": {"MGYM_LL_ROLLOUT_MIN_K": "8"}, "disabled": {"MGYM_LL_ROLLOUT": "0"},
         "large": {"MGYM_LL_ROLLOUT_MLP": "1"}}
# kRollMlpPersistent of lunar_lander.hip: the activations that run inside the launch without the knob (the ones measured faster there)
PERSISTENT_BY_DEFAULT = {RELU: False, TANH: False}


def weights(H, act):
    return normal_weights(np.random.default_rng(1000 + SEEDS[(H, act)]), D, A, H, IN_SCALE)


def make(monkeypatch, mode, n, auto_reset=True, limit=0, seed=ENV_SEED):
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    env = mg.VecEnv(mg.LUNARLANDER, n, seed=seed, enable_wind=True, auto_reset=auto_reset, max_episode_steps=limit)
    for k in MODES[mode]:
        monkeypatch.delenv(k)
    info = env.info()
    assert info["rollout"] == ("k_steps" if mode == "disabled" else "persistent_launch")
    if mode in ("persistent", "default_mlp"):
        assert info["rollout_min_k"] == "8"
    return env


def launches(env):
    return int(env.info()["rollout_persistent_launches"])


@pytest.fixture(scope="module")
def header():
    check_lib()   # compiled once, before the first GPU call
    return header_actions


class Loop:
    """the stepping loop: a second handle, the header's action for the observation it holds, mgym_step"""

    def __init__(self, header, n, auto_reset=True, limit=0, seed=ENV_SEED):
        self.header = header
        self.env = mg.VecEnv(mg.LUNARLANDER, n, seed=seed, enable_wind=True, auto_reset=auto_reset, max_episode_steps=limit)
        self.obs = self.env.reset()

    def check(self, got, H, act, what, facts=None):
        """every step of one call's outputs (actions, obs, reward, done, truncated) against header + mgym_step"""
        w = weights(H, act)
        pol = packed(w)
        acts, gobs, grew, gdone, gtrunc = got
        for t in range(acts.shape[0]):
            a = self.header(D, A, 1, act, GREEDY, (H,), pol, self.obs)[0]
            assert np.array_equal(acts[t], a), f"{what} step {t}: actions"
            o, r, d, tr = self.env.step(a)
            for g, e, nm in zip((gobs[t], grew[t], gdone[t], gtrunc[t]), (o, r, d, tr), ("obs", "reward", "done", "truncated")):
                assert same(g, e), f"{what} step {t}: {nm}"
            if facts is not None:
                facts.see(w, self.obs, a, o, d, tr)
            self.obs = o

    def follow(self, acts):
        for a in acts:
            self.obs = self.env.step(a)[0]

    def check_end(self, env, limit=0):
        assert same(env.get_state(), self.env.get_state())
        assert same(env.observation(), self.obs)
        assert env.episode_count() == self.env.episode_count()
        if limit:
            assert np.array_equal(env.elapsed_steps(), self.env.elapsed_steps())


class Facts:
    """what the weights reach, gathered from the GPU's own outputs"""

    def __init__(self):
        self.actions, self.pos, self.neg, self.legs, self.done, self.trunc = set(), 0, 0, 0, 0, 0

    def see(self, w, obs_before, acts, obs, done, trunc):
        with np.errstate(all="ignore"):
            pre = w[0].astype(np.float64) @ obs_before.astype(np.float64) + w[1].astype(np.float64)[:, None]
        self.pos += int((pre > 1e-3).sum())
        self.neg += int((pre < -1e-3).sum())
        self.actions |= set(int(v) for v in np.unique(acts))
        self.legs += int((obs[6:8] > 0).sum())
        self.done += int(done.sum())
        self.trunc += int(trunc.sum())


CASES = [(4096, 64, RELU, True, 0), (4096, 7, TANH, True, 0), (97, 64, TANH, True, 0), (97, 1, RELU, False, 0), (1, 7, RELU, True, 0), (300, 7, TANH, True, 60)]


@pytest.mark.parametrize("n,H,act,auto_reset,limit", [pytest.param(*c, id=f"n{c[0]}-H{c[1]}-{ACT_NAME[c[2]]}-{'auto' if c[3] else 'manual'}-limit{c[4]}") for c in CASES])
def test_persistent_form_equals_the_header_and_a_stepping_loop(monkeypatch, header, n, H, act, auto_reset, limit):
    """1 is one lane, 97 leaves partial 32- and 64-lane batches, 4096 fills every queue kind (touching, light, sub-step, reset)"""
    K, calls = 40, 4
    env = make(monkeypatch, "persistent", n, auto_reset, limit)
    loop = Loop(header, n, auto_reset, limit)
    assert same(env.reset(), loop.obs)
    facts = Facts()
    w = weights(H, act)
    for c in range(calls):
        before = launches(env)
        got = env.rollout_mlp(*w, K, activation=ACT_NAME[act])
        assert launches(env) == before + 1, "one persistent launch per call"
        loop.check(got, H, act, f"call {c}", facts)
    loop.check_end(env, limit)
    if n == 4096:
        assert facts.actions == set(range(A)), f"every action occurs: {facts.actions}"
        assert facts.pos > 0 and facts.neg > 0, "hidden pre-activations take both signs"
        assert facts.legs > 0 and facts.done > 100, "legs touch and more than 100 episodes finish"
    if limit:
        assert facts.trunc > 0, "the time limit truncates inside the launch"
    env.close(); loop.env.close()


def test_call_across_the_launch_split(monkeypatch, header):
    """K = 250 runs as launches of 240 and 10 steps: t and the next-action words carry across"""
    n, K = 97, 250
    env = make(monkeypatch, "persistent", n)
    loop = Loop(header, n)
    assert same(env.reset(), loop.obs)
    before = launches(env)
    got = env.rollout_mlp(*weights(7, RELU), K, activation="relu")
    assert launches(env) == before + 2
    loop.check(got, 7, RELU, "K = 250")
    loop.check_end(env)
    env.close(); loop.env.close()


def eager_words(monkeypatch, n, H, act, K, calls, seed):
    """the outputs of `calls` persistent calls of K steps on a fresh handle, and its final state"""
    env = make(monkeypatch, "persistent", n, seed=seed)
    env.reset()
    w = weights(H, act)
    before = launches(env)
    out = [env.rollout_mlp(*w, K, activation=ACT_NAME[act]) for _ in range(calls)]
    assert launches(env) == before + calls
    words = [np.concatenate([o[k] for o in out]) for k in range(5)]
    state = env.get_state()
    env.close()
    return words, state


@pytest.mark.parametrize("mode,K,calls", [("persistent", 5, 8), ("disabled", 40, 1)])
def test_k_step_form_stays_below_min_k_and_when_disabled(monkeypatch, mode, K, calls):
    n, H, act = 97, 7, TANH
    exp, exp_state = eager_words(monkeypatch, n, H, act, 40, 1, 19)
    env = make(monkeypatch, mode, n, seed=19)
    env.reset()
    w = weights(H, act)
    before = launches(env)
    out = [env.rollout_mlp(*w, K, activation="tanh") for _ in range(calls)]
    assert launches(env) == before, "no persistent launch"
    for k, nm in enumerate(("actions", "obs", "reward", "done", "truncated")):
        assert same(np.concatenate([o[k] for o in out]), exp[k]), nm
    assert same(env.get_state(), exp_state)
    env.close()


@pytest.mark.parametrize("act", [RELU, TANH], ids=["relu", "tanh"])
def test_default_form_of_each_activation(monkeypatch, act):
    """without MGYM_LL_ROLLOUT_MLP a call is a persistent launch only for an activation that earned it; the same words either way"""
    n, H, K = 97, 7, 40
    exp, exp_state = eager_words(monkeypatch, n, H, act, K, 1, 19)
    env = make(monkeypatch, "default_mlp", n, seed=19)
    env.reset()
    before = launches(env)
    got = env.rollout_mlp(*weights(H, act), K, activation=ACT_NAME[act])
    assert launches(env) == before + (1 if PERSISTENT_BY_DEFAULT[act] else 0)
    for g, e, nm in zip(got, exp, ("actions", "obs", "reward", "done", "truncated")):
        assert same(g, e), nm
    assert same(env.get_state(), exp_state)
    env.close()


def test_captured_call_stays_the_k_step_form_and_freezes_the_weights(monkeypatch):
    n, K, H = 512, 16, 64
    exp, exp_state = eager_words(monkeypatch, n, H, TANH, K, 2, 29)
    cap = make(monkeypatch, "persistent", n, seed=29)
    cap.reset()
    pol = packed(weights(H, TANH))
    bufs = [mg.DeviceArray((K, n), np.uint32), mg.DeviceArray((K, D, n), np.float32), mg.DeviceArray((K, n), np.float32),
            mg.DeviceArray((K, n), np.uint8), mg.DeviceArray((K, n), np.uint8)]
    before = launches(cap)
    g = cap.graph_capture(lambda: cap.rollout_mlp_device(pol, H, "tanh", K, *bufs))
    pol[:] = 0.0
    try:
        for rep in range(2):
            cap.graph_launch(g)
            cap.sync()
            for b, e, nm in zip(bufs, exp, ("actions", "obs", "reward", "done", "truncated")):
                assert same(b.numpy(), e[rep * K:(rep + 1) * K]), f"replay {rep}: {nm}"
    finally:
        cap.graph_destroy(g)
    assert launches(cap) == before, "a captured call records the K-step form"
    assert same(cap.get_state(), exp_state)
    cap.close()


def test_weights_are_per_call(monkeypatch, header):
    """two calls back to back with different weights and no synchronisation between them; the caller's arrays are zeroed as soon as each call returns"""
    n, K = 300, 16
    env = make(monkeypatch, "persistent", n)
    loop = Loop(header, n)
    assert same(env.reset(), loop.obs)
    calls = [(7, RELU), (64, TANH)]
    bufs = [[mg.DeviceArray((K, n), np.uint32), mg.DeviceArray((K, D, n), np.float32), mg.DeviceArray((K, n), np.float32),
             mg.DeviceArray((K, n), np.uint8), mg.DeviceArray((K, n), np.uint8)] for _ in calls]
    before = launches(env)
    for (H, act), b in zip(calls, bufs):
        pol = packed(weights(H, act))
        env.rollout_mlp_device(pol, H, ACT_NAME[act], K, *b)
        pol[:] = 0.0
    env.sync()
    assert launches(env) == before + 2
    for c, ((H, act), b) in enumerate(zip(calls, bufs)):
        loop.check([x.numpy() for x in b], H, act, f"call {c}")
    loop.check_end(env)
    env.close(); loop.env.close()


def test_interleaving_with_the_other_entry_points(monkeypatch, header):
    n = 300
    env = make(monkeypatch, "persistent", n, seed=23)
    loop = Loop(header, n, seed=23)
    rng = np.random.default_rng(1)
    assert same(env.reset(), loop.obs)
    lin = rng.normal(0, 1, A * (D + 1)).astype(np.float32)
    before = launches(env)

    def equal():
        assert same(env.get_state(), loop.env.get_state())
        assert same(env.observation(), loop.obs)

    def mlp(H, act, k):
        loop.check(env.rollout_mlp(*weights(H, act), k, activation=ACT_NAME[act]), H, act, f"H={H} K={k}")
        equal()

    mlp(7, RELU, 16)
    tab = rng.integers(0, A, (12, n)).astype(np.uint32)
    env.rollout(tab); loop.follow(tab); equal()
    mlp(64, TANH, 9)
    loop.follow(env.rollout_linear(lin, 16)[0]); equal()
    loop.follow(env.rollout_uniform(5, 16)[0]); equal()
    a = rng.integers(0, A, n).astype(np.uint32)
    env.step(a); loop.follow([a]); equal()
    m = (rng.random(n) < 0.3).astype(np.uint8)
    env.reset(m); loop.env.reset(m); loop.obs = loop.env.observation(); equal()
    mlp(64, RELU, 20)
    st = loop.env.get_state()
    env.set_state(st); loop.env.set_state(st); loop.obs = loop.env.observation(); equal()
    mlp(7, TANH, 12)
    assert launches(env) == before + 7, "four hidden-layer calls, one table, one linear, one uniform: each K >= 8 is one persistent launch"
    env.close(); loop.env.close()


def test_large_population_equals_steps(monkeypatch, header):
    """the population's own knobs at 262 144 environments (rollout_min_k 8, the grid of a full machine), as test_linear_rollout_large_population_equals_steps"""
    n, K, H = 262144, 16, 7
    env = make(monkeypatch, "large", n, seed=3)
    assert env.info()["rollout_min_k"] == "8"
    loop = Loop(header, n, seed=3)
    assert same(env.reset(), loop.obs)
    before = launches(env)
    got = env.rollout_mlp(*weights(H, RELU), K, activation="relu")
    assert launches(env) == before + 1
    loop.check(got, H, RELU, "262144")
    assert same(env.get_state(), loop.env.get_state())
    env.close(); loop.env.close()


def test_never_reset_reports_not_reset_through_the_persistent_form(monkeypatch):
    n, K = 8, 16
    env = make(monkeypatch, "persistent", n, auto_reset=False)
    acts = mg.DeviceArray.from_numpy(np.full((K, n), 0xFFFFFFFF, np.uint32))
    before = launches(env)
    env.rollout_mlp_device(packed(weights(7, RELU)), 7, "relu", K, acts)
    with pytest.raises(mg.NotResetError):
        env.sync()
    assert not acts.numpy().any(), "every action word written is 0"
    assert launches(env) == before + 1
    env.close()
