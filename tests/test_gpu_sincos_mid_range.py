"""Both environments stepped on the device at the 34 angles where mgym_math.h's sin / cos once differed from glibc
(tests/sincos_mid_range.py), word for word against the oracle, which calls glibc.  CartPole: theta set to each angle in all four
<is_euler, sutton_barto> variants, through the vec4 step kernel, the scalar one, mgym_rollout and the linear / uniform policy
rollouts, with and without auto-reset.  LunarLander: a reset state turned so that the lander's angle is each of them, in free
flight, every action, through mgym_step's free-flight and general paths and the persistent mgym_rollout."""
import numpy as np
import pytest

import modurl_gym_amd as mg
from oracle import oracle as ora
from sincos_mid_range import ANGLES, rotate_lander

pytestmark = pytest.mark.gpu


def words(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_words(got, exp, what):
    for g, e, nm in zip(got, exp, ("obs", "reward", "done", "truncated")):
        g, e = words(np.asarray(g)), words(np.asarray(e))
        if not np.array_equal(g, e):
            bad = np.argwhere(g != e)
            raise AssertionError(f"{what}{nm}: {len(bad)} words differ, first at {bad[0].tolist()}: {g[tuple(bad[0])]:#x} vs {e[tuple(bad[0])]:#x}")


# ------------------------------------------------------------------------------------------------ CartPole -----------
CP_PATHS = ("step_vec4", "step_scalar", "rollout", "rollout_linear", "rollout_uniform")


def _cartpole_pair(n, euler, sb, auto_reset):
    env = mg.VecEnv(mg.CARTPOLE, n, seed=29, auto_reset=auto_reset, is_euler=euler, sutton_barto_reward=sb)
    ref = ora.OracleVec(ora.CARTPOLE, n, seed=29, is_euler=euler, sutton_barto_reward=sb)
    env.reset(), ref.reset()
    s = ref.get_state()
    rng = np.random.default_rng(31)
    s[0] = rng.uniform(-1.0, 1.0, n)
    s[1] = rng.uniform(-0.5, 0.5, n)
    s[2] = np.resize(ANGLES, n)                                             # every angle at least 4 times
    s[3] = np.resize(np.array([0.0, 1e-3, -0.05, 0.3], np.float32), n)      # theta_dot small: theta stays in the range for a while
    s[2, -4:] = rng.uniform(-0.1, 0.1, 4)                                   # a few live poles beside them
    ref.set_state(s), env.set_state(s)
    assert np.array_equal(words(env.get_state()), words(ref.get_state()))
    return env, ref


def _ref_step(ref, a, auto_reset):
    o, r, d, t = ref.step(a)
    if auto_reset:
        m = (d | t).astype(np.uint8)
        ref.reset(mask=m)
        o = ref.get_state()[:4]
    return o, r, d, t


@pytest.mark.parametrize("path", CP_PATHS)
@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("euler,sb", [(True, False), (True, True), (False, False), (False, True)])
def test_cartpole_at_the_mid_range_angles_equals_oracle(euler, sb, auto_reset, path):
    n = 4 * len(ANGLES) + (1 if path == "step_scalar" else 0)   # n % 4 != 0: the scalar step kernel
    K = 10
    env, ref = _cartpole_pair(n, euler, sb, auto_reset)
    rng = np.random.default_rng(37)
    if path in ("step_vec4", "step_scalar"):
        for t in range(K):
            a = rng.integers(0, 2, n).astype(np.uint32)
            assert_words(env.step(a), _ref_step(ref, a, auto_reset), f"step {t}: ")
    elif path == "rollout":
        a = rng.integers(0, 2, (K, n)).astype(np.uint32)
        got = env.rollout(a)
        for t in range(K):
            assert_words([x[t] for x in got], _ref_step(ref, a[t], auto_reset), f"rollout step {t}: ")
    elif path == "rollout_uniform":
        acts, *got = env.rollout_uniform(0x5EED1234, K)
        for t in range(K):
            assert_words([x[t] for x in got], _ref_step(ref, acts[t], auto_reset), f"uniform rollout step {t}: ")
        assert 0 < acts.sum() < acts.size
    else:
        pol = np.array([0.1, 0.5, -0.01, -1.0, 0.003], np.float32)
        obs = ref.get_state()[:4].copy()
        acts, *got = env.rollout_linear(pol, K)
        for t in range(K):
            lin = ((pol[0] * obs[0] + pol[1] * obs[1]) + pol[2] * obs[2]) + pol[3] * obs[3]   # f32: every operation rounded
            a = ((lin + pol[4]) > 0).astype(np.uint32)
            assert np.array_equal(acts[t], a), f"linear rollout step {t}: actions"
            exp = _ref_step(ref, a, auto_reset)
            assert_words([x[t] for x in got], exp, f"linear rollout step {t}: ")
            obs = np.asarray(exp[0]).copy()
    assert np.array_equal(words(env.get_state()), words(ref.get_state()))


def test_cartpole_mid_range_angles_reach_the_reduction_unchanged():
    """The angles above are stepped as set: the blob round trip keeps each word, and one step without auto-reset
    leaves theta = angle + tau * theta_dot (Euler), so the first step's sin / cos really were of these angles."""
    env, ref = _cartpole_pair(4 * len(ANGLES), True, False, False)
    s = env.get_state()
    assert np.array_equal(words(s[2, :-4]), words(np.resize(ANGLES, s.shape[1])[:-4]))
    assert np.all(np.abs(s[2, :-4]) > 16) and np.all(np.abs(s[2, :-4]) < 120)


# ------------------------------------------------------------------------------------------------ LunarLander --------
def _lunar_pair(n, general=False, rollout=False, monkeypatch=None):
    if general:
        monkeypatch.setenv("MGYM_LL_GENERAL_ONLY", "1")
    if rollout:
        monkeypatch.setenv("MGYM_LL_ROLLOUT_MIN_K", "8")
    env = mg.VecEnv(mg.LUNARLANDER, n, seed=43)
    monkeypatch.delenv("MGYM_LL_GENERAL_ONLY", raising=False)
    monkeypatch.delenv("MGYM_LL_ROLLOUT_MIN_K", raising=False)
    ref = ora.OracleVec(ora.LUNARLANDER, n, seed=43)
    assert np.array_equal(words(env.reset()), words(ref.reset()))
    s = ref.get_state()
    for i in range(n):
        rotate_lander(s, i, ANGLES[(i // 4) % len(ANGLES)])
    ref.set_state(s), env.set_state(s)
    assert np.array_equal(words(env.get_state()), words(ref.get_state()))
    assert np.array_equal(words(env.get_state()[2]), words(np.repeat(ANGLES, 4)[:n]))
    return env, ref


@pytest.mark.parametrize("mode", ["free_flight_path", "general_path", "persistent_rollout"])
def test_lunar_lander_at_the_mid_range_angles_equals_oracle(mode, monkeypatch):
    n, K = 4 * len(ANGLES), 8        # each angle with each of the four actions
    env, ref = _lunar_pair(n, general=mode == "general_path", rollout=mode == "persistent_rollout", monkeypatch=monkeypatch)
    a = np.tile(np.arange(4, dtype=np.uint32), len(ANGLES))
    if mode == "persistent_rollout":
        assert env.info()["rollout"] == "persistent_launch"
        got = env.rollout(np.tile(a, (K, 1)))
        steps = [[x[t] for x in got] for t in range(K)]
    else:
        steps = [env.step(a) for _ in range(K)]
    for t in range(K):
        exp = ref.step(a)
        assert_words(steps[t], exp, f"{mode} step {t}: ")
        assert not exp[2].any(), f"step {t}: a lander left free flight"   # every step compared is a free-flight step
    assert np.array_equal(words(env.get_state()), words(ref.get_state()))
