"""The episode time limit (mgym_config::max_episode_steps, include/mgym.h) on the GPU, for MountainCar, MountainCarContinuous and
LunarLander, through every entry point that steps: mgym_step, mgym_rollout, mgym_rollout_linear, mgym_rollout_uniform and replays of
captured graphs.  The checker is the unchanged CPU oracle inside the Python TimeLimit wrapper of tests/time_limit_ref.py (after every
oracle step elapsed += 1, truncated = elapsed >= limit, `done` untouched; with auto-reset the envs with either flag are reset and their
reset observation replaces the step's).  Every comparison is bit for bit."""
import subprocess

import numpy as np
import pytest

import modurl_gym_amd as mg
import native_build
from oracle import oracle as ora
from device_buffers import CallBuffers
from families import BY_KIND
from time_limit_ref import TimeLimitRef
from words import same

pytestmark = pytest.mark.gpu
NAMES = ("obs", "reward", "done", "truncated")

# ---- MountainCar / MountainCarContinuous ------------------------------------------------------------------------------------------
# The velocity-following linear policy.  Discrete: rows (w_position, w_velocity, bias); the scores are -v, -1e30, v, so the argmax (the
# first of equal ones) is action 2 for velocity > 0 and action 0 otherwise.  Continuous: the force is 1e3 v (the step clamps it).
POL_D = np.array([0, -1, 0, 0, 0, -1e30, 0, 1, 0], np.float32)
POL_C = np.array([0, 1e3, 0], np.float32)
MC_SEED, MC_STEPS, MC_K, RESET_EVERY = 5, 400, 16, 32
ALL_OFF = (4, 4, 4, 1, 3)   # every caller buffer off its 16-byte alignment: the scalar kernels


def mc_policy(kind, obs):
    if kind == mg.MOUNTAINCAR_CONT:
        return (np.float32(0.0) * obs[0] + np.float32(1e3) * obs[1]) + np.float32(0.0)
    return np.where(obs[1] > 0, 2, 0).astype(np.uint32)


_median = {}


def mc_median_length(n):
    """MountainCarContinuous under that policy: the median episode length the ORACLE shows over 400 steps (fused reset on done), so that a
    limit equal to it ends about half of the episodes by `done` first, half by the limit, and some by both on the same step."""
    if n not in _median:
        ref = ora.OracleVec(ora.MOUNTAINCAR_CONT, n, seed=MC_SEED)
        obs, length, lens = ref.reset(), np.zeros(n, np.int64), []
        for _ in range(MC_STEPS):
            o, _, d, _ = ref.step(mc_policy(mg.MOUNTAINCAR_CONT, obs))
            length += 1
            m = d.astype(bool)
            if m.any():
                lens += list(length[m])
                o = np.where(m[None, :], ref.reset(d), o)
                length[m] = 0
            obs = o
        _median[n] = int(np.median(lens))
    return _median[n]


def mc_limit(kind, limit, n):
    return mc_median_length(n) if (kind == mg.MOUNTAINCAR_CONT and limit == 100) else limit


_mc_expected = {}


def mc_expected(kind, n, limit, auto_reset):
    """oracle + wrapper under the policy: per step (actions, obs, reward, done, truncated); without auto-reset the caller resets what has
    finished (done | truncated) after every RESET_EVERY-th step, so environments run on past their limit in between."""
    key = (kind, n, limit, auto_reset)
    if key not in _mc_expected:
        w = TimeLimitRef(ora.OracleVec(BY_KIND[kind].okind, n, seed=MC_SEED), limit, auto_reset)
        obs, steps, elapsed = w.reset(), [], []
        for t in range(MC_STEPS):
            a = mc_policy(kind, obs)
            o, r, d, tr = w.step(a)
            steps.append((a, o, r, d, tr))
            obs = o
            if not auto_reset and t % RESET_EVERY == RESET_EVERY - 1:
                m = (d | tr).astype(np.uint8)
                obs = np.where(m.astype(bool)[None, :], w.reset(m), obs)
            elapsed.append(w.elapsed.copy())
        _mc_expected[key] = (obs.copy(), steps, dict(w.kinds), w.finished, elapsed)
    return _mc_expected[key]


def mc_classes_ok(kind, limit, kinds):
    """the ending classes the window must hold, a condition on the oracle side.  No episode of either family ends within 7 steps (limit 7:
    truncations only); limit 100 (discrete: 40 % of the episodes end by `done` before step 100, 112 reach the goal exactly on it) and the
    continuous family's median limit must show all three; limit 200: whatever the family's lengths give, recorded by episode_count."""
    if limit == 7:
        return kinds["trunc_only"] > 0 and kinds["done_only"] == 0 and kinds["both"] == 0
    if limit == 200:
        return kinds["done_only"] > 0
    return kinds["done_only"] > 0 and kinds["trunc_only"] > 0 and kinds["both"] > 0


def mc_env(kind, n, limit, auto_reset, **kw):
    env = mg.VecEnv(kind, n, seed=MC_SEED, auto_reset=auto_reset, max_episode_steps=limit, **kw)
    assert env.info()["max_episode_steps"] == str(limit)
    return env


def caller_reset(env, t, auto_reset, d, tr):
    if not auto_reset and t % RESET_EVERY == RESET_EVERY - 1:
        dd, dt = mg.DeviceArray.from_numpy(np.ascontiguousarray(d, np.uint8)), mg.DeviceArray.from_numpy(np.ascontiguousarray(tr, np.uint8))
        env.reset_done_device(dd, dt)      # mgym_reset_done(done, truncated): starts the episodes the wrapper starts
        env.sync()


MC_CASES = [(k, n, lim, ar) for k in (mg.MOUNTAINCAR, mg.MOUNTAINCAR_CONT) for n in (4096, 4099) for lim in (7, 100, 200) for ar in (True, False)]


@pytest.mark.parametrize("kind,n,limit,auto_reset", MC_CASES)
def test_mountain_car_steps_and_graph_replays_equal_oracle_plus_wrapper(kind, n, limit, auto_reset):
    """mgym_step x 400 and 400 replays of ONE captured mgym_step (the count lives in device memory: a replay counts like a call).
    n = 4099 with misaligned caller buffers takes the scalar kernels, n = 4096 the 16-byte ones."""
    limit = mc_limit(kind, limit, n)
    final_obs, steps, kinds, finished, elapsed = mc_expected(kind, n, limit, auto_reset)
    assert mc_classes_ok(kind, limit if limit in (7, 200) else 100, kinds), kinds
    adt = np.float32 if kind == mg.MOUNTAINCAR_CONT else np.uint32
    for form in ("step", "graph"):
        env = mc_env(kind, n, limit, auto_reset)
        env.reset()
        b = CallBuffers(n, 2, adt, mis=ALL_OFF if n % 4 else (0,) * 5)
        graph = env.graph_capture(lambda: env.step_device(*b.pointers())) if form == "graph" else None
        for t, (a, eo, er, ed, et) in enumerate(steps):
            b.put_actions(a)
            if graph is not None:
                env.graph_launch(graph)
            else:
                env.step_device(*b.pointers())
            env.sync()
            for g, e, nm in zip(b.read(), (eo, er, ed, et), NAMES):
                assert same(g[0], e), f"{form} step {t}: {nm}"
            caller_reset(env, t, auto_reset, ed, et)
            if t in (6, 99, 250):
                assert np.array_equal(env.elapsed_steps(), elapsed[t]), f"{form} step {t}: elapsed"
        assert same(env.observation(), final_obs)
        assert env.episode_count() == finished      # an env-step with either flag counts once
        if graph is not None:
            env.graph_destroy(graph)
        env.close()


@pytest.mark.parametrize("kind,n,limit,auto_reset", MC_CASES)
def test_mountain_car_rollouts_equal_oracle_plus_wrapper(kind, n, limit, auto_reset):
    """mgym_rollout (K = 16, a table of the policy's actions) and mgym_rollout_linear (the policy on the device; n % 4 == 0 only), the count in
    registers across the K steps.  n = 4099 with misaligned buffers: the K-step form over the scalar kernels."""
    limit = mc_limit(kind, limit, n)
    final_obs, steps, kinds, finished, elapsed = mc_expected(kind, n, limit, auto_reset)
    adt = np.float32 if kind == mg.MOUNTAINCAR_CONT else np.uint32
    K = MC_K
    for form in ("table", "linear"):
        if form == "linear" and n % 4 != 0:
            continue
        env = mc_env(kind, n, limit, auto_reset)
        env.reset()
        b = CallBuffers(n, 2, adt, K, mis=ALL_OFF if n % 4 else (0,) * 5)
        for c in range(MC_STEPS // K):
            exp = steps[c * K:(c + 1) * K]
            if form == "table":
                b.put_actions(np.stack([s[0] for s in exp]))
                env.rollout_device(b.pointers()[0], K, *b.pointers()[1:])
                env.sync()
                got = b.read()
            else:
                acts, *got = env.rollout_linear(POL_C if kind == mg.MOUNTAINCAR_CONT else POL_D, K)
                assert same(acts.view(adt), np.stack([s[0] for s in exp])), f"{form} call {c}: actions"
            for k in range(K):
                for g, e, nm in zip((got[0][k], got[1][k], got[2][k], got[3][k]), exp[k][1:], NAMES):
                    assert same(g, e), f"{form} call {c} step {k}: {nm}"
            t = c * K + K - 1
            caller_reset(env, t, auto_reset, exp[-1][3], exp[-1][4])
            assert np.array_equal(env.elapsed_steps(), elapsed[t]), f"{form} call {c}: elapsed"
        assert same(env.observation(), final_obs)
        assert env.episode_count() == finished
        env.close()


@pytest.mark.parametrize("kind", [mg.MOUNTAINCAR, mg.MOUNTAINCAR_CONT])
@pytest.mark.parametrize("limit,auto_reset", [(7, True), (100, True), (7, False), (100, False)])
def test_mountain_car_uniform_rollout_equals_oracle_driven_by_the_same_draws(kind, limit, auto_reset):
    """mgym_rollout_uniform (include/mgym.h documents the draws, restated here with the oracle's Philox) against oracle + wrapper stepped with them.
    The window is 2 calls x 64 steps, and the uniform policy practically never reaches the goal: every ending here is a truncation (asserted: no
    `done` on the oracle side), which is what a limit is for under such a policy.  Limit 200 would not be reached within 128 steps and would test
    nothing in this form, so it is left out; limits 7 and 100, with and without auto-reset (without: truncated stays up from the limit on)."""
    n, K, base, seed = 4096, 64, 8192, 0x1234ABCD5678
    cont = kind == mg.MOUNTAINCAR_CONT
    env = mg.VecEnv(kind, n, seed=19, env_id_base=base, auto_reset=auto_reset, max_episode_steps=limit)
    w = TimeLimitRef(ora.OracleVec(BY_KIND[kind].okind, n, seed=19, env_id_base=base), limit, auto_reset)
    env.reset(), w.reset()
    for call in range(2):
        acts, obs, rew, done, trunc = env.rollout_uniform(seed, K)
        exp = np.zeros((K, n), np.uint32)
        for g0 in range(0, n, 4):
            gid = base + g0
            for blk in range(K if cont else K // 2):
                wd = ora.philox([gid & 0xFFFFFFFF, gid >> 32, call, 0x40000000 + blk], [seed & 0xFFFFFFFF, seed >> 32])
                for k in range(4):
                    if cont:
                        exp[blk, g0 + k] = np.float32(np.float32(int(wd[k]) >> 8) * np.float32(2.0 ** -23) - np.float32(1.0)).view(np.uint32)
                    else:
                        exp[2 * blk, g0 + k] = ((int(wd[k]) & 0xFFFF) * 3) >> 16
                        exp[2 * blk + 1, g0 + k] = ((int(wd[k]) >> 16) * 3) >> 16
        assert np.array_equal(acts, exp), f"call {call}: drawn actions"
        for t in range(K):
            eo, er, ed, et = w.step(exp[t].view(np.float32) if cont else exp[t])
            for g, e, nm in zip((obs[t], rew[t], done[t], trunc[t]), (eo, er, ed, et), NAMES):
                assert same(g, e), f"call {call} step {t}: {nm}"
        assert np.array_equal(env.elapsed_steps(), w.elapsed)
    assert w.kinds["trunc_only"] > 0 and w.kinds["done_only"] == 0 and w.kinds["both"] == 0
    assert env.episode_count() == w.finished


# ---- LunarLander ------------------------------------------------------------------------------------------------------------------
LL_N, LL_SEED, LL_STEPS = 4096, 11, 300


def ll_actions(steps=LL_STEPS, n=LL_N):
    rng = np.random.default_rng(LL_SEED)
    return [rng.integers(0, 4, n).astype(np.uint32) for _ in range(steps)]


_ll_expected = {}


def ll_expected(limit):
    """oracle + wrapper, wind on, auto-reset on, uniform actions: per step (obs, reward, done, truncated), and how the truncations fall"""
    if limit not in _ll_expected:
        w = TimeLimitRef(ora.OracleVec(ora.LUNARLANDER, LL_N, seed=LL_SEED, enable_wind=True), limit, True, nthreads=8)
        first = w.reset()
        steps, cls = [], {"free_flight": 0, "leg_on_ground": 0, "both_flags": 0}
        for a in ll_actions():
            out = w.step(a)
            steps.append(out)
            tr, dn = out[3].astype(bool), out[2].astype(bool)
            leg = (w.final_obs[6] > 0) | (w.final_obs[7] > 0)
            cls["free_flight"] += int((tr & ~dn & ~leg).sum())
            cls["leg_on_ground"] += int((tr & ~dn & leg).sum())
            cls["both_flags"] += int((tr & dn).sum())
        _ll_expected[limit] = (first, steps, cls, w.finished)
    return _ll_expected[limit]


def ll_classes_ok(limit, cls):
    """a condition on the inputs (the oracle side), so that a drifting seed fails loudly instead of testing nothing: at elapsed = 40 every live
    environment is in free flight (no episode of this family is that short), at elapsed = 100 truncations also meet environments with a leg on the
    ground and environments that finish on that very step"""
    if limit == 40:
        return cls["free_flight"] > 20000 and cls["leg_on_ground"] == 0 and cls["both_flags"] == 0
    return cls["free_flight"] > 0 and cls["leg_on_ground"] > 0 and cls["both_flags"] > 0


def ll_env(monkeypatch, limit, block=0, rollout_min_k=None, auto_reset=True, n=LL_N, seed=LL_SEED):
    if block:
        monkeypatch.setenv("MGYM_LL_GENERAL_BLOCK", str(block))
    if rollout_min_k:
        monkeypatch.setenv("MGYM_LL_ROLLOUT_MIN_K", str(rollout_min_k))
    env = mg.VecEnv(mg.LUNARLANDER, n, seed=seed, enable_wind=True, auto_reset=auto_reset, max_episode_steps=limit)
    monkeypatch.delenv("MGYM_LL_GENERAL_BLOCK", raising=False)
    monkeypatch.delenv("MGYM_LL_ROLLOUT_MIN_K", raising=False)
    return env


@pytest.mark.parametrize("limit", [40, 100])
@pytest.mark.parametrize("block", [32, 64])
def test_lunar_lander_steps_equal_oracle_plus_wrapper(monkeypatch, limit, block):
    """mgym_step x 300 in both contact-block layouts (32: the single-launch step; 64: free-flight and contact kernels of their own)"""
    first, steps, cls, finished = ll_expected(limit)
    assert ll_classes_ok(limit, cls), cls
    env = ll_env(monkeypatch, limit, block)
    info = env.info()
    assert info["contact_block"] == str(block) and info["max_episode_steps"] == str(limit)
    assert same(env.reset(), first)
    for t, (a, exp) in enumerate(zip(ll_actions(), steps)):
        for g, e, nm in zip(env.step(a), exp, NAMES):
            assert same(g, e), f"block {block} step {t}: {nm}"
    assert env.episode_count() == finished
    env.close()


@pytest.mark.parametrize("limit", [40, 100])
@pytest.mark.parametrize("K", [16, 64])
def test_lunar_lander_persistent_rollout_equals_oracle_plus_wrapper(monkeypatch, limit, K):
    first, steps, cls, _ = ll_expected(limit)
    assert ll_classes_ok(limit, cls), cls
    env = ll_env(monkeypatch, limit, rollout_min_k=8)
    info = env.info()
    assert info["rollout"] == "persistent_launch" and int(info["rollout_min_k"]) <= K      # the form that runs for K >= rollout_min_k outside a capture
    assert same(env.reset(), first)
    acts = ll_actions()
    finished = 0
    for c in range(LL_STEPS // K if K == 16 else 4):
        got = env.rollout(np.stack(acts[c * K:(c + 1) * K]))
        for k in range(K):
            for g, e, nm in zip((got[0][k], got[1][k], got[2][k], got[3][k]), steps[c * K + k], NAMES):
                assert same(g, e), f"K {K} call {c} step {k}: {nm}"
            finished += int((steps[c * K + k][2] | steps[c * K + k][3]).sum())
    assert env.episode_count() == finished
    env.close()


def test_lunar_lander_captured_rollout_replays_equal_oracle_plus_wrapper(monkeypatch):
    """a captured mgym_rollout records K steps (include/mgym.h); its replays count and truncate like eager calls"""
    limit, K = 40, 16
    first, steps, _, _ = ll_expected(limit)
    env = ll_env(monkeypatch, limit, rollout_min_k=8)
    assert same(env.reset(), first)
    acts = ll_actions()
    d_act = mg.DeviceArray((K, LL_N), np.uint32)
    d_obs, d_rew = mg.DeviceArray((K, 8, LL_N), np.float32), mg.DeviceArray((K, LL_N), np.float32)
    d_done, d_trunc = mg.DeviceArray((K, LL_N), np.uint8), mg.DeviceArray((K, LL_N), np.uint8)
    graph = env.graph_capture(lambda: env.rollout_device(d_act, K, d_obs, d_rew, d_done, d_trunc))
    truncated = 0
    for c in range(6):   # 96 steps: the truncations of elapsed = 40 and 80
        d_act.copy_from(np.stack(acts[c * K:(c + 1) * K]))
        env.graph_launch(graph)
        env.sync()
        got = (d_obs.numpy(), d_rew.numpy(), d_done.numpy(), d_trunc.numpy())
        for k in range(K):
            for g, e, nm in zip((got[0][k], got[1][k], got[2][k], got[3][k]), steps[c * K + k], NAMES):
                assert same(g, e), f"replay {c} step {k}: {nm}"
        truncated += int(got[3].sum())
    assert truncated == 2 * LL_N
    env.graph_destroy(graph)
    env.close()


def _ll_uniform_actions(seed, call, t, n):
    a = np.zeros(n, np.uint32)
    for g0 in range(0, n, 4):
        wd = ora.philox([g0, 0, call, 0x40000000 + t // 16], [seed & 0xFFFFFFFF, seed >> 32])
        for k in range(4):
            a[g0 + k] = (int(wd[k]) >> (2 * (t % 16))) & 3
    return a


LL_POL = np.zeros((4, 9), np.float32)   # (the weights of tests/test_gpu_lunar_policy.py: all four actions, leg contacts, many finished episodes)
LL_POL[0, 6] = 2.0; LL_POL[0, 7] = 2.0
LL_POL[1, 4] = 3.0; LL_POL[1, 5] = 1.5; LL_POL[1, 8] = -0.1
LL_POL[2, 1] = -0.5; LL_POL[2, 3] = -4.0; LL_POL[2, 8] = -0.6
LL_POL[3, 4] = -3.0; LL_POL[3, 5] = -1.5; LL_POL[3, 8] = -0.1


def _ll_linear_actions(obs):
    a, best = np.zeros(obs.shape[1], np.uint32), None
    for j in range(4):
        s = LL_POL[j, 0] * obs[0]
        for q in range(1, 8):
            s = s + LL_POL[j, q] * obs[q]
        s = s + LL_POL[j, 8]
        if j == 0:
            best = s
        else:
            m = s > best
            best = np.where(m, s, best)
            a[m] = j
    return a


@pytest.mark.parametrize("limit", [40, 100])
@pytest.mark.parametrize("policy", ["uniform", "linear"])
def test_lunar_lander_policy_rollouts_equal_step_loop_and_oracle_plus_wrapper(monkeypatch, policy, limit):
    """mgym_rollout_uniform / mgym_rollout_linear, K = 64, as the persistent launch, against a loop of mgym_step on a second handle (the K-step
    form's words) and against oracle + wrapper, both driven by the actions the documented policies give"""
    K, pseed = 64, 0xFEEDC0DE12345
    env = ll_env(monkeypatch, limit, rollout_min_k=8)
    info = env.info()
    assert info["rollout"] == "persistent_launch" and int(info["rollout_min_k"]) <= K
    loop = ll_env(monkeypatch, limit)
    w = TimeLimitRef(ora.OracleVec(ora.LUNARLANDER, LL_N, seed=LL_SEED, enable_wind=True), limit, True, nthreads=8)
    obs = w.reset()
    assert same(env.reset(), obs) and same(loop.reset(), obs)
    for call in range(2):
        got = env.rollout_uniform(pseed, K) if policy == "uniform" else env.rollout_linear(LL_POL.ravel(), K)
        for t in range(K):
            a = _ll_uniform_actions(pseed, call, t, LL_N) if policy == "uniform" else _ll_linear_actions(obs)
            assert np.array_equal(got[0][t], a), f"call {call} step {t}: actions"
            exp, stepped = w.step(a), loop.step(a)
            for g, s, e, nm in zip((got[1][t], got[2][t], got[3][t], got[4][t]), stepped, exp, NAMES):
                assert same(s, e), f"call {call} step {t}: stepping loop vs oracle + wrapper: {nm}"
                assert same(g, e), f"call {call} step {t}: {nm}"
            obs = exp[0]
    assert w.kinds["trunc_only"] > 0
    assert np.array_equal(env.elapsed_steps(), w.elapsed) and np.array_equal(loop.elapsed_steps(), w.elapsed)
    assert env.episode_count() == w.finished and loop.episode_count() == w.finished
    assert same(env.get_state(), loop.get_state())
    env.close(), loop.close()


# ---- non-interference, no auto-reset, checkpoints, host layers --------------------------------------------------------------------
def test_lunar_lander_limit_beyond_every_episode_changes_nothing(monkeypatch):
    """limit 1000 over 320 steps (no episode of the window is that long) against a handle without a limit: every word equal, truncated all 0 —
    through mgym_step and through the persistent rollout"""
    acts = ll_actions(320)
    for form in ("step", "rollout"):
        a_env, b_env = ll_env(monkeypatch, 1000, rollout_min_k=8), ll_env(monkeypatch, 0, rollout_min_k=8)
        assert b_env.info()["max_episode_steps"] == "0" and a_env.info()["max_episode_steps"] == "1000"
        assert same(a_env.reset(), b_env.reset())
        if form == "step":
            for t, a in enumerate(acts):
                ga, gb = a_env.step(a), b_env.step(a)
                assert all(same(x, y) for x, y in zip(ga, gb)), f"step {t}"
                assert not ga[3].any()
        else:
            for c in range(5):
                tab = np.stack(acts[c * 64:(c + 1) * 64])
                ga, gb = a_env.rollout(tab), b_env.rollout(tab)
                assert all(same(x, y) for x, y in zip(ga, gb)), f"rollout {c}"
                assert not ga[3].any()
        assert same(a_env.get_state(), b_env.get_state()) and a_env.episode_count() == b_env.episode_count()
        a_env.close(), b_env.close()


@pytest.mark.parametrize("kind", [mg.MOUNTAINCAR, mg.MOUNTAINCAR_CONT])
def test_mountain_car_largest_limit_changes_nothing(kind):
    n = 4096
    a_env, b_env = mc_env(kind, n, 65535, True), mc_env(kind, n, 0, True)
    obs = a_env.reset()
    assert same(obs, b_env.reset())
    for t in range(MC_STEPS):
        a = mc_policy(kind, obs)
        ga, gb = a_env.step(a), b_env.step(a)
        assert all(same(x, y) for x, y in zip(ga, gb)), f"step {t}"
        assert not ga[3].any()
        obs = ga[0]
    pol = POL_C if kind == mg.MOUNTAINCAR_CONT else POL_D
    assert all(same(x, y) for x, y in zip(a_env.rollout_linear(pol, 64), b_env.rollout_linear(pol, 64)))
    assert same(a_env.get_state(), b_env.get_state()) and a_env.episode_count() == b_env.episode_count() > 0


def test_lunar_lander_without_auto_reset_keeps_integrating_past_the_limit(monkeypatch):
    """after the limit truncated stays 1 and the state keeps integrating like the oracle's; mgym_reset_done(done, truncated) then starts the
    episodes the wrapper starts"""
    n, limit = 1024, 40
    env = ll_env(monkeypatch, limit, auto_reset=False, n=n, seed=17)
    w = TimeLimitRef(ora.OracleVec(ora.LUNARLANDER, n, seed=17, enable_wind=True), limit, False, nthreads=8)
    assert same(env.reset(), w.reset())
    rng = np.random.default_rng(4)
    for t in range(110):   # (the caller's resets come soon after the limit: a crashed lander is not stepped on for long)
        a = rng.integers(0, 4, n).astype(np.uint32)
        got, exp = env.step(a), w.step(a)
        for g, e, nm in zip(got, exp, NAMES):
            assert same(g, e), f"step {t}: {nm}"
        if 39 <= t < 60:
            assert exp[3].all()                   # past the limit, not reset: truncated on every step
        if 99 <= t < 104:
            assert exp[3].all()
        if t == 59 or t == 104:
            dd, dt = mg.DeviceArray.from_numpy(exp[2]), mg.DeviceArray.from_numpy(exp[3])
            do = mg.DeviceArray((8, n), np.float32)
            env.reset_done_device(dd, dt, do)
            env.sync()
            m = (exp[2] | exp[3]).astype(bool)
            ro = w.reset(m.astype(np.uint8))
            assert same(np.ascontiguousarray(do.numpy()[:, m]), np.ascontiguousarray(ro[:, m]))
            assert np.array_equal(env.elapsed_steps(), w.elapsed)
    assert env.episode_count() == w.finished
    env.close()


@pytest.mark.parametrize("kind", [mg.MOUNTAINCAR, mg.MOUNTAINCAR_CONT])
def test_mountain_car_checkpoint_carries_the_elapsed_count(kind):
    """state + elapsed exported from one handle mid-run and imported into a second one: both continue identically through the next truncations.
    The blob stays 3 columns and mgym_set_state alone starts the count at 0; mgym_set_elapsed_steps clamps to 65535."""
    n, limit = 4096, mc_limit(kind, 100, 4096)
    a_env, b_env = mc_env(kind, n, limit, True), mc_env(kind, n, limit, True)
    w = TimeLimitRef(ora.OracleVec(BY_KIND[kind].okind, n, seed=MC_SEED), limit, True)
    obs = a_env.reset()
    assert same(obs, w.reset())
    for t in range(150):
        a = mc_policy(kind, obs)
        got, exp = a_env.step(a), w.step(a)
        assert all(same(g, e) for g, e in zip(got, exp)), f"step {t}"
        obs = got[0]
    el = a_env.elapsed_steps()
    assert np.array_equal(el, w.elapsed) and 0 < int(el.max()) < limit
    blob = a_env.get_state()
    assert blob.shape == (3, n)
    b_env.set_state(blob)
    assert not b_env.elapsed_steps().any()          # mgym_set_state: the count starts at 0
    b_env.set_elapsed_steps(el)
    assert np.array_equal(b_env.elapsed_steps(), el)
    truncated = 0
    for t in range(150):
        a = mc_policy(kind, obs)
        ga, gb, exp = a_env.step(a), b_env.step(a), w.step(a)
        assert all(same(x, e) for x, e in zip(ga, exp)) and all(same(y, e) for y, e in zip(gb, exp)), f"continued step {t}"
        truncated += int(exp[3].sum())
        obs = ga[0]
    assert truncated > 0
    assert same(a_env.get_state(), b_env.get_state()) and np.array_equal(a_env.elapsed_steps(), b_env.elapsed_steps())
    b_env.set_elapsed_steps(np.full(n, 70000, np.uint32))
    assert (b_env.elapsed_steps() == 65535).all()
    cp = mg.VecEnv(mg.CARTPOLE, 8)
    with pytest.raises(mg.MgymError) as ei:         # CartPole's counter is blob column 4
        cp.elapsed_steps()
    assert ei.value.status == mg.envs.L.ERR_BAD_ARG


def test_lunar_lander_elapsed_count_is_the_step_counter_of_the_blob(monkeypatch):
    """LunarLander counts in the step counter the blob carries (column 25 = elapsed + 1: reset()'s implicit step(0) is not a caller's step).  Two
    handles run side by side to the same point (the blob does not carry the terrain, which belongs to the episode — include/mgym.h — so a state can
    only be imported into a handle whose environments are in the same episodes: a fresh handle will not do).  The second then has its count
    overwritten, imports the first one's exported state (mgym_set_state restores column 25) with the count overwritten once more, and gets the
    exported count through mgym_set_elapsed_steps; both continue identically through the next truncations (the counter also keys the dispersion
    draws, so a wrong restore shows in every word)."""
    n, limit = 2048, 100
    a_env, b_env = ll_env(monkeypatch, limit, n=n, seed=23), ll_env(monkeypatch, limit, n=n, seed=23)
    w = TimeLimitRef(ora.OracleVec(ora.LUNARLANDER, n, seed=23, enable_wind=True), limit, True, nthreads=8)
    first = w.reset()
    assert same(a_env.reset(), first) and same(b_env.reset(), first)
    assert not a_env.elapsed_steps().any()
    rng = np.random.default_rng(9)
    for t in range(70):
        a = rng.integers(0, 4, n).astype(np.uint32)
        ga, gb, exp = a_env.step(a), b_env.step(a), w.step(a)
        assert all(same(x, e) for x, e in zip(ga, exp)) and all(same(y, e) for y, e in zip(gb, exp)), f"step {t}"
    el = a_env.elapsed_steps()
    assert np.array_equal(el, w.elapsed)
    assert np.array_equal(a_env.get_state()[25].view(np.uint32), el + 1)
    b_env.set_elapsed_steps(np.zeros(n, np.uint32))
    assert np.array_equal(b_env.get_state()[25].view(np.uint32), np.ones(n, np.uint32))
    blob = a_env.get_state()
    b_env.set_state(blob)                            # export from one handle, import into the second: the blob brings the count back ...
    assert np.array_equal(b_env.elapsed_steps(), el)
    b_env.set_elapsed_steps(np.full(n, 5, np.uint32))
    assert np.array_equal(b_env.get_state()[25].view(np.uint32), np.full(n, 6, np.uint32))
    b_env.set_elapsed_steps(el)                      # ... and so does the exported count
    assert same(a_env.get_state(), b_env.get_state())
    a_env.set_state(blob), w.ref.set_state(blob)     # (every side through the same import, as tests/test_gpu_lunar_rollout.py does)
    truncated = 0
    for t in range(60):
        a = rng.integers(0, 4, n).astype(np.uint32)
        ga, gb, exp = a_env.step(a), b_env.step(a), w.step(a)
        assert all(same(x, e) for x, e in zip(ga, exp)) and all(same(y, e) for y, e in zip(gb, exp)), f"continued step {t}"
        truncated += int(exp[3].sum())
    assert truncated > 0
    a_env.close(), b_env.close()


def test_torch_env_with_a_limit_equals_the_ctypes_path():
    torch = pytest.importorskip("torch")
    n, limit = 4096, 7
    te = mg.TorchVecEnv(mg.MOUNTAINCAR, n, seed=MC_SEED, auto_reset=True, max_episode_steps=limit)
    ve = mc_env(mg.MOUNTAINCAR, n, limit, True)
    obs = ve.reset()
    assert same(te.reset().cpu().numpy(), obs)
    for t in range(20):
        a = mc_policy(mg.MOUNTAINCAR, obs)
        got = te.step(torch.from_numpy(a.astype(np.int32)).to(te.device))
        exp = ve.step(a)
        torch.cuda.synchronize()
        for g, e, nm in zip(got, exp, NAMES):
            g = g.cpu().numpy()
            assert same(g.astype(np.uint8) if g.dtype == np.bool_ else g, e), f"step {t}: {nm}"
        assert bool(exp[3].all()) == (t % limit == limit - 1)
        obs = exp[0]
    el = te.elapsed_steps()
    assert el.dtype == torch.int32 and el.device == te.device
    assert np.array_equal(el.cpu().numpy().astype(np.uint32), ve.elapsed_steps())
    te.close(), ve.close()


def test_single_env_classes_and_the_cpp_mirror_step_to_truncation():
    env = mg.MountainCarV0(seed=3, max_episode_steps=5)
    env.reset()
    infos = [env.step(np.uint32(1)) for _ in range(5)]
    assert [i.truncated for i in infos] == [False] * 4 + [True] and not any(i.done for i in infos)
    env.close()
    ll = mg.LunarLanderV3(seed=3, max_episode_steps=3)
    ll.reset()
    assert [ll.step(np.uint32(0)).truncated for _ in range(4)] == [False, False, True, True]   # no auto-reset: it stays up
    ll.close()
    exe = native_build.program("time_limit_mirror_test.cpp", base=(), extra=("-O1", "-std=c++17"), link=native_build.MGYM_LINK)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "time limit mirror ok" in r.stdout
