"""CartPole fused auto-reset: the draw pass gives every finished env of a wave two lanes (one Philox evaluation each), so
one pass holds 32 finished envs and a wave with more takes further passes.  Forces exact per-wave finished counts on
both sides of every pass boundary (0, 1, 31, 32, 33, 63, 64, 65, 128, a whole wave) through the step kernel at each
lane shape the host launches and through the fused rollout, against the CPU oracle bit for bit, finished-episode
counter included."""
import numpy as np
import pytest

import modurl_gym_amd as mg
from oracle import oracle as ora

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 31, 32, 33, 63, 64, 65, 128, 256]   # finished envs per 256-env wave (4 envs per lane)
COUNTS_SCALAR = [0, 1, 31, 32, 33, 63, 64]          # per 64-env wave (1 env per lane)


def force(s, rng, first, span, count):
    """Make `count` envs of [first, first + span) finish on the next step: half leave the track (done), half reach
    step 500 (truncated).  Picked at random, so the list order crosses lanes and the 4 envs of a lane."""
    idx = first + rng.choice(span, count, replace=False)
    half = count // 2
    s[0, idx[:half]] = np.where(rng.random(half) < 0.5, 3.0, -3.0).astype(np.float32)
    s[4, idx[half:]] = np.full(count - half, 499, np.uint32).view(np.float32)


def check_step(env, ref, n, wave, counts, steps=3):
    rng = np.random.default_rng(11)
    env.reset(), ref.reset()
    total = 0
    for t in range(steps):
        s = ref.get_state()
        per_wave = list(np.roll(counts, t))
        tail = n - len(counts) * wave   # a partial last wave finishes whole
        if tail:
            per_wave.append(tail)
        for w, c in enumerate(per_wave):
            force(s, rng, w * wave, min(wave, n - w * wave), c)
        ref.set_state(s), env.set_state(s)
        a = rng.integers(0, 2, n).astype(np.uint32)
        got, exp = env.step(a), ref.step(a)
        for g, e, nm in zip(got[1:], exp[1:], ("reward", "done", "truncated")):
            assert np.array_equal(g, e), f"step {t}: {nm}"
        m = exp[2] | exp[3]
        fin = [int(m[w * wave:(w + 1) * wave].sum()) for w in range(len(per_wave))]
        assert fin == per_wave, f"step {t}: forced per-wave finished counts"
        total += int(m.sum())
        ref.reset(mask=m)
        post = ref.get_state()[:4]
        assert np.array_equal(got[0].view(np.uint32), post.view(np.uint32)), f"step {t}: post-reset obs_out"
        assert np.array_equal(env.observation().view(np.uint32), post.view(np.uint32)), f"step {t}: engine state"
    assert np.array_equal(env.get_state().view(np.uint32), ref.get_state().view(np.uint32))
    assert env.episode_count() == total


@pytest.mark.parametrize("block", [64, 128, 256])
def test_step_kernel_reset_passes_vec4(block, monkeypatch):
    monkeypatch.setenv("MGYM_CARTPOLE_BLOCK", str(block))   # read when the handle is created
    n = 256 * len(COUNTS)
    env = mg.VecEnv(mg.CARTPOLE, n, seed=41, env_id_base=1 << 33, auto_reset=True)   # ids above 2^32: both Philox id words
    ref = ora.OracleVec(ora.CARTPOLE, n, seed=41, env_id_base=1 << 33)
    check_step(env, ref, n, 256, COUNTS)


def test_step_kernel_reset_passes_scalar_lanes():
    # n % 4 != 0: the one-env-per-lane kernel (64 envs per wave); the last wave is partial and finishes whole
    n = 64 * len(COUNTS_SCALAR) + 2
    env = mg.VecEnv(mg.CARTPOLE, n, seed=42, auto_reset=True)
    ref = ora.OracleVec(ora.CARTPOLE, n, seed=42)
    check_step(env, ref, n, 64, COUNTS_SCALAR)


@pytest.mark.parametrize("sb,euler", [(False, True), (True, False)])
def test_fused_rollout_reset_passes(sb, euler):
    """K fused steps with auto-reset: bursts of every size at step 0 and again part-way through (truncations timed
    by the step counter), state carried across two rollout calls."""
    n, K = 256 * len(COUNTS), 20
    env = mg.VecEnv(mg.CARTPOLE, n, seed=43, auto_reset=True, sutton_barto_reward=sb, is_euler=euler)
    ref = ora.OracleVec(ora.CARTPOLE, n, seed=43, sutton_barto_reward=sb, is_euler=euler)
    env.reset(), ref.reset()
    rng = np.random.default_rng(12)
    total = 0
    for call in range(2):
        orig = ref.get_state()
        s = orig.copy()
        for w, c in enumerate(COUNTS):
            force(s, rng, w * 256, 256, c)
            # a second burst of another size, 7 + w steps in: envs not forced above whose step counter reaches 500 then
            c2 = COUNTS[(w + 3) % len(COUNTS)]
            sl = slice(w * 256, (w + 1) * 256)
            untouched = np.flatnonzero((s[0, sl].view(np.uint32) == orig[0, sl].view(np.uint32)) & (s[4, sl].view(np.uint32) == orig[4, sl].view(np.uint32)))
            idx = w * 256 + rng.choice(untouched, min(c2, untouched.size), replace=False)
            s[4, idx] = np.full(idx.size, 499 - 7 - w, np.uint32).view(np.float32)
        ref.set_state(s), env.set_state(s)
        a = rng.integers(0, 2, (K, n)).astype(np.uint32)
        obs, rew, done, trunc = env.rollout(a)
        for t in range(K):
            eo, er, ed, et = ref.step(a[t])
            assert np.array_equal(rew[t], er) and np.array_equal(done[t], ed) and np.array_equal(trunc[t], et), f"call {call} step {t}"
            m = ed | et
            if call == 0 and t == 0:   # later calls start from envs that may fall on their own
                assert [int(m[w * 256:(w + 1) * 256].sum()) for w in range(len(COUNTS))] == COUNTS
            total += int(m.sum())
            ref.reset(mask=m)
            assert np.array_equal(obs[t].view(np.uint32), ref.get_state()[:4].view(np.uint32)), f"call {call} step {t}: post-reset obs"
    assert np.array_equal(env.get_state().view(np.uint32), ref.get_state().view(np.uint32))
    assert total > 2 * sum(COUNTS) and env.episode_count() == total
