"""The two launch forms of the classic step kernels (CartPole, MountainCar, MountainCarContinuous): the single-pass form (one block per tile,
no loop) that every population up to the block cap takes, and the grid-stride form beyond it, which MGYM_CLASSIC_MAX_BLOCKS brings within reach of
a few thousand environments.  Sizes are the smallest at which a tile, tail or pass boundary exists: one lane, a tile less one lane, a whole tile
(1024 envs), a tile and one lane, three tiles and one lane.  Everything is compared word for word: with the CPU oracle (reward, done, truncated,
obs_out, engine observation, state blob, episode_count), and the grid-stride form with the single-pass form on the same seed and actions."""
import numpy as np
import pytest

import modurl_gym_amd as mg
from oracle import oracle as ora
from families import BY_KIND
from time_limit_ref import TimeLimitRef
from words import same

pytestmark = pytest.mark.gpu

STEPS = 64
NAMES = ("obs_out", "reward", "done", "truncated")


def actions(kind, rng, n):
    if kind == mg.MOUNTAINCAR_CONT:
        return rng.uniform(-1.5, 1.5, n).astype(np.float32)   # beyond [-1, 1]: the step clamps
    return rng.integers(0, 2 if kind == mg.CARTPOLE else 3, n).astype(np.uint32)


# ---- CartPole against the oracle ----------------------------------------------------------------------------------------------------
def cartpole_vs_oracle(n, seed):
    env = mg.VecEnv(mg.CARTPOLE, n, seed=seed, auto_reset=True)
    ref = ora.OracleVec(ora.CARTPOLE, n, seed=seed)
    rng = np.random.default_rng(seed)
    assert same(env.reset(), ref.reset())
    total = 0
    for t in range(STEPS):
        a = actions(mg.CARTPOLE, rng, n)
        got, exp = env.step(a), ref.step(a)
        for g, e, nm in zip(got[1:], exp[1:], NAMES[1:]):
            assert same(g, e), f"n={n} step {t}: {nm}"
        m = exp[2] | exp[3]
        total += int(m.sum())
        if m.any():
            ref.reset(mask=m)
        post = ref.get_state()[:4]
        assert same(got[0], post), f"n={n} step {t}: obs_out"
        assert same(env.observation(), post), f"n={n} step {t}: engine observation"
    assert same(env.get_state(), ref.get_state()), f"n={n}: state blob"
    assert total > 0 and env.episode_count() == total
    env.close()


@pytest.mark.parametrize("n", [4, 1020, 1024, 1028, 3076])
def test_cartpole_four_envs_per_lane(n):
    cartpole_vs_oracle(n, 100 + n)


@pytest.mark.parametrize("block", [64, 128, 256])
def test_cartpole_block_sizes(block, monkeypatch):
    monkeypatch.setenv("MGYM_CARTPOLE_BLOCK", str(block))   # read when the handle is created
    cartpole_vs_oracle(3076, 7 + block)


@pytest.mark.parametrize("n", [1, 1023, 1027])
def test_cartpole_one_env_per_lane(n):
    cartpole_vs_oracle(n, 200 + n)   # n % 4 != 0: the one-env-per-lane kernel (tiles of 256)


# ---- grid-stride form against single-pass form --------------------------------------------------------------------------------------
def run_handle(kind, n, seed, limit):
    env = mg.VecEnv(kind, n, seed=seed, auto_reset=True, max_episode_steps=limit)
    rng = np.random.default_rng(seed)
    out = [env.reset().copy()]
    for _ in range(STEPS):
        out += [x.copy() for x in env.step(actions(kind, rng, n))]
        out.append(env.observation())
    out.append(env.get_state().copy())
    count = env.episode_count()
    env.close()
    return out, count


@pytest.mark.parametrize("kind,limit", [(mg.CARTPOLE, 0), (mg.MOUNTAINCAR, 5), (mg.MOUNTAINCAR_CONT, 5)])
@pytest.mark.parametrize("cap", [2, 3])
def test_grid_stride_equals_single_pass(kind, limit, cap, monkeypatch):
    """n = 3076 is four tiles: a cap of 2 blocks gives every block two passes, a cap of 3 gives block 0 two passes and the others one."""
    n, seed = 3076, 31
    monkeypatch.delenv("MGYM_CLASSIC_MAX_BLOCKS", raising=False)
    one, count_one = run_handle(kind, n, seed, limit)
    monkeypatch.setenv("MGYM_CLASSIC_MAX_BLOCKS", str(cap))   # read when the handle is created
    strided, count_strided = run_handle(kind, n, seed, limit)
    assert len(one) == len(strided)
    for i, (a, b) in enumerate(zip(one, strided)):
        assert same(a, b), f"output {i} differs between the forms"
    assert count_one == count_strided and count_one > 0


# ---- MountainCar / MountainCarContinuous against the oracle -------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [mg.MOUNTAINCAR, mg.MOUNTAINCAR_CONT])
@pytest.mark.parametrize("limit", [0, 5])
@pytest.mark.parametrize("n", [4, 1028, 3076])
def test_mountaincar_vs_oracle(kind, limit, n):
    """limit = 5 forces truncations and resets every few steps and takes the instantiation that reads the elapsed column."""
    seed = 300 + n + limit
    env = mg.VecEnv(kind, n, seed=seed, auto_reset=True, max_episode_steps=limit)
    ref = TimeLimitRef(ora.OracleVec(BY_KIND[kind].okind, n, seed=seed), limit, True)
    rng = np.random.default_rng(seed)
    assert same(env.reset(), ref.reset())
    for t in range(STEPS):
        a = actions(kind, rng, n)
        got, exp = env.step(a), ref.step(a)
        for g, e, nm in zip(got, exp, NAMES):
            assert same(g, e), f"n={n} step {t}: {nm}"
        assert same(env.observation(), exp[0]), f"n={n} step {t}: engine observation"
    assert same(env.get_state(), ref.ref.get_state()), f"n={n}: state blob"
    assert env.episode_count() == ref.finished
    if limit:
        assert ref.finished >= n * (STEPS // limit) and np.array_equal(env.elapsed_steps(), ref.elapsed)
    env.close()


# ---- graph replay of the single-pass form -------------------------------------------------------------------------------------------
def test_graph_replay_single_pass():
    """3 captured steps over 3 action columns, replayed twice = 6 eager steps on a second handle."""
    n, seed = 1028, 77
    rng = np.random.default_rng(seed)
    cols = rng.integers(0, 2, (3, n)).astype(np.uint32)
    genv = mg.VecEnv(mg.CARTPOLE, n, seed=seed, auto_reset=True)
    eenv = mg.VecEnv(mg.CARTPOLE, n, seed=seed, auto_reset=True)
    assert same(genv.reset(), eenv.reset())
    dact = [mg.DeviceArray.from_numpy(c) for c in cols]
    obs = [mg.DeviceArray((4, n), np.float32) for _ in cols]
    rew = [mg.DeviceArray(n, np.float32) for _ in cols]
    done = [mg.DeviceArray(n, np.uint8) for _ in cols]
    trunc = [mg.DeviceArray(n, np.uint8) for _ in cols]

    def three_steps():
        for k in range(3):
            genv.step_device(dact[k], obs[k], rew[k], done[k], trunc[k])

    g = genv.graph_capture(three_steps)
    try:
        for rep in range(2):
            genv.graph_launch(g)
            genv.sync()
            for k in range(3):
                exp = eenv.step(cols[k])
                for got, e, nm in zip((obs[k], rew[k], done[k], trunc[k]), exp, NAMES):
                    assert same(got.numpy().reshape(e.shape), e), f"replay {rep} step {k}: {nm}"
    finally:
        genv.graph_destroy(g)
    assert same(genv.get_state(), eenv.get_state())
    assert genv.episode_count() == eenv.episode_count()
    genv.close(), eenv.close()
