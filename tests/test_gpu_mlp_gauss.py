"""mgym_rollout_mlp_gauss (include/mgym.h): Gaussian-sampled continuous actions inside the MountainCarContinuous and Pendulum rollout kernels.  The reference
for the actions is the numpy restatement of the documented draw (the fmaf chains of tests/mlp_ref.py for mu, the Box-Muller normal of tests/mlp_gauss_ref.py
for z, a = mu + sigma * z) applied to the observation each env holds before the step; the reference for everything else is a second handle stepped with those
actions.  Whole words, no tolerance.  The distribution is not tested here: it follows from word equality with the specification, whose distribution
tests/test_mlp_gauss_host.py checks."""
import numpy as np
import pytest

import modurl_gym_amd as mg
from families import CLASSIC, FAMILIES, KIND
import mlp_gauss_ref as R
import mlp_ref as M
from mlp_ref import RELU, TANH, packed
from words import bits, same

pytestmark = pytest.mark.gpu

F = np.float32
BOX_FAMILIES = [fam for fam in CLASSIC if FAMILIES[fam].box]
DIMS = {fam: FAMILIES[fam].D for fam in BOX_FAMILIES}
IN_SCALE = {"mountain_car_continuous": (2.0, 40.0), "pendulum": (1.0, 1.0, 0.3)}
ACT_NAME = {RELU: "relu", TANH: "tanh"}
N, K, HALF = 2056, 7, 1028            # 514 lanes: two full blocks of the rollout kernel and a two-lane tail
BASE = (1 << 32) - HALF               # the ids straddle 2^32
POLICY_SEED, CALL, SIGMA = 0xC0FFEE1234, 5, 0.6
ENV_SEED, LIMIT = 11, 3               # resets fall inside the call (steps 2 and 5)


def weights(fam, H, act):
    rng = np.random.default_rng(3000 + 10 * H + act + (100 if fam == "pendulum" else 0))
    return M.normal_weights(rng, DIMS[fam], 1, H, IN_SCALE[fam], b2_scale=0.3)


def make(fam, n=N, base=BASE, limit=LIMIT, auto_reset=True):
    return mg.VecEnv(KIND[fam], n, seed=ENV_SEED, auto_reset=auto_reset, max_episode_steps=limit, env_id_base=base)


@pytest.mark.parametrize("H", [1, 5, 64])
@pytest.mark.parametrize("act", [RELU, TANH], ids=["relu", "tanh"])
@pytest.mark.parametrize("fam", ["mountain_car_continuous", "pendulum"])
def test_rollout_equals_the_restated_draw_and_a_stepping_loop(fam, act, H):
    D, w = DIMS[fam], weights(fam, H, act)
    pol, name = packed(w), ACT_NAME[act]
    env, twin = make(fam), make(fam)
    obs = twin.reset()
    assert same(env.reset(), obs)
    state0 = env.get_state()
    g = np.uint64(BASE) + np.arange(N, dtype=np.uint64)
    acts, gobs, grew, gdone, gtrunc = env.rollout_mlp_gauss(*w, K, SIGMA, POLICY_SEED, CALL, activation=name)
    assert acts.dtype == np.float32 and acts.shape == (K, N)
    moved = 0
    for t in range(K):
        mu = M.scores(pol, D, 1, H, obs, act)[0]                 # the observation held before step t: the handle's, then obs_out[t - 1]
        a = R.gauss_actions(mu, SIGMA, POLICY_SEED, CALL, g, t)
        bad = np.nonzero(bits(acts[t]) != bits(a))[0]
        assert bad.size == 0, f"step {t}: {bad.size} actions differ; env {bad[0]}: device {acts[t][bad[0]]!r}, restatement {a[bad[0]]!r}, mu {mu[bad[0]]!r}"
        moved += int((acts[t] != mu).sum())
        o, r, d, tr = twin.step(acts[t])
        for got, exp, nm in zip((gobs[t], grew[t], gdone[t], gtrunc[t]), (o, r, d, tr), ("obs", "reward", "done", "truncated")):
            assert same(got, exp), f"step {t}: {nm}"
        obs = gobs[t]
    assert moved > K * N * 0.99                             # a draw, not mgym_rollout_mlp
    assert gtrunc[2].all() and gtrunc[5].all() and not gtrunc[0].any()   # the time limit and its fused resets fall inside the call
    state_end = env.get_state()
    assert same(state_end, twin.get_state()) and np.array_equal(env.elapsed_steps(), twin.elapsed_steps())
    assert env.episode_count() == twin.episode_count() >= 2 * N
    twin.close()

    # the same (seed, call) on the same imported state redraws the same actions; call + 1 does not
    env.set_state(state0)
    again = env.rollout_mlp_gauss(*w, K, SIGMA, POLICY_SEED, CALL, activation=name)
    assert all(same(x, y) for x, y in zip(again, (acts, gobs, grew, gdone, gtrunc)))
    env.set_state(state0)
    assert not same(env.rollout_mlp_gauss(*w, K, SIGMA, POLICY_SEED, CALL + 1, activation=name)[0], acts)

    # actions_out = NULL and obs_out = NULL: the other outputs are unchanged
    env.set_state(state0)
    rew, done, trunc = mg.DeviceArray((K, N), np.float32), mg.DeviceArray((K, N), np.uint8), mg.DeviceArray((K, N), np.uint8)
    env.rollout_mlp_gauss_device(pol, H, name, SIGMA, POLICY_SEED, CALL, K, None, None, rew, done, trunc)
    env.sync()
    assert same(rew.numpy(), grew) and same(done.numpy(), gdone) and same(trunc.numpy(), gtrunc)
    assert same(env.get_state(), state_end)

    # sigma = 0 reproduces mgym_rollout_mlp: obs, reward and flag words; the actions as float values (a -0 mu becomes +0)
    env.set_state(state0)
    zero = env.rollout_mlp_gauss(*w, K, 0.0, POLICY_SEED, CALL, activation=name)
    env.set_state(state0)
    plain = env.rollout_mlp(*w, K, activation=name)
    assert np.array_equal(zero[0], plain[0]) and all(same(x, y) for x, y in zip(zero[1:], plain[1:]))
    env.close()

    # two handles of 1028 envs with bases 2^32 - 1028 and 2^32 reproduce the whole population's words
    lo, hi = make(fam, HALF, BASE), make(fam, HALF, 1 << 32)
    lo.reset(); hi.reset()
    lo.set_state(state0[:, :HALF]); hi.set_state(state0[:, HALF:])
    parts = [e.rollout_mlp_gauss(*w, K, SIGMA, POLICY_SEED, CALL, activation=name) for e in (lo, hi)]
    for x, y, z, nm in zip(parts[0], parts[1], (acts, gobs, grew, gdone, gtrunc), ("actions", "obs", "reward", "done", "truncated")):
        assert same(np.concatenate([x, y], axis=-1), z), f"split population: {nm}"
    lo.close(); hi.close()


def test_torch_rollout_mlp_gauss_equals_vecenv():
    torch = pytest.importorskip("torch")
    fam = "pendulum"
    te = mg.TorchVecEnv(KIND[fam], N, seed=31, auto_reset=True, env_id_base=BASE, max_episode_steps=LIMIT)
    ve = mg.VecEnv(KIND[fam], N, seed=31, auto_reset=True, env_id_base=BASE, max_episode_steps=LIMIT)
    te.reset()
    ve.reset()
    w = weights(fam, 5, TANH)
    got = te.rollout_mlp_gauss(*(torch.from_numpy(x) for x in w), K, SIGMA, POLICY_SEED, call=CALL, activation="tanh")
    torch.cuda.synchronize()
    exp = ve.rollout_mlp_gauss(*w, K, SIGMA, POLICY_SEED, CALL, activation="tanh")
    assert got[0].dtype == torch.float32
    for g, e, nm in zip(got, exp, ("actions", "obs", "reward", "done", "truncated")):
        g = g.cpu().numpy()
        g = g.astype(np.uint8) if g.dtype == np.bool_ else g
        assert same(g, e), nm
    ve.close()


def test_bad_arguments_are_reported_before_any_launch():
    L = mg.envs.L

    def bad(env, what, *args):
        with pytest.raises(mg.MgymError) as ei:
            env.rollout_mlp_gauss_device(*args)
        assert ei.value.status == L.ERR_BAD_ARG and str(ei.value).split(": ", 1)[1].startswith("mgym_rollout_mlp_gauss:") and what in str(ei.value), (what, str(ei.value))

    def untouched(env, before):
        env.sync()
        assert same(env.get_state(), before)
        env.close()

    for fam in BOX_FAMILIES:
        pol = packed(weights(fam, 5, RELU))
        env = make(fam, 8, 0)
        env.reset()
        before = env.get_state()
        for sigma in (float("nan"), float("inf"), -float("inf"), -1.0):
            bad(env, "sigma", pol, 5, "relu", sigma, 1, 0, 4)
        bad(env, "hidden", pol, 0, "relu", SIGMA, 1, 0, 4)
        bad(env, "hidden", pol, 65, "relu", SIGMA, 1, 0, 4)
        bad(env, "activation", pol, 5, 2, SIGMA, 1, 0, 4)
        bad(env, "policy", None, 5, "relu", SIGMA, 1, 0, 4)
        bad(env, "K", pol, 5, "relu", SIGMA, 1, 0, -1)
        untouched(env, before)
        for n, base, what in ((2054, 0, "multiple of 4"), (2056, 2, "env_id_base")):
            e = make(fam, n, base)
            e.reset()
            before = e.get_state()
            bad(e, what, pol, 5, "relu", SIGMA, 1, 0, 4)
            untouched(e, before)
    for kind, name in ((mg.CARTPOLE, "CartPole"), (mg.MOUNTAINCAR, "MountainCar"), (mg.LUNARLANDER, "LunarLander")):
        e = mg.VecEnv(kind, 8, seed=ENV_SEED)
        e.reset()
        before = e.get_state()
        D, A = e.mlp_dims()
        bad(e, f"{name} has discrete actions: use mgym_rollout_mlp_sample", np.zeros(5 * (D + 1) + A * 6, F), 5, "relu", SIGMA, 1, 0, 4)
        untouched(e, before)
