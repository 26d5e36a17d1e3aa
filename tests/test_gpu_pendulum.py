"""Pendulum-v1 on the MI355X against the word-exact restatement of include/mgym.h (tests/pendulum_ref.py), bit for bit.  Shapes are the smallest at
which each launch form can go wrong: 2052 = two full 1024-env tiles plus one ragged lane group for the 16-byte kernel (single-pass, and grid-stride
with MGYM_CLASSIC_MAX_BLOCKS = 1), 1027 (no multiple of 4) and 2052 with a reward buffer 4 bytes off for the generic kernel."""
import numpy as np
import pytest

import modurl_gym_amd as mg
import pendulum_ref as R
from device_buffers import CallBuffers
from words import bits, same
from modurl_gym_amd import _lib as L

pytestmark = pytest.mark.gpu

F = np.float32
LIMIT, STEPS = 7, 40
SEED = 0x51A7E5
# form: (n, MGYM_CLASSIC_MAX_BLOCKS, byte offset of the reward buffer, obs_out passed).  The generic kernel runs one env per lane when a buffer is
# misaligned or obs_out cannot be written 16 bytes at a time, and four per lane with a ragged last group when n % 4 != 0 and obs_out is NULL.
FORMS = {"single_pass": (2052, None, 0, True), "grid_stride": (2052, "1", 0, True), "generic_1027": (1027, None, 0, True),
         "generic_offset_reward": (2052, None, 4, True), "generic_ragged_no_obs_out": (1027, None, 0, False)}


def step_actions(n):
    return np.random.default_rng(1000 + n).uniform(-2.5, 2.5, (STEPS, n)).astype(F)


_refs = {}


def reference(n, auto_reset):
    """the reference run every form of a population shares: computed once, never changed"""
    key = (n, auto_reset)
    if key not in _refs:
        ref = R.PendulumRef(n, SEED, 0, 10.0, LIMIT, auto_reset)
        obs0 = ref.reset()
        steps = [ref.step(a) for a in step_actions(n)]
        _refs[key] = dict(obs0=obs0, steps=steps, state=ref.get_state(), elapsed=ref.elapsed.copy(), finished=ref.finished, final_obs=ref.obs())
        for v in (obs0, *[x for s in steps for x in s]):
            v.setflags(write=False)
    return _refs[key]


def test_spec_and_defaults():
    s = mg.get_spec(mg.PENDULUM)
    assert (s.obs_dim, s.n_actions, s.action_is_float, s.state_cols) == (3, 0, 1, 3) and (s.action_low, s.action_high) == (-2.0, 2.0)
    assert list(s.obs_high[:3]) == [1.0, 1.0, 8.0] and list(s.obs_low[:3]) == [-1.0, -1.0, -8.0]
    cfg = L.Config()
    assert L.load().mgym_default_config(mg.PENDULUM, cfg) == L.OK and cfg.gravity == 10.0 and cfg.max_episode_steps == 0
    env = mg.VecEnv(mg.PENDULUM, 8)
    assert env.info()["kind"] == "pendulum"
    assert same(env.observation(), np.array([[1.0] * 8, [0.0] * 8, [0.0] * 8], F))   # as created: th = 0
    env.reset()
    assert same(env.reset_deterministic(), np.array([[1.0] * 8, [0.0] * 8, [0.0] * 8], F)) and not env.elapsed_steps().any()
    single = mg.PendulumV1(seed=3, max_episode_steps=2)
    o = single.reset()
    ref = R.PendulumRef(1, 3, 0, 10.0, 2)
    assert same(o, ref.reset()[:, 0])
    info = single.step(np.float32(1.5))
    eo, er, _, et = ref.step(np.array([1.5], F))
    assert same(info.state, eo[:, 0]) and same(F(info.reward), er[0]) and (info.done, info.truncated) == (False, bool(et[0]))
    assert single.step(2.5).truncated and single.action_space() == ("Box", -2.0, 2.0)


def test_reset_observation_and_sharding():
    n = 2048
    ref = R.PendulumRef(n, SEED)
    exp = ref.reset()
    whole = mg.VecEnv(mg.PENDULUM, n, seed=SEED)
    assert same(whole.reset(), exp) and same(whole.observation(), exp)
    assert np.all(np.abs(exp[2]) <= 1)
    halves = [mg.VecEnv(mg.PENDULUM, n // 2, seed=SEED, env_id_base=b) for b in (0, n // 2)]
    assert same(np.concatenate([h.reset() for h in halves], axis=1), exp)
    # a masked reset draws the next episode of the chosen environments only
    m = (np.arange(n) % 3 == 0).astype(np.uint8)
    assert same(whole.reset(m), ref.reset(m)) and same(whole.get_state(), ref.get_state())


@pytest.mark.parametrize("auto_reset", [True, False])
@pytest.mark.parametrize("form", list(FORMS))
def test_step_forms_equal_the_reference(form, auto_reset, monkeypatch):
    n, max_blocks, offset, with_obs = FORMS[form]
    if max_blocks:
        monkeypatch.setenv("MGYM_CLASSIC_MAX_BLOCKS", max_blocks)   # read when the handle is created
    exp = reference(n, auto_reset)
    env = mg.VecEnv(mg.PENDULUM, n, seed=SEED, auto_reset=auto_reset, max_episode_steps=LIMIT)
    buf = CallBuffers(n, 3, F, 1, offset, with_obs)
    assert same(env.reset(), exp["obs0"])
    for t, a in enumerate(step_actions(n)):
        got = buf.step(env, a)
        for g, e, name in zip(got, exp["steps"][t], ("obs", "reward", "done", "truncated")):
            assert same(g, e), f"{form} step {t}: {name}"
        assert not got[2].any()
    assert same(env.observation(), exp["final_obs"]) and same(env.get_state(), exp["state"]) and np.array_equal(env.elapsed_steps(), exp["elapsed"])
    assert env.episode_count() == exp["finished"] == (5 * n if auto_reset else (STEPS - LIMIT + 1) * n)
    if not auto_reset:   # truncated stays up and the count goes on (it saturates at 65535)
        assert np.all(exp["steps"][-1][3] == 1) and np.all(exp["elapsed"] == STEPS)
        env.set_elapsed_steps(np.full(n, 65534, np.uint32))
        buf.step(env, np.zeros(n, F)); buf.step(env, np.zeros(n, F))
        assert np.all(env.elapsed_steps() == 65535)


@pytest.mark.parametrize("n", [2052, 1027])
def test_rollout_equals_steps(n):
    K = 33
    acts = step_actions(n)[:K]
    exp = reference(n, True)
    fused = mg.VecEnv(mg.PENDULUM, n, seed=SEED, auto_reset=True, max_episode_steps=LIMIT)
    loop = mg.VecEnv(mg.PENDULUM, n, seed=SEED, auto_reset=True, max_episode_steps=LIMIT)
    fused.reset(); loop.reset()
    gobs, grew, gdone, gtrunc = fused.rollout(acts)   # n = 1027: the fallback to K steps
    for t in range(K):
        step = loop.step(acts[t])
        for g, s, e in zip((gobs[t], grew[t], gdone[t], gtrunc[t]), step, exp["steps"][t]):
            assert same(g, s) and same(g, e), f"n = {n} step {t}"
    assert same(fused.get_state(), loop.get_state()) and np.array_equal(fused.elapsed_steps(), loop.elapsed_steps())
    assert fused.episode_count() == loop.episode_count() == (K // LIMIT) * n


def mlp_weights(H):
    rng = np.random.default_rng(40 + H)
    return rng.normal(0, 1.5, (H, 3)).astype(F), rng.normal(0, 0.5, H).astype(F), rng.normal(0, 2.0 / np.sqrt(H), (1, H)).astype(F), rng.normal(0, 0.3, 1).astype(F)


POLICIES = ["uniform", "linear"] + [f"mlp-{H}-{act}" for H in (1, 33, 64) for act in ("relu", "tanh")]


@pytest.mark.parametrize("policy", POLICIES)
def test_policy_rollouts(policy):
    n, K, base = 2052, 16, 4096
    kw = dict(seed=SEED, env_id_base=base, auto_reset=True, max_episode_steps=LIMIT)
    env, table = mg.VecEnv(mg.PENDULUM, n, **kw), mg.VecEnv(mg.PENDULUM, n, **kw)
    ref = R.PendulumRef(n, SEED, base, 10.0, LIMIT, True)
    assert same(env.reset(), ref.reset())
    table.reset()
    rounds = 2 if policy == "uniform" else 1   # a second uniform call draws with the next call word
    for rnd in range(rounds):
        if policy == "uniform":
            got, exp = env.rollout_uniform(0xABCDEF12345, K), ref.rollout_uniform(0xABCDEF12345, K)
        elif policy == "linear":
            pol = np.array([-2.0, 3.0, -1.0, 0.25], F)
            got, exp = env.rollout_linear(pol, K), ref.rollout_linear(pol, K)
        else:
            H, act = int(policy.split("-")[1]), policy.split("-")[2]
            w = mlp_weights(H)
            got = env.rollout_mlp(*w, K, activation=act)
            exp = ref.rollout_mlp(np.concatenate([x.ravel() for x in w]), H, R.TANH if act == "tanh" else R.RELU, K)
        for g, e, name in zip(got, exp, ("actions", "obs", "reward", "done", "truncated")):
            assert same(g, e), f"{policy} call {rnd}: {name}"
        acts = bits(got[0]).view(F)
        assert len(np.unique(acts)) > n // 4 and (policy != "uniform" or (acts.min() >= -2 and acts.max() < 2))
        fed = table.rollout(acts)   # the same K steps from an action table
        assert all(same(g, f) for g, f in zip(got[1:], fed)), f"{policy}: differs from mgym_rollout fed its actions"
        if rnd:
            assert not same(got[0], first)
        first = got[0]
    assert same(env.get_state(), ref.get_state()) and np.array_equal(env.elapsed_steps(), ref.elapsed)
    assert env.episode_count() == ref.finished == rounds * (K // LIMIT) * n


def test_set_state_recomputes_cos_and_sin():
    n = 1027
    th = np.array([R.BIG_TH[i % len(R.BIG_TH)] for i in range(n)], F)
    thdot = ((np.arange(n) % 17) - 8).astype(F)
    blob = np.stack([bits(th), bits(thdot), np.arange(n, dtype=np.uint32)])
    env = mg.VecEnv(mg.PENDULUM, n, seed=1, max_episode_steps=LIMIT)
    env.reset()
    env.step(np.zeros(n, F))
    env.set_state(blob.view(F))
    assert same(env.get_state(), blob) and not env.elapsed_steps().any()
    assert same(env.observation(), np.stack([R.cosf(th), R.sinf(th), thdot]))
    ref = R.PendulumRef(n, 1, 0, 10.0, LIMIT)
    ref.set_state(blob)
    a = np.random.default_rng(2).uniform(-2.5, 2.5, n).astype(F)
    for _ in range(3):
        assert all(same(g, e) for g, e in zip(env.step(a), ref.step(a)))
    assert same(env.get_state(), ref.get_state())


def test_errors():
    n = 2052
    env = mg.VecEnv(mg.PENDULUM, n, seed=5, max_episode_steps=LIMIT)
    w1, b1, w2, b2 = mlp_weights(4)
    with pytest.raises(mg.MgymError) as ei:
        env.rollout_mlp_sample(w1, b1, w2, b2, 4, seed=1)
    assert ei.value.status == L.ERR_BAD_ARG and "Pendulum" in str(ei.value)
    env.reset()
    before, obs = env.get_state().copy(), env.observation()
    a = np.zeros(n, F)
    a[[0, 1029, 2051]] = np.nan
    buf = CallBuffers(n, 3, F)
    buf.put_actions(a)
    env.step_device(*buf.pointers())
    with pytest.raises(mg.InvalidActionError):
        env.sync()
    after = env.get_state()
    bad = np.isnan(a)
    assert same(after[:, bad], before[:, bad]) and same(env.observation()[:, bad], obs[:, bad]) and not same(after[:, ~bad], before[:, ~bad])
    o, r, d, t = (x[0] for x in buf.read())
    assert same(o[:, bad], obs[:, bad]) and not r[bad].any() and not d.any() and not t.any()
    env.sync()   # the status was cleared
    # +-inf is inside the Box once clamped: the words of +-2
    twin = mg.VecEnv(mg.PENDULUM, n, seed=5, max_episode_steps=LIMIT)
    twin.set_state(env.get_state())
    inf = np.where(np.arange(n) % 2 == 0, np.inf, -np.inf).astype(F)
    assert all(same(g, e) for g, e in zip(env.step(inf), twin.step(np.clip(inf, -2, 2))))
    with pytest.raises(mg.BadConfigError):
        mg.VecEnv(mg.PENDULUM, 4, gravity=float("inf"))
    with pytest.raises(mg.BadConfigError):
        mg.VecEnv(mg.PENDULUM, 4, gravity=float("nan"))
    with pytest.raises(mg.BadConfigError):
        mg.VecEnv(mg.PENDULUM, 4, max_episode_steps=70000)
    with pytest.raises(mg.MgymError):
        mg.VecEnv(mg.PENDULUM, 6).rollout_uniform(1, 4)   # the fused forms need n_envs % 4 == 0
    with pytest.raises(mg.PolicyShapeError):
        mg.VecEnv(mg.PENDULUM, 8).rollout_linear(np.zeros(3, F), 4)


def test_captured_step_replays_like_eager_steps():
    n = 2052
    kw = dict(seed=9, auto_reset=True, max_episode_steps=2)
    env, eager = mg.VecEnv(mg.PENDULUM, n, **kw), mg.VecEnv(mg.PENDULUM, n, **kw)
    env.reset(); eager.reset()
    a = np.random.default_rng(3).uniform(-2.5, 2.5, n).astype(F)
    buf = CallBuffers(n, 3, F)
    buf.put_actions(a)
    graph = env.graph_capture(lambda: env.step_device(*buf.pointers()))   # one stream, one kernel node
    for t in range(3):
        env.graph_launch(graph)
        env.sync()
        assert all(same(g, e) for g, e in zip((x[0] for x in buf.read()), eager.step(a))), f"replay {t}"
    env.graph_destroy(graph)
    assert same(env.get_state(), eager.get_state()) and env.episode_count() == eager.episode_count() == n


def test_torch_vec_env_equals_the_ctypes_path():
    torch = pytest.importorskip("torch")
    n, K = 2052, 9
    kw = dict(seed=11, auto_reset=True, max_episode_steps=LIMIT)
    tenv, env = mg.TorchVecEnv(mg.PENDULUM, n, **kw), mg.VecEnv(mg.PENDULUM, n, **kw)
    assert tenv.action_is_float and same(tenv.reset().cpu().numpy(), env.reset())
    acts = np.random.default_rng(4).uniform(-2.5, 2.5, (K + 1, n)).astype(F)
    got = tenv.step(torch.from_numpy(acts[0]).cuda(), check=True)
    assert all(same(g.cpu().numpy().view(np.uint8) if g.dtype == torch.bool else g.cpu().numpy(), e) for g, e in zip(got, env.step(acts[0])))
    got = tenv.rollout(torch.from_numpy(acts[1:]).cuda())
    tenv.check()
    assert all(same(g.cpu().numpy().view(np.uint8) if g.dtype == torch.bool else g.cpu().numpy(), e) for g, e in zip(got, env.rollout(acts[1:])))
    w = mlp_weights(33)
    got = tenv.rollout_mlp(*(torch.from_numpy(x) for x in w), K, activation="tanh")
    tenv.check()
    assert got[0].dtype == torch.float32
    assert all(same(g.cpu().numpy().view(np.uint8) if g.dtype == torch.bool else g.cpu().numpy(), e) for g, e in zip(got, env.rollout_mlp(*w, K, activation="tanh")))
