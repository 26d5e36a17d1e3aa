"""Acrobot-v1 on the MI355X against the word-exact restatement of include/mgym.h (tests/acrobot_ref.py), bit for bit.  Shapes are the smallest at which
each launch form can go wrong: n = 1 and 1027 with an obs buffer (the generic kernel, one environment per lane; K plain steps for a rollout), 1024 (one
full tile of the 16-byte kernel, single-pass), 1024 with the caller's reward buffer 4 bytes off its alignment (one per lane again, and the rollout's
fallback), 2052 = two tiles and one lane group with MGYM_CLASSIC_MAX_BLOCKS = 1 (the 16-byte kernel's grid-stride form: one block, three passes) and
1027 with obs_out NULL (the generic kernel with four environments per lane and a ragged last group).
Every run starts from imported states just short of the swing-up height, so that `done` endings occur within a few steps beside the time limit's."""
import numpy as np
import pytest

import acrobot_ref as R
from device_buffers import CallBuffers, FinalBuf, twin_steps
from glibc_f32 import glibc_has_fdlibm_expm1f
from words import bits, same
import modurl_gym_amd as mg
from modurl_gym_amd import _lib as L

pytestmark = pytest.mark.gpu

F = np.float32
LIMIT, STEPS = 7, 33
SEED = 0xAC20B07
PSEED = 0xABCDEF12345
# form: (n, byte offset of the reward buffer, obs_out passed, MGYM_CLASSIC_MAX_BLOCKS)
FORMS = {"n1": (1, 0, True, None), "generic_1027": (1027, 0, True, None), "tile_1024": (1024, 0, True, None), "offset_1024": (1024, 4, True, None),
         "grid_stride_2052": (2052, 0, True, "1"), "ragged_1027_no_obs_out": (1027, 0, False, None)}


def form_env(form, limit, auto, monkeypatch):
    """-> (a handle of the form's population, its Buffers factory arguments)"""
    n, offset, with_obs, max_blocks = FORMS[form]
    if max_blocks:
        monkeypatch.setenv("MGYM_CLASSIC_MAX_BLOCKS", max_blocks)   # read when the handle is created
    return make(n, limit, auto), n, offset, with_obs
MODES = [(LIMIT, True), (0, False), (LIMIT, False), (0, True)]   # (max_episode_steps, auto_reset)
needs_fdlibm = pytest.mark.skipif(not glibc_has_fdlibm_expm1f(), reason="this glibc's expm1f is not the fdlibm one that mg_expm1f restates")


def table_actions(n, steps=STEPS):
    return np.random.default_rng(1000 + n).integers(0, 3, (steps, n)).astype(np.uint32)


def near_swing_up(n):
    """a state blob whose arms are a few steps below the bar and moving up: th1 in +-(1.7, 2.09), th2 small, w1 towards the top; a few of the first
    environments a step or two from reset-like rest, so that lanes with one, several and no finished environment all occur"""
    rng = np.random.default_rng(77 + n)
    sign = np.where(rng.integers(0, 2, n) == 0, -1.0, 1.0)
    th1, th2 = sign * rng.uniform(1.7, 2.09, n), rng.uniform(-0.3, 0.3, n)
    w1, w2 = sign * rng.uniform(0.3, 2.5, n), rng.uniform(-1.0, 1.0, n)
    rest = np.arange(n) % 5 == 0
    th1[rest], w1[rest] = 0.05, 0.0
    return np.stack([bits(v.astype(F)) for v in (th1, th2, w1, w2)] + [np.arange(n, dtype=np.uint32) * 3])


def make(n, limit, auto, **kw):
    return mg.VecEnv(mg.ACROBOT, n, seed=SEED, auto_reset=auto, max_episode_steps=limit, **kw)


_refs = {}


def reference(n, limit, auto):
    """the table-action run every form of a population shares: reset, 2 steps, then the imported states and STEPS steps.  Computed once, never changed"""
    key = (n, limit, auto)
    if key not in _refs:
        ref = R.AcrobotRef(n, SEED, 0, limit, auto)
        acts = table_actions(n, STEPS + 2)
        obs0 = ref.reset()
        head = [ref.step(a) for a in acts[:2]]
        ref.set_state(near_swing_up(n))
        steps = [ref.step(a) for a in acts[2:]]
        _refs[key] = dict(obs0=obs0, head=head, steps=steps, state=ref.get_state(), elapsed=ref.elapsed.copy(), finished=ref.finished, final_obs=ref.obs())
        for v in (obs0, *[x for s in head + steps for x in s]):
            v.setflags(write=False)
    return _refs[key]


def test_spec_created_state_and_single_env():
    s = mg.get_spec(mg.ACROBOT)
    assert (s.obs_dim, s.n_actions, s.action_is_float, s.state_cols) == (6, 3, 0, 5)
    assert list(s.obs_high[:6]) == [1.0, 1.0, 1.0, 1.0, float(R.V1), float(R.V2)] and list(s.obs_low[:6]) == [-1.0, -1.0, -1.0, -1.0, -float(R.V1), -float(R.V2)]
    rest = np.array([[1.0] * 8, [0.0] * 8, [1.0] * 8, [0.0] * 8, [0.0] * 8, [0.0] * 8], F)
    env = mg.VecEnv(mg.ACROBOT, 8)
    assert env.info()["kind"] == "acrobot" and same(env.observation(), rest)   # as created: every state word 0
    env.reset()
    assert same(env.reset_deterministic(), rest) and not env.elapsed_steps().any() and not env.get_state()[:4].any()
    single = mg.AcrobotV1(seed=3, max_episode_steps=2)
    ref = R.AcrobotRef(1, 3, 0, 2)
    assert same(single.reset(), ref.reset()[:, 0])
    info = single.step(np.uint32(2))
    eo, er, ed, et = ref.step(np.array([2], np.uint32))
    assert same(info.state, eo[:, 0]) and same(F(info.reward), er[0]) and (info.done, info.truncated) == (False, False)
    assert single.step(0).truncated and single.action_space() == ("Discrete", 3)


def test_reset_observation_masked_reset_and_sharding():
    n = 1024
    ref = R.AcrobotRef(n, SEED)
    exp = ref.reset()
    whole = make(n, 0, False)
    assert same(whole.reset(), exp) and same(whole.observation(), exp) and np.all(np.abs(exp[4:]) < 0.1)
    halves = [make(n // 2, 0, False, env_id_base=b) for b in (0, n // 2)]
    assert same(np.concatenate([h.reset() for h in halves], axis=1), exp)
    m = (np.arange(n) % 3 == 0).astype(np.uint8)   # a masked reset draws the next episode of the chosen environments only
    assert same(whole.reset(m), ref.reset(m)) and same(whole.get_state(), ref.get_state())


@pytest.mark.parametrize("limit,auto", MODES)
@pytest.mark.parametrize("form", list(FORMS))
def test_step_forms_equal_the_reference(form, limit, auto, monkeypatch):
    env, n, offset, with_obs = form_env(form, limit, auto, monkeypatch)
    exp = reference(n, limit, auto)
    buf = CallBuffers(n, 6, np.uint32, 1, offset, with_obs)
    acts = table_actions(n, STEPS + 2)
    assert same(env.reset(), exp["obs0"])
    for t in range(2):
        assert all(same(g, e) for g, e in zip(buf.step(env, acts[t]), exp["head"][t])), f"{form}: step {t} after the reset"
    env.set_state(near_swing_up(n).view(F))
    assert not env.elapsed_steps().any()
    for t in range(STEPS):
        got = buf.step(env, acts[2 + t])
        for g, e, name in zip(got, exp["steps"][t], ("obs", "reward", "done", "truncated")):
            assert same(g, e), f"{form} limit {limit} auto {auto} step {t}: {name}"
        assert same(env.observation(), got[0])   # the zero-copy view is the observation just returned
    assert same(env.get_state(), exp["state"]) and np.array_equal(env.elapsed_steps(), exp["elapsed"]) and env.episode_count() == exp["finished"]
    done = np.array([s[2] for s in exp["steps"]])
    if n > 1:
        assert done.any() and not done.all() and (limit == 0 or np.array([s[3] for s in exp["steps"]]).any())   # both kinds of ending were checked


@pytest.mark.parametrize("K", [1, 5, 33])
@pytest.mark.parametrize("limit,auto", MODES)
@pytest.mark.parametrize("form", list(FORMS))
def test_table_rollout_equals_the_reference(form, limit, auto, K, monkeypatch):
    """mgym_rollout: the fused kernel at 1024 and 2052, K plain steps at n = 1, 1027 (with and without obs_out) and with the misaligned buffer — the same words"""
    env, n, offset, with_obs = form_env(form, limit, auto, monkeypatch)
    exp = reference(n, limit, auto)
    env.set_state(near_swing_up(n).view(F))
    buf = CallBuffers(n, 6, np.uint32, K, offset, with_obs)
    buf.put_actions(table_actions(n, STEPS + 2)[2:2 + K])
    act, *outs = buf.pointers()
    env.rollout_device(act, K, *outs)
    env.sync()
    got = buf.read()
    for t in range(K):
        for g, e, name in zip(got, exp["steps"][t], ("obs", "reward", "done", "truncated")):
            assert g is None or same(g[t], e), f"{form} limit {limit} auto {auto} K {K} step {t}: {name}"
    assert same(env.observation(), exp["steps"][K - 1][0])   # the engine's columns after the call: what obs_out NULL leaves the caller to read
    if K == STEPS:
        assert same(env.get_state(), exp["state"]) and np.array_equal(env.elapsed_steps(), exp["elapsed"]) and env.episode_count() == exp["finished"]


def mlp_weights(H, seed=0):
    """weights that see the sines and velocities: those inputs scaled up, the two cosines taken out of the hidden bias"""
    rng = np.random.default_rng(40 + H + seed)
    w1 = rng.normal(0, 1.0, (H, 6)) * np.array([1.0, 3.0, 1.0, 3.0, 1.0, 1.0])
    return w1.astype(F), rng.normal(0, 0.3, H).astype(F), rng.normal(0, 2.0 / np.sqrt(H), (3, H)).astype(F), np.zeros(3, F)


SWING = np.zeros(21, F)   # push with the first link's velocity once it is fast enough, else no torque
SWING[[4, 13, 18]] = -10.0, 0.3, 10.0
POLICIES = ["uniform", "linear", "mlp-relu", "mlp-tanh", pytest.param("sample-relu", marks=needs_fdlibm), pytest.param("sample-tanh", marks=needs_fdlibm)]


def policy_call(env, ref, policy, K, call=3):
    H = 33
    w = mlp_weights(H)
    flat = np.concatenate([x.ravel() for x in w])
    if policy == "uniform":
        return env.rollout_uniform(PSEED, K), ref.rollout_uniform(PSEED, K)
    if policy == "linear":
        return env.rollout_linear(SWING, K), ref.rollout_linear(SWING, K)
    form, act = policy.split("-")
    if form == "mlp":
        return env.rollout_mlp(*w, K, activation=act), ref.rollout_mlp(flat, H, R.TANH if act == "tanh" else R.RELU, K)
    return env.rollout_mlp_sample(*w, K, seed=PSEED, call=call, activation=act), ref.rollout_mlp_sample(flat, H, R.TANH if act == "tanh" else R.RELU, PSEED, call, K)


@pytest.mark.parametrize("K", [1, 5, 33])
@pytest.mark.parametrize("limit,auto", MODES[:2])
@pytest.mark.parametrize("policy", POLICIES)
def test_policy_rollouts(policy, limit, auto, K):
    n, base = 1024, 4096
    env, table = make(n, limit, auto, env_id_base=base), make(n, limit, auto, env_id_base=base)
    ref = R.AcrobotRef(n, SEED, base, limit, auto)
    for e in (env, table):
        e.set_state(near_swing_up(n).view(F))
    ref.set_state(near_swing_up(n))
    rounds = 2 if policy == "uniform" else 1   # a second uniform call draws with the next call word
    for rnd in range(rounds):
        got, exp = policy_call(env, ref, policy, K)
        for g, e, name in zip(got, exp, ("actions", "obs", "reward", "done", "truncated")):
            assert same(g, e), f"{policy} limit {limit} K {K} call {rnd}: {name}"
        assert K < 5 or len(np.unique(got[0])) >= 2   # the policy really chooses
        fed = table.rollout(got[0])   # the same K steps from an action table
        assert all(same(g, f) for g, f in zip(got[1:], fed)), f"{policy}: differs from mgym_rollout fed its actions"
    assert same(env.get_state(), ref.get_state()) and np.array_equal(env.elapsed_steps(), ref.elapsed) and env.episode_count() == ref.finished
    assert K < 5 or ref.finished > 0


def test_results_do_not_depend_on_sharding():
    n, K = 1024, 5
    whole = make(n, LIMIT, True)
    halves = [make(n // 2, LIMIT, True, env_id_base=b) for b in (0, n // 2)]
    st = near_swing_up(n)
    whole.set_state(st.view(F))
    for h, sl in zip(halves, (slice(0, n // 2), slice(n // 2, n))):
        h.set_state(np.ascontiguousarray(st[:, sl]).view(F))
    w = mlp_weights(8)
    for call in (lambda e: e.rollout_uniform(PSEED, K), lambda e: e.rollout_mlp(*w, K), lambda e: e.rollout(table_actions(e.n, K) * 0 + 2)):
        got, parts = call(whole), [call(h) for h in halves]
        assert all(same(g, np.concatenate([p[k] for p in parts], axis=-1)) for k, g in enumerate(got))
    assert same(whole.get_state(), np.concatenate([h.get_state() for h in halves], axis=1))


def test_state_and_elapsed_round_trip():
    n = 1027
    env = make(n, LIMIT, False)
    env.reset()
    env.step(np.ones(n, np.uint32))
    big = np.array([1e6, -12345.678, 3.1415927, -3.1415927, -0.0, 119.9, 125.0], F)
    blob = np.stack([bits(np.resize(big, n)), bits(np.resize(big[::-1], n)), bits(((np.arange(n) % 17) - 8).astype(F)), bits(((np.arange(n) % 41) - 20).astype(F)),
                     np.arange(n, dtype=np.uint32)])
    env.set_state(blob.view(F))
    th1, th2 = blob[0].view(F), blob[1].view(F)
    assert same(env.get_state(), blob) and not env.elapsed_steps().any()   # taken as they are: no wrap, no clamp; the count starts at 0
    assert same(env.observation(), np.stack([R.cosf(th1), R.sinf(th1), R.cosf(th2), R.sinf(th2), blob[2].view(F), blob[3].view(F)]))
    el = (np.arange(n) * 97 % 70000).astype(np.uint32)
    env.set_elapsed_steps(el)
    assert np.array_equal(env.elapsed_steps(), np.minimum(el, 65535))
    ref = R.AcrobotRef(n, SEED, 0, LIMIT)
    ref.set_state(blob)
    ref.elapsed = np.minimum(el, 65535).astype(np.uint32)
    a = table_actions(n, 3)
    for t in range(3):
        assert all(same(g, e) for g, e in zip(env.step(a[t]), ref.step(a[t])))
    assert same(env.get_state(), ref.get_state()) and np.array_equal(env.elapsed_steps(), ref.elapsed)


def test_refusals_leave_the_state_untouched():
    n = 1024
    env = make(n, LIMIT, True)
    env.set_state(near_swing_up(n).view(F))
    before, view = env.get_state().copy(), env.observation().copy()
    w = mlp_weights(4)
    with pytest.raises(mg.MgymError) as ei:
        env.rollout_mlp_gauss(*w, 4, sigma=0.5, seed=1)
    assert ei.value.status == L.ERR_BAD_ARG and "Acrobot has discrete actions" in str(ei.value)
    fin = mg.DeviceArray((2, 6, n), F)
    env.set_final_obs_out_device(fin, 2)
    for call in (lambda: env.rollout_uniform(1, 3), lambda: env.rollout(table_actions(n, 3)), lambda: env.rollout_mlp(*w, 3), lambda: env.rollout_linear(SWING, 3),
                 lambda: env.rollout_mlp_sample(*w, 3, seed=1)):
        with pytest.raises(mg.MgymError) as ei:
            call()
        assert ei.value.status == L.ERR_BAD_ARG and "steps_cap" in str(ei.value)
    env.set_final_obs_out_device(None)
    for bad in (lambda: make(6, 0, False).rollout_uniform(1, 4), lambda: make(1027, 0, False).rollout_mlp(*w, 4), lambda: make(8, 0, False, env_id_base=2).rollout_uniform(1, 4)):
        with pytest.raises(mg.MgymError):
            bad()   # the fused policy forms need n_envs % 4 == 0 and, where they draw, env_id_base % 4 == 0
    with pytest.raises(mg.PolicyShapeError):
        env.rollout_linear(np.zeros(9, F), 4)
    assert same(env.get_state(), before) and same(env.observation(), view) and env.episode_count() == 0 and not env.elapsed_steps().any()


@pytest.mark.parametrize("form", ["tile_1024", "generic_1027", "grid_stride_2052", "ragged_1027_no_obs_out"])
def test_action_3_is_a_sticky_error_and_leaves_the_environment(form, monkeypatch):
    env, n, _, with_obs = form_env(form, LIMIT, False, monkeypatch)
    env.set_state(near_swing_up(n).view(F))
    before, obs = env.get_state().copy(), env.observation().copy()
    a = np.ones(n, np.uint32)
    bad = np.zeros(n, bool)
    bad[[0, 513, n - 1]] = True
    a[bad] = (3, 0xFFFFFFFF, 1 << 31)
    buf = CallBuffers(n, 6, np.uint32, with_obs=with_obs)
    buf.put_actions(a)
    env.step_device(*buf.pointers())
    with pytest.raises(mg.InvalidActionError):
        env.sync()
    after = env.get_state()
    assert same(after[:, bad], before[:, bad]) and same(env.observation()[:, bad], obs[:, bad]) and not same(after[:, ~bad], before[:, ~bad])
    o, r, d, t = buf.read()
    o, r, d, t = (o[0] if with_obs else env.observation()), r[0], d[0], t[0]
    assert same(o[:, bad], obs[:, bad]) and not r[bad].any() and not d[bad].any() and not t[bad].any() and np.all(env.elapsed_steps() == 1)
    env.sync()   # the status was cleared


def twin_finals(n, limit, actions):
    """device_buffers.twin_steps from the seeded states: -> (the twin's obs [K, 6, n] — what each step produced before any reset — and its
    done | truncated [K, n])"""
    stepper, twin = make(n, limit, True), make(n, limit, False)
    stepper.set_state(near_swing_up(n).view(F))
    _, tobs, tdone, ttrunc = twin_steps(stepper, twin, actions)
    return tobs, tdone | ttrunc


@pytest.mark.parametrize("limit", [LIMIT, 0])
@pytest.mark.parametrize("src", ["step", "step_generic", "step_grid_stride", "step_ragged_no_obs_out", "table", "table_steps", "uniform", "linear", "mlp",
                                 pytest.param("sample", marks=needs_fdlibm)])
def test_final_observations_equal_a_twin_without_auto_reset(src, limit, monkeypatch):
    """the seeded states end by `done` at steps 0 and 1 and, under the limit, by truncation at steps 6 to 8: nine steps see both.  The step sources are
    the launch forms of FORMS: single-pass, one environment per lane, grid-stride, and four per lane with a ragged last group (obs_out NULL)"""
    form = {"step": "tile_1024", "step_generic": "generic_1027", "step_grid_stride": "grid_stride_2052", "step_ragged_no_obs_out": "ragged_1027_no_obs_out",
            "table_steps": "generic_1027"}.get(src, "tile_1024")
    env, n, _, with_obs = form_env(form, limit, True, monkeypatch)
    K = 9
    env.set_state(near_swing_up(n).view(F))
    cap = 1 if src.startswith("step") else K
    fb = FinalBuf(cap, 6, n)
    env.set_final_obs_out_device(fb.ptr, cap)
    w = mlp_weights(33)
    used = table_actions(n, K)
    if src.startswith("step"):   # nine mgym_step calls, the one slab checked and refilled after each
        tobs, tfin = twin_finals(n, limit, list(used))
        buf = CallBuffers(n, 6, np.uint32, with_obs=with_obs)
        for t, a in enumerate(used):
            buf.step(env, a)
            fb.check(tobs[t: t + 1], tfin[t: t + 1], f"{src} step {t}")
            fb.fill()
    else:
        if src.startswith("table"):
            env.rollout(used)
        else:
            call = {"uniform": lambda: env.rollout_uniform(PSEED, K), "linear": lambda: env.rollout_linear(SWING, K), "mlp": lambda: env.rollout_mlp(*w, K),
                    "sample": lambda: env.rollout_mlp_sample(*w, K, seed=PSEED, call=3)}[src]
            used = call()[0]
        tobs, tfin = twin_finals(n, limit, list(used))
        fb.check(tobs, tfin, src)
    env.set_final_obs_out_device(None)
    assert tfin[:2].sum() >= 8 and (limit == 0 or tfin[6:].sum() >= 8), "the case has endings of both kinds"


def test_final_observations_cover_done_and_truncated_endings():
    """the seeded states give `done` endings (with the limit off there is nothing else) as well as truncation ones"""
    for limit in (0, LIMIT):
        done = np.array([s[2] for s in reference(1024, limit, True)["steps"]]).astype(bool)
        trunc = np.array([s[3] for s in reference(1024, limit, True)["steps"]]).astype(bool)
        assert done[:9].sum() >= 8 and (limit == 0 or (trunc & ~done)[:9].sum() >= 8)


def test_captured_step_and_rollout_replay_like_eager_calls():
    n, K = 1024, 5
    env, eager = make(n, 2, True), make(n, 2, True)
    for e in (env, eager):
        e.set_state(near_swing_up(n).view(F))
    a = table_actions(n, K)
    buf = CallBuffers(n, 6, np.uint32)
    buf.put_actions(a[:1])
    graph = env.graph_capture(lambda: env.step_device(*buf.pointers()))
    for t in range(3):
        env.graph_launch(graph)
        env.sync()
        assert all(same(g[0], e) for g, e in zip(buf.read(), eager.step(a[0]))), f"step replay {t}"
    env.graph_destroy(graph)
    rb = CallBuffers(n, 6, np.uint32, K)
    rb.put_actions(a)
    graph = env.graph_capture(lambda: env.rollout_device(rb.pointers()[0], K, *rb.pointers()[1:]))
    for t in range(2):
        env.graph_launch(graph)
        env.sync()
        assert all(same(g, e) for g, e in zip(rb.read(), eager.rollout(a))), f"rollout replay {t}"
    env.graph_destroy(graph)
    assert same(env.get_state(), eager.get_state()) and env.episode_count() == eager.episode_count() > 0


def test_torch_vec_env_shapes_and_dtypes():
    torch = pytest.importorskip("torch")
    n, K = 1024, 5
    tenv, env = mg.TorchVecEnv(mg.ACROBOT, n, seed=11, max_episode_steps=LIMIT), mg.VecEnv(mg.ACROBOT, n, seed=11, auto_reset=True, max_episode_steps=LIMIT)
    obs = tenv.reset()
    assert not tenv.action_is_float and tuple(obs.shape) == (6, n) and obs.dtype == torch.float32 and same(obs.cpu().numpy(), env.reset())
    host = lambda g: g.cpu().numpy().view(np.uint8) if g.dtype == torch.bool else g.cpu().numpy()
    acts = table_actions(n, K + 1).astype(np.int32)
    got = tenv.step(torch.from_numpy(acts[0]).cuda(), check=True)
    assert tuple(got[0].shape) == (6, n) and tuple(got[1].shape) == (n,) and got[1].dtype == torch.float32
    assert all(same(host(g), e) for g, e in zip(got, env.step(acts[0].astype(np.uint32))))
    got = tenv.rollout(torch.from_numpy(acts[1:]).cuda())
    tenv.check()
    assert tuple(got[0].shape) == (K, 6, n) and all(same(host(g), e) for g, e in zip(got, env.rollout(acts[1:].astype(np.uint32))))
    w = mlp_weights(33)
    got = tenv.rollout_mlp(*(torch.from_numpy(x) for x in w), K, activation="tanh")
    tenv.check()
    assert got[0].dtype == torch.int32 and tuple(got[0].shape) == (K, n) and tuple(got[1].shape) == (K, 6, n)
    assert all(same(host(g).view(np.uint32) if host(g).dtype == np.int32 else host(g), e) for g, e in zip(got, env.rollout_mlp(*w, K, activation="tanh")))
