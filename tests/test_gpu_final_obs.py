"""The final observations of auto-reset episodes (mgym_set_final_obs_out, include/mgym.h) for CartPole, MountainCar, MountainCarContinuous and Pendulum.

The reference is a TWIN handle of the same kind, configuration and seed WITHOUT MGYM_FLAG_AUTO_RESET (code that predates the channel): before each
step the state of a stepping auto-reset handle with the channel unset is copied into the twin (get_state -> set_state, plus the elapsed count for
MountainCar and Pendulum; CartPole's counters travel in the blob), the twin takes the same actions, and its obs where its done | truncated is set is the
expected final observation.  Policy rollouts are replayed this way from their actions_out.  Everything is compared bit for bit:
  (a) the call under test gives the same obs_out / reward / done / truncated / actions_out (and state, engine observation, episode count) as the same
      call on a handle with the channel unset;
  (b) the finals equal the twin's words at every finished env-step;
  (c) every other word of the buffer (and a guard word on either side) still holds the fill pattern, a NaN word;
  (d) after set(NULL) a further call leaves the buffer untouched.
Each case first asserts, on the twin's flags, that the classes of endings it claims are present (check_coverage).

Shapes: n = 2052 is two full 1024-env tiles plus one lane; n = 1030 (not a multiple of 4) and a misaligned reward buffer take the one-env-per-lane
kernels and mgym_rollout's K x step form; MGYM_CLASSIC_MAX_BLOCKS=1 gives the grid-stride form of the 4-per-lane step kernels; a final-observation
buffer 4 bytes off a 16-byte boundary is accepted everywhere (its stores are 4-byte ones)."""
import numpy as np
import pytest

import modurl_gym_amd as mg
from modurl_gym_amd import _lib
from device_buffers import FILL, CallBuffers, FinalBuf, copy_state, policy_call, twin_steps
from families import BY_KIND, FAMILIES as FAM
from words import bits, same

pytestmark = pytest.mark.gpu

SEED, PSEED, H, N = 2024, 77, 8, 2052
LIMIT = 7
MC_KINDS = (mg.MOUNTAINCAR, mg.MOUNTAINCAR_CONT)
DISCRETE_SRC = ["table", "uniform", "linear", "mlp_relu", "mlp_tanh", "sample_relu", "sample_tanh"]
BOX_SRC = ["table", "uniform", "linear", "mlp_relu", "mlp_tanh", "gauss_relu", "gauss_tanh"]
CASES = [("cartpole", 0), ("mountain_car", LIMIT), ("mountain_car", 0), ("mountain_car_continuous", LIMIT), ("mountain_car_continuous", 0), ("pendulum", LIMIT)]
FAMILIES = [(FAM[f].kind, lim, DISCRETE_SRC if FAM[f].box is None else BOX_SRC) for f, lim in CASES]
FAMILY_IDS = ["cartpole", "mountaincar-tl", "mountaincar", "mountaincar_cont-tl", "mountaincar_cont", "pendulum-tl"]   # the cases' ids, kept as they were
SOURCE_CASES = [pytest.param(k, lim, s, id=f"{fid}-{s}") for (k, lim, srcs), fid in zip(FAMILIES, FAMILY_IDS) for s in srcs]
KIND_CASES = [pytest.param(k, lim, id=fid) for (k, lim, _), fid in zip(FAMILIES, FAMILY_IDS)]


def make(kind, n, limit, auto_reset=True):
    return mg.VecEnv(kind, n, seed=SEED, auto_reset=auto_reset, max_episode_steps=limit)


# ---- inputs that make endings sparse and mixed within a lane --------------------------------------------------------------------------
def staggered_elapsed(n, limit):
    """counts 0 .. limit - 1 from a seeded permutation: a lane's four environments finish on different steps; lanes 0 .. limit - 1 hold one count each,
    so that all four of a lane finish on one step as well"""
    el = (np.random.default_rng(11).permutation(n) % limit).astype(np.uint32)
    for lane in range(limit):
        el[4 * lane: 4 * lane + 4] = lane
    return el


def prep(env, limit):
    """reset, then the family's imported states and counts; the same for every handle of a case"""
    kind, n = env.kind, env.n
    env.reset()
    rng = np.random.default_rng(5)
    if kind == mg.CARTPOLE:
        blob = env.get_state().copy()
        w = blob.view(np.uint32)

        def near_500(idx, steps):   # near-zero pole, step counter just short of the 500-step limit: truncated-only endings
            blob[0:4, idx] = rng.uniform(-0.01, 0.01, (4, len(idx))).astype(np.float32)
            w[4, idx] = steps
        idx = np.arange(256, 512)
        near_500(idx, 497 + idx % 3)
        if n > 1164:
            idx = np.arange(1100, 1164)   # the second tile
            near_500(idx, 497 + idx % 3)
        tail = np.arange(n - (n % 4 or 4), n)   # the last lane (or the ragged tail): all of it at once
        near_500(tail, np.full(len(tail), 499))
        blob[2, 512:768] = 0.3   # one 256-env wave wholly beyond the angle threshold (12 degrees = 0.2095): it finishes at once, two draw passes
        env.set_state(blob)
        return
    if kind in MC_KINDS:
        blob = env.get_state().copy()
        goal = 0.45 if kind == mg.MOUNTAINCAR_CONT else 0.5
        idx = np.arange(256, 768)
        j = np.where(idx < 512, (idx // 4) % 3, idx % 3)   # reaches the goal at step j: whole lanes together (256 ..), mixed within a lane (512 ..)
        blob[0, idx] = (goal - 0.05 * j - 0.02).astype(np.float32)
        blob[1, idx] = 0.05
        env.set_state(blob)   # (zeroes the elapsed counts)
    if limit:
        env.set_elapsed_steps(staggered_elapsed(n, limit))


def table_actions(kind, K, n):
    rng = np.random.default_rng(3)
    if kind == mg.PENDULUM:
        return rng.uniform(-2.5, 2.5, (K, n)).astype(np.float32)   # beyond [-2, 2]: the step clamps
    if kind == mg.MOUNTAINCAR_CONT:
        return rng.uniform(-1.5, 1.5, (K, n)).astype(np.float32)
    return rng.integers(0, 2 if kind == mg.CARTPOLE else 3, (K, n)).astype(np.uint32)


def policies(env):
    rng = np.random.default_rng(9)
    D, A = env.mlp_dims()
    mlp, _ = env.pack_mlp(rng.normal(0, 1, (H, D)), rng.normal(0, 1, H), rng.normal(0, 1, (A, H)), rng.normal(0, 1, A))
    return dict(linear=rng.normal(0, 1, BY_KIND[env.kind].lin).astype(np.float32), mlp=mlp)


def buffers(env, K, mis_rew=0, with_obs=True):
    """device buffers of one K-step call; mis_rew = 1 puts the reward buffer 4 bytes off a 16-byte boundary (the one-env-per-lane kernels)"""
    return CallBuffers(env.n, env.obs_dim, env.action_dtype, K, 4 * mis_rew, with_obs)


def do_call(env, src, K, o):
    """the call of the source on o, whose actions a step or a table reads"""
    p = policies(env)
    policy_call(env, src, K, o, p["linear"], (p["mlp"], H), PSEED, 3, 0.5)


def twin_replay(kind, n, limit, actions, mis_rew=0, with_obs=True):
    """K single steps of an auto-reset handle with the channel unset, its state copied into the twin before each (device_buffers.twin_steps): -> (the
    stepping handle's outputs, the twin's obs [K, D, n], done and truncated [K, n]).  The twin steps on buffers of the case's shape (mis_rew, with_obs),
    so the launch form under test runs without auto-reset as well; without obs_out its observation is the engine's view."""
    stepper, twin = make(kind, n, limit), make(kind, n, limit, auto_reset=False)
    prep(stepper, limit)
    twin.reset()
    res = twin_steps(stepper, twin, actions, buffers(twin, 1, mis_rew, with_obs).step)
    stepper.close(), twin.close()
    return res


def check_coverage(kind, limit, d, t):
    """the classes of endings a case claims, on the twin's flags"""
    K, n = d.shape
    fin = d | t
    has_done, has_trunc = kind != mg.PENDULUM, kind == mg.CARTPOLE or limit != 0
    if not (has_done or has_trunc):   # Pendulum without a limit: nothing ever finishes
        assert not fin.any()
        return
    if has_done and has_trunc:
        assert (d & ~t).sum() >= 8 and (~d & t).sum() >= 8, "done-only and truncated-only endings"
    assert fin.sum() >= 8
    if kind in MC_KINDS and limit:
        assert (d & t).sum() >= 1, "an ending with both flags"
    per_lane = fin[:, : n // 4 * 4].reshape(K, -1, 4).sum(axis=2)
    assert (per_lane == 1).any() and (per_lane == 4).any(), "a lane with exactly one finished environment and one with all four"
    if kind == mg.CARTPOLE:
        assert fin[0, 512:768].sum() >= 33, "more than 32 endings in one wave: two draw passes"


def run_case(kind, limit, src, K, n=N, mis_fin=0, mis_rew=0, with_obs=True):
    what = f"{mg.envs.KIND_NAMES[kind]} limit {limit} {src} K={K} n={n}"
    cap = K + 1
    is_table = src in ("step", "table")
    acts = table_actions(kind, K, n)
    res = {}
    for mode in ("unset", "set"):
        env = make(kind, n, limit)
        prep(env, limit)
        o = buffers(env, K, mis_rew, with_obs)
        if is_table:
            o.put_actions(acts)
        if mode == "set":
            fb = FinalBuf(cap, env.obs_dim, env.n, mis_fin)
            env.set_final_obs_out_device(fb.ptr, cap)
        do_call(env, src, K, o)
        res[mode] = dict(o.host(), state=env.get_state(), view=env.observation(), count=np.array([env.episode_count()]))
        if limit and kind != mg.CARTPOLE:
            res[mode]["elapsed"] = env.elapsed_steps()
        env.close()
    for key, got in res["set"].items():   # (a)
        assert same(got, res["unset"][key]), f"{what}: {key} differs from the same call with the channel unset"
    used = acts if is_table else res["set"]["act"]
    outs, tobs, tdone, ttrunc = twin_replay(kind, n, limit, used, mis_rew, with_obs)
    for t, (so, sr, sd, st) in enumerate(outs):   # the call is K steps of the stepping handle, so the twin saw the states the call went through
        got = res["set"]
        assert same(got["rew"][t], sr) and same(got["done"][t], sd) and same(got["trunc"][t], st) and (not with_obs or same(got["obs"][t], so)), f"{what}: step {t}"
    check_coverage(kind, limit, tdone, ttrunc)
    fb.check(tobs, tdone | ttrunc, what)   # (b), (c)


# ---- every action source, fused kernels -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 5, 16])
@pytest.mark.parametrize("kind,limit,src", SOURCE_CASES)
def test_rollout_sources(kind, limit, src, K):
    run_case(kind, limit, src, K)


def test_cartpole_uniform_rollout_64_steps():
    """`done` endings throughout, the imported counters' truncations at steps 0 .. 2 and the whole wave at step 0"""
    run_case(mg.CARTPOLE, 0, "uniform", 64)


@pytest.mark.parametrize("kind,limit", KIND_CASES)
def test_policy_rollout_with_misaligned_final_buffer(kind, limit):
    run_case(kind, limit, "uniform", 5, mis_fin=1)


# ---- mgym_step: every launch form -----------------------------------------------------------------------------------------------------
STEP_SHAPES = {"tiles": dict(), "odd": dict(n=1030), "odd_no_obs": dict(n=1030, with_obs=False), "misaligned_reward": dict(mis_fin=1, mis_rew=1),
               "misaligned_final": dict(mis_fin=1), "grid_stride": dict()}


@pytest.mark.parametrize("shape", list(STEP_SHAPES))
@pytest.mark.parametrize("kind,limit", KIND_CASES + [pytest.param(mg.PENDULUM, 0, id="pendulum")])
def test_step_launch_forms(kind, limit, shape, monkeypatch):
    """4 per lane single-pass (tiles), one env per lane (odd, misaligned_reward), 4 per lane with a ragged last group (odd_no_obs: MountainCar and
    Pendulum), 4 per lane grid-stride (MGYM_CLASSIC_MAX_BLOCKS=1, read when a handle is created: three passes of one block).  Each with auto-reset and the
    channel unset, with the channel set, and (the twin) without auto-reset.  Pendulum without a limit: the forms that never finish and never write."""
    if shape == "grid_stride":
        monkeypatch.setenv("MGYM_CLASSIC_MAX_BLOCKS", "1")
    else:
        monkeypatch.delenv("MGYM_CLASSIC_MAX_BLOCKS", raising=False)
    run_case(kind, limit, "step", 1, **STEP_SHAPES[shape])


# ---- mgym_rollout: the K x step form --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,K", [("odd", 5), ("odd", 16), ("misaligned_reward", 5), ("misaligned_final", 5)])
@pytest.mark.parametrize("kind,limit", KIND_CASES)
def test_table_rollout_shapes(kind, limit, shape, K):
    """n % 4 != 0 or a misaligned output: K plain steps, step t writing slab t; a misaligned final buffer alone keeps the fused kernel"""
    run_case(kind, limit, "table", K, **STEP_SHAPES[shape])


# ---- (d) and the handle's bookkeeping -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,limit,K", [(mg.CARTPOLE, 0, 64), (mg.MOUNTAINCAR, LIMIT, 16), (mg.MOUNTAINCAR_CONT, LIMIT, 16), (mg.PENDULUM, LIMIT, 16)])
def test_null_turns_the_channel_off(kind, limit, K):
    env = make(kind, N, limit)
    prep(env, limit)
    fb = FinalBuf(K, env.obs_dim, env.n)
    env.set_final_obs_out_device(fb.ptr, K)
    o = buffers(env, K)
    do_call(env, "uniform", K, o)
    before = fb.dev.numpy()
    assert (before != FILL).any()
    env.set_final_obs_out_device(None)
    do_call(env, "uniform", K, o)
    h = o.host()
    assert (h["done"] | h["trunc"]).sum() >= 8, "the further call has endings of its own"
    assert np.array_equal(fb.dev.numpy(), before)
    env.set_final_obs_out_device(fb.ptr, K)   # ... and on again: replaced, not latched off
    fb.fill()
    do_call(env, "uniform", K, o)
    assert (fb.dev.numpy() != FILL).any()
    env.close()


def test_pendulum_without_a_limit_never_writes():
    """nothing ever finishes: the call is accepted, launches the kernels it always did, and the buffer keeps its fill"""
    res = []
    for with_channel in (False, True):
        env = make(mg.PENDULUM, N, 0)
        env.reset()
        fb = FinalBuf(5, env.obs_dim, env.n)
        if with_channel:
            env.set_final_obs_out_device(fb.ptr, 5)
        o = buffers(env, 5)
        do_call(env, "uniform", 5, o)
        do_call(env, "step", 1, o)
        res.append(dict(o.host(), state=env.get_state()))
        assert (fb.dev.numpy() == FILL).all()
        env.close()
    assert all(same(res[1][k], res[0][k]) for k in res[0])


# ---- errors ---------------------------------------------------------------------------------------------------------------------------
def bad_arg(fn, *needles):
    with pytest.raises(mg.MgymError) as e:
        fn()
    assert e.value.status == _lib.ERR_BAD_ARG and all(s in str(e.value) for s in needles), str(e.value)


def test_errors_of_the_setter():
    buf = mg.DeviceArray(16 * 4 * 8, np.float32)
    plain = make(mg.CARTPOLE, 8, 0, auto_reset=False)
    bad_arg(lambda: plain.set_final_obs_out_device(buf, 16), "final_obs_out", "MGYM_FLAG_AUTO_RESET", "obs_out already holds the final observation")
    plain.set_final_obs_out_device(None)         # NULL is always accepted
    plain.set_final_obs_out_device(None, -3)     # ... whatever steps_cap says
    plain.close()
    env = make(mg.CARTPOLE, 8, 0)
    bad_arg(lambda: env.set_final_obs_out_device(buf, 0), "steps_cap")
    bad_arg(lambda: env.set_final_obs_out_device(buf, -1), "steps_cap")
    bad_arg(lambda: env.set_final_obs_out_device(buf.ptr + 2, 4), "final_obs_out", "4-byte aligned")
    env.set_final_obs_out_device(buf.ptr + 4, 4)   # no 16-byte requirement
    env.set_final_obs_out_device(None)
    env.close()
    ll = make(mg.LUNARLANDER, 8, 0)
    bad_arg(lambda: ll.set_final_obs_out_device(buf, 16), "final_obs_out", "LunarLander")
    ll.set_final_obs_out_device(None)
    ll.close()


@pytest.mark.parametrize("kind,limit", KIND_CASES)
def test_more_steps_than_the_cap(kind, limit):
    """refused before any launch, the message naming the entry point, the state untouched; K <= cap and mgym_step go on working"""
    n, cap, K = 1028, 4, 5
    env = make(kind, n, limit)
    prep(env, limit)
    fb = FinalBuf(cap, env.obs_dim, env.n)
    env.set_final_obs_out_device(fb.ptr, cap)
    o = buffers(env, K)
    o.put_actions(table_actions(kind, K, n))
    state, view, count = env.get_state(), env.observation(), env.episode_count()
    sources = {"table": "mgym_rollout:", "uniform": "mgym_rollout_uniform:", "linear": "mgym_rollout_linear:", "mlp_relu": "mgym_rollout_mlp:"}
    sources["sample_tanh" if kind in (mg.CARTPOLE, mg.MOUNTAINCAR) else "gauss_tanh"] = "mgym_rollout_mlp_sample:" if kind in (mg.CARTPOLE, mg.MOUNTAINCAR) else "mgym_rollout_mlp_gauss:"
    for src, name in sources.items():
        bad_arg(lambda: do_call(env, src, K, o), name, "steps_cap")
        env.sync()
        assert same(env.observation(), view) and same(env.get_state(), state) and env.episode_count() == count, src
        assert (fb.dev.numpy() == FILL).all(), src
    do_call(env, "table", cap, o)
    do_call(env, "step", 1, o)
    env.close()


# ---- graph capture: the pointer is frozen, each replay indexes t from 0 ---------------------------------------------------------------
@pytest.mark.parametrize("kind,limit", [(mg.CARTPOLE, 0), (mg.MOUNTAINCAR, LIMIT), (mg.MOUNTAINCAR_CONT, LIMIT), (mg.PENDULUM, LIMIT)])
def test_graph_replay_of_a_step(kind, limit):
    env, twin = make(kind, N, limit), make(kind, N, limit, auto_reset=False)
    prep(env, limit)
    twin.reset()
    acts = table_actions(kind, 1, N)
    o, fb = buffers(env, 1), FinalBuf(1, env.obs_dim, env.n)
    o.put_actions(acts)
    env.set_final_obs_out_device(fb.ptr, 1)
    g = env.graph_capture(lambda: env.step_device(*o.pointers()))
    env.set_final_obs_out_device(None)   # later settings leave the captured launch what it was (and the graph valid)
    try:
        for rep in range(2):
            copy_state(env, twin)
            fb.fill()
            env.graph_launch(g)
            env.sync()
            tobs, _, td, tt = twin.step(acts[0])
            fin = (td | tt).astype(bool)
            assert fin.sum() >= 8, f"replay {rep} has endings"
            h = o.host()
            assert same(h["done"][0], td) and same(h["trunc"][0], tt)
            fb.check(tobs[None], fin[None], f"{mg.envs.KIND_NAMES[kind]} replay {rep}")
    finally:
        env.graph_destroy(g)
    env.close(), twin.close()


# ---- TorchVecEnv ----------------------------------------------------------------------------------------------------------------------
def test_torch_env_bootstrap_obs():
    torch = pytest.importorskip("torch")
    from modurl_gym_amd.torch_env import TorchVecEnv
    K = 16
    with pytest.raises(ValueError):
        TorchVecEnv(mg.PENDULUM, 8, seed=SEED, obs_layout="aos", final_obs_steps=K, max_episode_steps=LIMIT)
    env = TorchVecEnv(mg.PENDULUM, N, seed=SEED, final_obs_steps=K, max_episode_steps=LIMIT)
    assert tuple(env.final_obs.shape) == (K, 3, N) and env.final_obs.dtype == torch.float32
    env.reset()
    env.set_elapsed_steps(torch.from_numpy(staggered_elapsed(N, LIMIT).astype(np.int32)).to(env.device))
    rng = np.random.default_rng(9)
    w1, b1, w2, b2 = (rng.normal(0, 1, s).astype(np.float32) for s in ((H, 3), (H,), (1, H), (1,)))
    act, obs, rew, done, trunc = env.rollout_mlp_gauss(w1, b1, w2, b2, K, 0.5, PSEED, 3)
    boot = env.bootstrap_obs(obs, done, trunc)
    env.check()
    _, tobs, tdone, ttrunc = twin_replay(mg.PENDULUM, N, LIMIT, act.cpu().numpy())
    fin = tdone | ttrunc
    check_coverage(mg.PENDULUM, LIMIT, tdone, ttrunc)
    assert same((done | trunc).cpu().numpy(), fin)
    expected = np.where(fin[:, None, :], bits(tobs), bits(obs.cpu().numpy()))
    assert np.array_equal(bits(boot.cpu().numpy()), expected)
    env.close()
