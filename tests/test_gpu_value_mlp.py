"""mgym_value_mlp on the device against the numpy restatement of its text (tests/value_ref.py), word for word (words.same: exact words).

Inputs are synthetic, from seeded generators (value_ref.case): observations uniform inside each family's bounds, flag bytes of any non-zero value with the first
waves of the final pass patched by hand (0, exactly 1, exactly 64, 65 and every env-step selected; value_ref.check_coverage asserts them before a case is used).
final_obs holds a NaN word wherever the text does not read it; every output is pre-filled with that word between two guards: each word the text writes must have
been written, no other word — guards included — may have been, and the inputs are untouched.

Shapes: n = 2052 is two 1024-environment tiles of the four-per-lane kernel plus one lane, and eight waves of the final pass plus four environments; n = 1030
(not a multiple of 4) and an obs buffer 4 bytes off a 16-byte boundary take the one-environment-per-lane kernel (1030: the flags as bytes); K = 1, 2 and 17 (one
step beyond a chunk of the final pass)."""
import functools

import numpy as np
import pytest

import device_buffers
import families
import gae_ref
import mlp2_ref
import modurl_gym_amd as mg
import value_ref as R
from modurl_gym_amd import _lib
from words import same

pytestmark = pytest.mark.gpu

F = np.float32
N = 2052
KS = (1, 2, 17)
Guarded = functools.partial(device_buffers.Guarded, fill=R.POISON)
bad_arg = lambda fn, *needles: device_buffers.bad_arg(fn, "mgym_value_mlp", *needles)


@functools.lru_cache(maxsize=None)
def expected(family, K, n, widths, act, with_final=True, with_d=True):
    c = R.case(family, K, n)
    crit, _ = R.critic(family, widths)
    fo = (c["final_obs_d"] if with_d else c["final_obs_nd"]) if with_final else None
    return R.value_mlp(crit, c["D"], widths, act, c["obs_first"], c["obs"], fo, c["d"] if with_d else None, c["u"] if with_final else None)


class Slabs:
    def __init__(self, family, K, n, mis_obs=0, with_final=True, with_d=True, case=None):
        c = case or R.case(family, K, n)
        self.c, self.K, self.n, self.with_final, self.with_d = c, K, n, with_final, with_d
        D = c["D"]
        self.obs_first, self.obs = Guarded(D * n, 0, c["obs_first"]), Guarded(K * D * n, mis_obs, c["obs"])
        self.final_obs = Guarded(K * D * n, 0, c["final_obs_d"] if with_d else c["final_obs_nd"]) if with_final else None
        self.d = mg.DeviceArray.from_numpy(c["d"]) if with_d else None
        self.u = mg.DeviceArray.from_numpy(c["u"]) if with_final else None
        self.value, self.last = Guarded(K * n), Guarded(n)
        self.final = Guarded(K * n) if with_final else None

    def call(self, env, critic, widths, act):
        env.value_mlp_device(critic, widths[0], (*widths, 0)[1], act, self.K, self.obs_first, self.obs, self.final_obs, self.d, self.u, self.value, self.last, self.final)

    def outputs_untouched(self):
        return all(b.untouched() for b in (self.value, self.last, self.final) if b is not None)

    def inputs_untouched(self):
        return (all(b.untouched() for b in (self.obs_first, self.obs, self.final_obs) if b is not None)
                and (self.d is None or same(self.d.numpy(), self.c["d"])) and (self.u is None or same(self.u.numpy(), self.c["u"])))

    def check(self, exp, what):
        K, n = self.K, self.n
        for name, buf, e, shape in (("value_out", self.value, exp[0], (K, n)), ("last_value_out", self.last, exp[1], (n,))):
            got = buf.payload(shape, F)
            assert (got.view(np.uint32) != R.POISON).all(), f"{what}: {name} has words that were not written"
            assert same(got, e), f"{what}: {int((got.view(np.uint32) != e.view(np.uint32)).sum())} words of {name} differ from the restatement"
            assert buf.guards_hold(), f"{what}: a guard word of {name} was written"
        if self.final is not None:
            got, sel = self.final.payload((K, n)), R.selection(self.c["d"] if self.with_d else None, self.c["u"])
            assert (got[~sel] == R.POISON).all(), f"{what}: {int((got[~sel] != R.POISON).sum())} words of final_value_out outside the selection were written"
            assert same(got, exp[2]), f"{what}: {int((got != exp[2]).sum())} selected words of final_value_out differ from the restatement"
            assert np.isfinite(got[sel].view(F)).all() and self.final.guards_hold(), f"{what}: final_value_out"
        assert self.inputs_untouched(), f"{what}: an input was written"


def run(env, family, K, n, widths, act, **kw):
    b = Slabs(family, K, n, **kw)
    b.call(env, R.critic(family, widths)[0], widths, act)
    env.sync()
    b.check(expected(family, K, n, widths, act, kw.get("with_final", True), kw.get("with_d", True)), f"{family} K={K} n={n} {widths} act={act} {kw}")


@pytest.fixture(scope="module")
def env():
    e = mg.VecEnv(mg.CARTPOLE, N)
    yield e
    e.close()


@pytest.fixture(scope="module")
def pend():
    e = mg.VecEnv(mg.PENDULUM, N, seed=5, auto_reset=True)
    e.reset()
    yield e
    e.close()


@pytest.mark.parametrize("with_d", [True, False], ids=["done", "done-null"])
@pytest.mark.parametrize("K", KS)
def test_four_per_lane(env, K, with_d):
    run(env, "cartpole", K, N, (17,), R.TANH, with_d=with_d)
    run(env, "cartpole", K, N, (3, 5), R.TANH_FAST, with_d=with_d)


def test_without_the_final_triple(env):
    """final_obs and final_value_out NULL: done and trunc are ignored (trunc NULL here; test_errors passes them non-NULL)"""
    run(env, "cartpole", 17, N, (17,), R.RELU, with_final=False, with_d=False)
    run(env, "cartpole", 2, N, (17, 33), R.RELU, with_final=False, with_d=True)


@pytest.mark.parametrize("widths", R.WIDTHS, ids=str)
def test_widths(pend, widths):
    for act in R.ACTS[len(widths)]:
        run(pend, "pendulum", 2, N, widths, act)


@pytest.mark.parametrize("K", [1, 17])
def test_one_per_lane(K):
    e = mg.VecEnv(mg.MOUNTAINCAR, 1030)
    run(e, "mountain_car", K, 1030, (17,), R.RELU)
    run(e, "mountain_car", K, 1030, (3, 5), R.RELU, with_d=False)
    e.close()


def test_more_rows_than_the_grid_holds():
    """K = 65 540 at n = 4 on MountainCar with H = 3, without the final triple: rows 65 535 .. 65 540 of the K + 1 come from the stride loop; then one per lane
    (n = 5) with the same K"""
    K, widths = 65540, (3,)
    crit = R.critic("mountain_car", widths)[0]
    for n in (4, 5):
        rng = np.random.default_rng(n)
        c = dict(D=2, obs_first=R.observations(rng, "mountain_car", (), n), obs=R.observations(rng, "mountain_car", (K,), n))
        e = mg.VecEnv(mg.MOUNTAINCAR, n)
        b = Slabs("mountain_car", K, n, with_final=False, with_d=False, case=c)
        b.call(e, crit, widths, R.RELU)
        e.sync()
        b.check(R.value_mlp(crit, 2, widths, R.RELU, c["obs_first"], c["obs"]), f"K={K} n={n}")
        e.close()


@pytest.mark.parametrize("K", [2, 17])
def test_misaligned_obs(env, K):
    run(env, "cartpole", K, N, (17,), R.TANH_FAST, mis_obs=1)
    run(env, "cartpole", K, N, (17, 33), R.TANH_FAST, mis_obs=1)


@pytest.mark.parametrize("family", ["mountain_car", "pendulum", "cartpole", "acrobot", "lunar_lander"])
def test_every_kind(family):
    """D = 2, 3, 4, 6, 8 at K = 2, every accepted (depth, activation): n = 1028 (four per lane, the flags as words) and n = 1030 (one per lane, the flags as
    bytes) — every instantiation of the three kernels in both forms of the flags.  The LunarLander handle was never reset and still is not afterwards"""
    for n in (1028, 1030):
        e = mg.VecEnv(families.KIND[family], n)
        for widths in ((17,), (3, 5)):
            for act in R.ACTS[len(widths)]:
                run(e, family, 2, n, widths, act, with_d=(act != R.RELU) or n == 1030)
        if family == "lunar_lander":
            assert e.episode_count() == 0
            with pytest.raises(mg.NotResetError):
                e.step(np.zeros(n, np.uint32))
        e.close()


@pytest.mark.parametrize("act", (R.RELU, R.TANH_FAST))
def test_a_signed_zero_reaches_value_out(pend, act):
    """mlp2_ref.signed_zero_policy gives 0x80000000 everywhere; a chain padded with zero weights would give 0"""
    b = Slabs("pendulum", 2, N)
    b.call(pend, R.packed(mlp2_ref.signed_zero_policy(3, act)), (3, 5), act)
    pend.sync()
    sel = R.selection(b.c["d"], b.c["u"])
    assert (b.value.payload((2, N)) == 0x80000000).all() and (b.last.payload((N,)) == 0x80000000).all()
    got = b.final.payload((2, N))
    assert (got[sel] == 0x80000000).all() and (got[~sel] == R.POISON).all()


def actor_weights():
    rng = np.random.default_rng(31)
    return mlp2_ref.packed(mlp2_ref.normal_weights(rng, 3, 1, 9, 12, (1.0, 1.0, 0.125))), 9, 12


def rollout_alone(K):
    """the words of the actor's mgym_rollout_mlp2 on a handle of pend's seed that runs nothing else"""
    twin = mg.VecEnv(mg.PENDULUM, N, seed=5, auto_reset=True)
    twin.reset()
    bufs = device_buffers.CallBuffers(N, 3, F, K)
    twin.rollout_mlp2_device(*actor_weights(), "tanh_fast", "greedy", 0.0, 0, 0, K, *bufs.pointers())
    twin.sync()
    out = bufs.host()
    twin.close()
    return out


def test_two_critics_and_an_actor_back_to_back():
    """two two-layer calls with different critics and a mgym_rollout_mlp2 between them, no synchronisation in between: each gives its own words"""
    K = 2
    e = mg.VecEnv(mg.PENDULUM, N, seed=5, auto_reset=True)
    e.reset()
    a, b = Slabs("pendulum", K, N), Slabs("pendulum", K, N)
    bufs = device_buffers.CallBuffers(N, 3, F, K)
    a.call(e, R.critic("pendulum", (17, 33))[0], (17, 33), R.TANH_FAST)
    e.rollout_mlp2_device(*actor_weights(), "tanh_fast", "greedy", 0.0, 0, 0, K, *bufs.pointers())
    b.call(e, R.critic("pendulum", (64, 64))[0], (64, 64), R.TANH_FAST)
    e.sync()
    a.check(expected("pendulum", K, N, (17, 33), R.TANH_FAST), "first critic")
    b.check(expected("pendulum", K, N, (64, 64), R.TANH_FAST), "second critic")
    assert not same(a.value.payload((K, N)), b.value.payload((K, N)))
    got, alone = bufs.host(), rollout_alone(K)
    assert all(same(got[k], alone[k]) for k in alone), "the actor's rollout between two critic calls"
    e.close()


def test_graph_replay_equals_the_eager_calls():
    """one graph holding a mgym_rollout_mlp2 and a two-layer mgym_value_mlp: capture launches nothing, the replay gives each call its own weights"""
    K = 2
    e = mg.VecEnv(mg.PENDULUM, N, seed=5, auto_reset=True)
    e.reset()
    b, one = Slabs("pendulum", K, N), Slabs("pendulum", K, N)
    bufs = device_buffers.CallBuffers(N, 3, F, K)
    state = e.get_state()

    def both():
        e.rollout_mlp2_device(*actor_weights(), "tanh_fast", "greedy", 0.0, 0, 0, K, *bufs.pointers())
        b.call(e, R.critic("pendulum", (17, 33))[0], (17, 33), R.TANH_FAST)
        one.call(e, R.critic("pendulum", (17,))[0], (17,), R.TANH)

    g = e.graph_capture(both)
    try:
        e.sync()
        assert b.outputs_untouched() and one.outputs_untouched() and same(e.get_state(), state)   # capture launches nothing
        e.graph_launch(g)
        e.sync()
        b.check(expected("pendulum", K, N, (17, 33), R.TANH_FAST), "graph replay, two layers")
        one.check(expected("pendulum", K, N, (17,), R.TANH), "graph replay, one layer")
        got, alone = bufs.host(), rollout_alone(K)
        assert all(same(got[k], alone[k]) for k in alone), "the actor's rollout in the same graph"
    finally:
        e.graph_destroy(g)
        e.close()


def test_host_array_form(env):
    """VecEnv.value_mlp: numpy in, numpy out, the same words; final_value 0 where not written, None without final_obs"""
    K, widths = 2, (17, 33)
    c, (_, w) = R.case("cartpole", K, N), R.critic("cartpole", widths)
    exp = expected("cartpole", K, N, widths, R.RELU)
    v, last, fv = env.value_mlp(w, c["obs_first"], c["obs"], c["final_obs_d"], c["d"], c["u"], "relu")
    sel = R.selection(c["d"], c["u"])
    assert same(v, exp[0]) and same(last, exp[1]) and same(fv.view(np.uint32)[sel], exp[2][sel]) and (fv.view(np.uint32)[~sel] == 0).all()
    v, last, fv = env.value_mlp(w, c["obs_first"], c["obs"], activation="relu")
    assert same(v, exp[0]) and same(last, exp[1]) and fv is None
    with pytest.raises(mg.PolicyShapeError):
        env.value_mlp(w[:5], c["obs_first"], c["obs"])


def test_no_environments():
    e = mg.VecEnv(mg.CARTPOLE, 0)
    x, crit = mg.DeviceArray(16, F), R.critic("cartpole", (17,))[0]
    e.value_mlp_device(crit, 17, 0, "relu", 3, x, x.ptr + 16, None, None, None, Guarded(4), Guarded(4), None)   # MGYM_OK without a launch
    with pytest.raises(mg.MgymError):
        e.value_mlp_device(crit, 17, 0, "relu", 0, x, x.ptr + 16, None, None, None, Guarded(4), Guarded(4), None)   # ... after the argument checks
    e.close()


def test_errors(env):
    K, widths = 2, (17,)
    b = Slabs("cartpole", K, N)
    crit = R.critic("cartpole", widths)[0]
    crit2 = R.critic("cartpole", (17, 33))[0]
    lib, h = env._lib, env._h
    ICRIT, IH1, IH2, IACT, IK, IOF, IOBS, IFO, ID, IU, IV, ILV, IFV = range(13)
    ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.data_ptr())
    good = [crit, 17, 0, _lib.ACT_RELU, K, b.obs_first, b.obs, b.final_obs, b.d, b.u, b.value, b.last, b.final]

    def call(repl):
        args = list(good)
        for k, v in repl.items():
            args[k] = v
        c = args[ICRIT]
        fp = None if c is None else np.ascontiguousarray(c, F).ctypes.data_as(_lib.C.POINTER(_lib.C.c_float))
        return lambda: mg.envs._check(lib.mgym_value_mlp(h, fp, *args[IH1: IK + 1], *(ptr(x) for x in args[IOF:])))

    rows = [({IK: 0}, "K"), ({IK: -1}, "K"), ({ICRIT: None}, "critic"), ({IOF: None}, "obs_first"), ({IOBS: None}, "obs"), ({IV: None}, "value_out"),
            ({ILV: None}, "last_value_out"), ({IH1: 0}, "hidden1"), ({IH1: 65}, "hidden1"), ({IH2: -1}, "hidden2"), ({IH2: 65}, "hidden2"),
            ({IACT: 2}, "activation"), ({IACT: 4}, "activation"), ({IACT: -1}, "activation"),
            ({ICRIT: crit2, IH2: 33, IACT: _lib.ACT_TANH}, "activation", "MGYM_ACT_TANH"),
            ({IFO: None}, "final_obs"), ({IFV: None}, "final_value_out"), ({IU: None}, "trunc"), ({IFO: None, IU: None}, "final_obs"),
            ({IOF: b.obs_first.ptr + 2}, "obs_first", "4-byte aligned"), ({IOBS: b.obs.ptr + 1}, "obs", "4-byte aligned"),
            ({IFO: b.final_obs.ptr + 2}, "final_obs", "4-byte aligned"), ({IV: b.value.ptr + 2}, "value_out", "4-byte aligned"),
            ({ILV: b.last.ptr + 3}, "last_value_out", "4-byte aligned"), ({IFV: b.final.ptr + 2}, "final_value_out", "4-byte aligned"),
            ({IV: b.obs_first.ptr}, "value_out", "obs_first"), ({ILV: b.obs.ptr}, "last_value_out", "obs"), ({IFV: b.final_obs.ptr}, "final_value_out", "final_obs"),
            ({IV: b.d.ptr}, "value_out", "done"), ({IFV: b.u.ptr}, "final_value_out", "trunc"),
            ({IV: b.last.ptr}, "value_out is the same pointer as last_value_out"), ({IFV: b.value.ptr}, "final_value_out", "value_out"),
            # two faults: the earlier group's is the one reported — K, the NULLs, widths and activation, the final triple, alignment, aliasing
            ({IK: 0, ICRIT: None}, "K must be"), ({IV: None, IH1: 0}, "value_out is NULL"), ({IH1: 0, IFV: None}, "hidden1 must be"),
            ({IFV: None, IOBS: b.obs.ptr + 1}, "final_value_out is NULL"), ({IOBS: b.obs.ptr + 1, IV: b.last.ptr}, "obs must be 4-byte aligned")]
    state = env.get_state()
    for repl, *needles in rows:
        bad_arg(call(repl), *needles)
    env.sync()
    assert b.inputs_untouched() and b.outputs_untouched() and same(env.get_state(), state)
    call({})()
    env.sync()
    b.check(expected("cartpole", K, N, widths, R.RELU), "after the refused calls")
    # without the final arguments done and trunc are ignored, whatever they point to
    c = Slabs("cartpole", K, N)
    env.value_mlp_device(crit, 17, 0, "relu", K, c.obs_first, c.obs, None, c.value.ptr, c.value.ptr, c.value, c.last, None)
    env.sync()
    assert same(c.value.payload((K, N), F), expected("cartpole", K, N, widths, R.RELU)[0]) and c.final.untouched()


def test_torch_collector_end_to_end():
    """Pendulum under a 7-step limit with staggered elapsed counts, a Gaussian MLP collector: rollout_mlp_gauss -> TorchVecEnv.value_mlp -> TorchVecEnv.gae equals
    gae_ref.gae fed value_ref's values, word for word, and differs from the run without final_value"""
    torch = pytest.importorskip("torch")
    from modurl_gym_amd.torch_env import TorchVecEnv
    K, LIMIT, H, GAMMA, LAM = 16, 7, 8, 0.99, 0.95
    env = TorchVecEnv(mg.PENDULUM, N, seed=2024, final_obs_steps=K, max_episode_steps=LIMIT)
    obs0 = env.reset().clone()
    el0 = (np.random.default_rng(11).permutation(N) % LIMIT).astype(np.int32)
    env.set_elapsed_steps(torch.from_numpy(el0).to(env.device))
    rng = np.random.default_rng(9)
    w1, b1, w2, b2 = (rng.normal(0, 1, s).astype(F) for s in ((H, 3), (H,), (1, H), (1,)))
    for widths, act in (((17,), "tanh"), ((17, 33), "tanh_fast")):
        crit, w = R.critic("pendulum", widths)
        tw = [torch.from_numpy(x) for x in w]
        _, obs, rew, done, trunc = env.rollout_mlp_gauss(w1, b1, w2, b2, K, 0.5, 77, len(widths))
        value, last, fv = env.value_mlp(tw, obs0, obs, done, trunc, activation=act)
        adv, ret = env.gae(rew, done, trunc, value, last, fv, GAMMA, LAM)
        env.check()
        h = {k: x.cpu().numpy() for k, x in dict(obs0=obs0, obs=obs, rew=rew, done=done, trunc=trunc, value=value, last=last, fv=fv, adv=adv, ret=ret,
                                                 fo=env.final_obs[:K]).items()}
        assert h["trunc"].sum() >= 2 * N and not h["done"].any()
        sel = R.selection(h["done"], h["trunc"])
        ev, el, ef = R.value_mlp(crit, 3, widths, {"tanh": R.TANH, "tanh_fast": R.TANH_FAST}[act], h["obs0"], h["obs"],
                                 R.poisoned_final_obs(h["fo"], sel), h["done"], h["trunc"], fill=0)
        assert same(h["value"], ev) and same(h["last"], el) and same(h["fv"].view(np.uint32), ef)
        exp = gae_ref.gae(h["rew"], h["done"], h["trunc"], ev, el, ef.view(F), GAMMA, LAM)
        assert same(h["adv"], exp[0]) and same(h["ret"], exp[1])
        assert not same(exp[0], gae_ref.gae(h["rew"], h["done"], h["trunc"], ev, el, None, GAMMA, LAM)[0])   # final_value matters here
        obs0 = obs[-1].clone()
    # an env built without final_obs_steps, or a call without `truncated`, returns no final values
    assert env.value_mlp(tw, obs0, obs, activation="tanh_fast")[2] is None
    env.close()
