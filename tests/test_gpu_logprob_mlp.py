"""mgym_logprob_mlp on the device against the numpy restatement of its text (tests/logprob_ref.py), word for word (words.same: exact words).

Inputs are synthetic, from seeded generators (logprob_ref.full_case): observations uniform inside each family's bounds, action words uniform over the family's
actions or mu + 0.5 z.  logp_out is pre-filled with a poison word between two guards: every word must have been written, no guard may have been, and the inputs
are untouched.

Shapes: n = 2052 is two 1024-environment tiles of the four-per-lane kernel plus one lane; n = 1030 (not a multiple of 4) and an obs or actions buffer 4 bytes
off a 16-byte boundary take the one-environment-per-lane kernel; K = 1, 2 and 17; K = 65 540 at n = 4 walks the row stride loop beyond the grid's 65 535."""
import functools

import numpy as np
import pytest

import device_buffers
import families
import logprob_ref as R
import modurl_gym_amd as mg
import value_ref
from modurl_gym_amd import _lib
from words import same, same_words

pytestmark = pytest.mark.gpu

F = np.float32
N = 2052
KS = (1, 2, 17)
SIGMA = 0.5
Guarded = functools.partial(device_buffers.Guarded, fill=R.POISON)
bad_arg = lambda fn, *needles: device_buffers.bad_arg(fn, "mgym_logprob_mlp", *needles)


class Slabs:
    """the four device buffers of one call: the inputs of logprob_ref.full_case and a poisoned logp_out"""

    def __init__(self, family, K, n, widths, act, mis_obs=0, mis_act=0, case=None):
        self.family, self.K, self.n, self.widths, self.act = family, K, n, widths, act
        self.pol, of, ob, acts, self.exp = case or R.full_case(family, K, n, widths, act, SIGMA)
        D = R.dims(family)[0]
        self.obs_first, self.obs, self.actions = Guarded(D * n, 0, of), Guarded(K * D * n, mis_obs, ob), Guarded(K * n, mis_act, acts)
        self.logp = Guarded(K * n)

    def call(self, env, pol=None, sigma=SIGMA):
        head = "gauss" if R.head_of(self.family) == R.GAUSS else "sample"
        env.logprob_mlp_device(self.pol if pol is None else pol, self.widths[0], (*self.widths, 0)[1], self.act, head, sigma, self.K, self.obs_first, self.obs,
                               self.actions, self.logp)

    def inputs_untouched(self):
        return all(b.untouched() for b in (self.obs_first, self.obs, self.actions))

    def check(self, what, exp=None, eq=same):
        exp = self.exp if exp is None else exp
        got = self.logp.payload((self.K, self.n))
        assert (got != R.POISON).all(), f"{what}: {int((got == R.POISON).sum())} words of logp_out were not written"
        assert eq(got, exp), f"{what}: {int((got != exp).sum())} of {got.size} words of logp_out differ from the restatement"
        assert self.logp.guards_hold(), f"{what}: a guard word of logp_out was written"
        assert self.inputs_untouched(), f"{what}: an input was written"


def run(env, family, K, n, widths, act, **kw):
    b = Slabs(family, K, n, widths, act, **kw)
    b.call(env)
    env.sync()
    b.check(f"{family} K={K} n={n} {widths} act={act} {kw}")


@pytest.fixture(scope="module")
def env():
    e = mg.VecEnv(mg.CARTPOLE, N)
    yield e
    e.close()


@pytest.fixture(scope="module")
def pend():
    e = mg.VecEnv(mg.PENDULUM, N)
    yield e
    e.close()


@pytest.mark.parametrize("K", KS)
def test_four_per_lane(env, pend, K):
    run(env, "cartpole", K, N, (17,), R.TANH)
    run(env, "cartpole", K, N, (3, 5), R.TANH_FAST)
    run(pend, "pendulum", K, N, (17,), R.RELU)
    run(pend, "pendulum", K, N, (17, 33), R.RELU)


@pytest.mark.parametrize("K", [1, 17])
def test_one_per_lane(K):
    for family in ("mountain_car", "mountain_car_continuous"):
        e = mg.VecEnv(families.KIND[family], 1030)
        run(e, family, K, 1030, (17,), R.RELU)
        run(e, family, K, 1030, (3, 5), R.TANH_FAST)
        e.close()


@pytest.mark.parametrize("which", ["obs", "actions"])
def test_a_misaligned_buffer(env, pend, which):
    kw = {"mis_obs": 1} if which == "obs" else {"mis_act": 1}
    run(env, "cartpole", 2, N, (17,), R.TANH_FAST, **kw)
    run(env, "cartpole", 17, N, (17, 33), R.TANH_FAST, **kw)
    run(pend, "pendulum", 2, N, (17,), R.TANH, **kw)


@pytest.mark.parametrize("family", R.ALL)
def test_every_kind(family):
    """the six (D, A) at K = 2, every accepted (depth, activation): n = 1028 (four per lane) and n = 1030 (one per lane) — every instantiation of both kernels.
    The LunarLander handle was never reset and still is not afterwards"""
    for n in (1028, 1030):
        e = mg.VecEnv(families.KIND[family], n)
        for widths in ((17,), (3, 5)):
            for act in R.ACTS[len(widths)]:
                run(e, family, 2, n, widths, act)
        if family == "lunar_lander":
            assert e.episode_count() == 0
            with pytest.raises(mg.NotResetError):
                e.step(np.zeros(n, np.uint32))
        e.close()


@pytest.mark.parametrize("widths", R.WIDTHS, ids=str)
def test_widths(widths):
    """both depths at every width class, every accepted activation, on Acrobot (A = 3)"""
    e = mg.VecEnv(mg.ACROBOT, 1028)
    for act in R.ACTS[len(widths)]:
        run(e, "acrobot", 2, 1028, widths, act)
    e.close()


def test_more_rows_than_the_grid_holds():
    """K = 65 540 at n = 4 on MountainCar with H = 3: rows 65 535 .. 65 539 come from the stride loop; then one per lane (n = 5) with the same K"""
    for n in (4, 5):
        e = mg.VecEnv(mg.MOUNTAINCAR, n)
        run(e, "mountain_car", 65540, n, (3,), R.RELU)
        e.close()


def test_hand_built_scores_and_bad_action_words(env):
    """constant scores 18 apart, equal, with a NaN; action words >= A give the NaN word and no error, also for the handle's later calls"""
    K, n = 1, N
    c = R.case("cartpole", K, n)
    acts = (np.arange(n) % 4).astype(np.uint32).reshape(K, n)
    acts[0, 7] = 0xFFFFFFFF
    for widths in ((3,), (3, 5)):
        for b in ((0.0, -18.0), (-17.0, 0.0), (1.5, 1.5), (np.nan, 0.0), (0.0, np.inf)):
            pol = R.packed(R.constant_actor("cartpole", widths, np.array(b, F)))
            exp = R.logprob_mlp(pol, 4, 2, widths, R.TANH_FAST, c["obs_first"], c["obs"], acts)
            s = Slabs("cartpole", K, n, widths, R.TANH_FAST, case=(pol, c["obs_first"], c["obs"], acts, exp))
            s.call(env)
            env.sync()
            s.check(f"scores {b} {widths}")
            assert ((exp == R.NAN_WORD) | (acts < 2)).all() and (exp == R.NAN_WORD).sum() >= n // 2
    env.sync()   # a function of buffers: no sticky invalid-action status is raised


@pytest.mark.parametrize("sigma", (R.SIGMA_MIN, R.SIGMA_MAX), ids=("2^-126", "FLT_MAX"))
def test_the_ends_of_sigma(pend, sigma):
    pol, of, ob, acts, _ = R.full_case("pendulum", 2, N, (17,), R.TANH, SIGMA)
    mu = R.row_scores(pol, 3, 1, (17,), R.TANH, R.acted_rows(of, ob))[0]
    a = np.where(np.arange(N) % 2 == 0, mu, acts).astype(F)   # a == mu gives k exactly; the others overflow q under the small sigma
    exp = R.logprob_mlp(pol, 3, 1, (17,), R.TANH, of, ob, a, sigma)
    s = Slabs("pendulum", 2, N, (17,), R.TANH, case=(pol, of, ob, a, exp))
    s.call(pend, sigma=sigma)
    pend.sync()
    s.check(f"sigma = {sigma}")
    assert (exp[:, ::2].view(F) == R.gauss_k(sigma)).all()


def test_two_calls_back_to_back_see_their_own_weights(env):
    """two two-layer calls (the handle's one pack) and two one-layer calls with different weights, nothing synchronised in between"""
    K = 2
    for widths in ((17, 33), (17,)):
        a, b = Slabs("cartpole", K, N, widths, R.TANH_FAST), Slabs("cartpole", K, N, widths, R.TANH_FAST)
        other = R.actor("cartpole", widths, seed=1)[0]
        exp_b = R.logprob_mlp(other, 4, 2, widths, R.TANH_FAST, *R.full_case("cartpole", K, N, widths, R.TANH_FAST, SIGMA)[1:4])
        a.call(env)
        b.call(env, pol=other)
        env.sync()
        a.check(f"first call {widths}")
        b.check(f"second call {widths}", exp=exp_b)
        assert not same(a.exp, exp_b)


def _collector(seed):
    e = mg.VecEnv(mg.CARTPOLE, N, seed=seed, auto_reset=True)
    first = Guarded(4 * N, 0, e.reset())
    return e, first


def _three_calls(e, first, bufs, value, last, logp, K):
    """an actor's sampled two-layer rollout, a two-layer critic over its observations, the actor's log-probabilities of its actions"""
    actor, critic = R.actor("cartpole", (9, 12))[0], value_ref.critic("cartpole", (17, 33))[0]
    act, obs = bufs.pointers()[:2]
    e.rollout_mlp2_device(actor, 9, 12, "tanh_fast", "sample", 0.0, 77, 3, K, *bufs.pointers())
    e.value_mlp_device(critic, 17, 33, "tanh_fast", K, first, obs, None, None, None, value, last, None)
    e.logprob_mlp_device(actor, 9, 12, "tanh_fast", "sample", 0.0, K, first, obs, act, logp)


def test_graph_replay_equals_the_eager_calls():
    """one graph holding a mgym_rollout_mlp2 (sample head), a two-layer mgym_value_mlp and a two-layer mgym_logprob_mlp — three packs of one handle: capture
    launches nothing, and the replay gives the words of the same three calls made eagerly on a handle of the same seed, which are the restatement's"""
    K = 4
    out = []
    for captured in (True, False):
        e, first = _collector(5)
        bufs = device_buffers.CallBuffers(N, 4, np.uint32, K)
        value, last, logp = Guarded(K * N), Guarded(N), Guarded(K * N)
        calls = lambda: _three_calls(e, first, bufs, value, last, logp, K)
        if captured:
            state = e.get_state()
            g = e.graph_capture(calls)
            try:
                e.sync()
                assert value.untouched() and logp.untouched() and same(e.get_state(), state)   # capture launches nothing
                e.graph_launch(g)
                e.sync()
            finally:
                e.graph_destroy(g)
        else:
            calls()
            e.sync()
        assert value.guards_hold() and last.guards_hold() and logp.guards_hold() and first.untouched()
        out.append(dict(bufs.host(), first=first.payload((4, N), F), value=value.payload((K, N)), last=last.payload((N,)), logp=logp.payload((K, N))))
        e.close()
    replay, eager = out
    assert all(same(replay[k], eager[k]) for k in eager), [k for k in eager if not same(replay[k], eager[k])]
    actor = R.actor("cartpole", (9, 12))[0]
    assert same(eager["logp"], R.logprob_mlp(actor, 4, 2, (9, 12), R.TANH_FAST, eager["first"], eager["obs"], eager["act"]))
    exp_v = value_ref.value_mlp(value_ref.critic("cartpole", (17, 33))[0], 4, (17, 33), R.TANH_FAST, eager["first"], eager["obs"])
    assert same(eager["value"].view(F), exp_v[0]) and same(eager["last"].view(F), exp_v[1])
    assert len(np.unique(eager["act"])) == 2 and np.isfinite(eager["logp"].view(F)).all()


def test_no_environments():
    e = mg.VecEnv(mg.CARTPOLE, 0)
    x, pol = mg.DeviceArray(32, F), R.actor("cartpole", (17,))[0]
    e.logprob_mlp_device(pol, 17, 0, "relu", "sample", 0.0, 3, x, x.ptr + 16, x.ptr + 32, x.ptr + 48)   # MGYM_OK without a launch
    with pytest.raises(mg.MgymError):
        e.logprob_mlp_device(pol, 17, 0, "relu", "sample", 0.0, 0, x, x.ptr + 16, x.ptr + 32, x.ptr + 48)   # ... after the argument checks
    e.close()


def _raw_call(env, good, repl):
    IPOL, IH1, IK, IOF = 0, 1, 6, 7
    args = list(good)
    for k, v in repl.items():
        args[k] = v
    p = args[IPOL]
    fp = None if p is None else np.ascontiguousarray(p, F).ctypes.data_as(_lib.C.POINTER(_lib.C.c_float))
    ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.data_ptr())
    return lambda: mg.envs._check(env._lib.mgym_logprob_mlp(env._h, fp, *args[IH1: IK + 1], *(ptr(x) for x in args[IOF:])))


def test_errors(env, pend):
    K = 2
    IPOL, IH1, IH2, IACT, IHEAD, ISIG, IK, IOF, IOBS, IA, IOUT = range(11)
    b = Slabs("cartpole", K, N, (17,), R.RELU)
    pol2 = R.actor("cartpole", (17, 33))[0]
    good = [b.pol, 17, 0, _lib.ACT_RELU, _lib.HEAD_SAMPLE, float("nan"), K, b.obs_first, b.obs, b.actions, b.logp]   # (sigma is ignored under the sample head)
    rows = [({IK: 0}, "K"), ({IK: -1}, "K"), ({IPOL: None}, "policy"), ({IOF: None}, "obs_first"), ({IOBS: None}, "obs"), ({IA: None}, "actions"),
            ({IOUT: None}, "logp_out"), ({IH1: 0}, "hidden1"), ({IH1: 65}, "hidden1"), ({IH2: -1}, "hidden2"), ({IH2: 65}, "hidden2"),
            ({IACT: 2}, "activation"), ({IACT: 4}, "activation"), ({IACT: -1}, "activation"),
            ({IPOL: pol2, IH2: 33, IACT: _lib.ACT_TANH}, "activation", "MGYM_ACT_TANH"),
            ({IHEAD: _lib.HEAD_GREEDY}, "head", "MGYM_HEAD_GREEDY", "density"), ({IHEAD: 3}, "head"), ({IHEAD: -1}, "head"),
            ({IHEAD: _lib.HEAD_GAUSS, ISIG: 0.5}, "head", "MGYM_HEAD_GAUSS", "CartPole"),
            ({IOF: b.obs_first.ptr + 2}, "obs_first", "4-byte aligned"), ({IOBS: b.obs.ptr + 1}, "obs", "4-byte aligned"),
            ({IA: b.actions.ptr + 2}, "actions", "4-byte aligned"), ({IOUT: b.logp.ptr + 3}, "logp_out", "4-byte aligned"),
            ({IOUT: b.obs_first.ptr}, "logp_out", "obs_first"), ({IOUT: b.obs.ptr}, "logp_out", "obs"), ({IOUT: b.actions.ptr}, "logp_out", "actions"),
            # two faults: the earlier group's is the one reported — K, the NULLs, widths and activation, head and sigma, alignment, aliasing
            ({IK: 0, IPOL: None}, "K must be"), ({IOUT: None, IH1: 0}, "logp_out is NULL"), ({IH1: 0, IHEAD: 3}, "hidden1 must be"),
            ({IHEAD: 3, IOBS: b.obs.ptr + 1}, "head must be"), ({IOBS: b.obs.ptr + 1, IOUT: b.actions.ptr}, "obs must be 4-byte aligned")]
    state = env.get_state()
    for repl, *needles in rows:
        bad_arg(_raw_call(env, good, repl), *needles)
    env.sync()
    assert b.inputs_untouched() and b.logp.untouched() and same(env.get_state(), state)
    _raw_call(env, good, {})()
    env.sync()
    b.check("after the refused calls")
    # the continuous side: the sample head, and every sigma that has no density
    p = Slabs("pendulum", K, N, (17,), R.RELU)
    goodp = [p.pol, 17, 0, _lib.ACT_RELU, _lib.HEAD_GAUSS, SIGMA, K, p.obs_first, p.obs, p.actions, p.logp]
    bad_arg(_raw_call(pend, goodp, {IHEAD: _lib.HEAD_SAMPLE}), "head", "MGYM_HEAD_SAMPLE", "Pendulum")
    bad_arg(_raw_call(pend, goodp, {IHEAD: _lib.HEAD_GREEDY}), "head", "MGYM_HEAD_GREEDY")
    for sg in (0.0, -0.0, 1e-45, float(np.nextafter(F(R.SIGMA_MIN), F(0))), -1.0, float("nan"), float("inf"), float("-inf")):
        bad_arg(_raw_call(pend, goodp, {ISIG: sg}), "sigma")
    pend.sync()
    assert p.logp.untouched()
    _raw_call(pend, goodp, {})()
    pend.sync()
    p.check("pendulum after the refused calls")


def test_host_array_form(env):
    K, widths = 2, (17, 33)
    pol, of, ob, acts, exp = R.full_case("cartpole", K, N, widths, R.RELU, SIGMA)
    w = R.actor("cartpole", widths)[1]
    assert same(env.logprob_mlp(w, of, ob, acts, "relu"), exp.view(F))
    with pytest.raises(mg.PolicyShapeError):
        env.logprob_mlp(w[:5], of, ob, acts)


def test_cartpole_sampled_rollout_end_to_end():
    """rollout_mlp_sample, then logprob_mlp over its own obs and actions_out: the restatement's words, under auto-reset with episodes ending inside the call"""
    K, H = 64, 17
    e = mg.VecEnv(mg.CARTPOLE, N, seed=11, auto_reset=True)
    obs0 = e.reset().copy()
    w = R.actor("cartpole", (H,))[1]
    acts, obs, _, done, trunc = e.rollout_mlp_sample(*w, K, 99, 1, "tanh_fast")
    assert (done | trunc).any()
    got = e.logprob_mlp(w, obs0, obs, acts, "tanh_fast")
    exp = R.logprob_mlp(R.packed(w), 4, 2, (H,), R.TANH_FAST, obs0, obs, acts)
    assert same(got, exp.view(F)) and np.isfinite(got).all() and (got <= 0).all()
    assert abs(float(np.exp(got.astype(np.float64)).mean()) - 0.5) < 0.4   # probabilities of a two-action policy, not all near 0
    e.close()


def test_pendulum_gauss_rollout_end_to_end():
    """rollout_mlp_gauss, then logprob_mlp: the unclamped action word is the one used — some actions lie outside Pendulum's [-2, 2], and z is what the draw made"""
    K, H, sigma = 16, 17, 1.5
    e = mg.VecEnv(mg.PENDULUM, N, seed=11, auto_reset=True)
    obs0 = e.reset().copy()
    w = R.actor("pendulum", (H,))[1]
    acts, obs, *_ = e.rollout_mlp_gauss(*w, K, sigma, 99, 1, "tanh")
    assert (np.abs(acts) > 2.0).any()
    got = e.logprob_mlp(w, obs0, obs, acts, "tanh", sigma=sigma)
    exp = R.logprob_mlp(R.packed(w), 3, 1, (H,), R.TANH, obs0, obs, acts, sigma)
    assert same(got, exp.view(F)) and np.isfinite(got).all()
    clamped = R.logprob_mlp(R.packed(w), 3, 1, (H,), R.TANH, obs0, obs, np.clip(acts, -2.0, 2.0), sigma)
    assert not same(got, clamped.view(F))
    e.close()


def test_torch_against_float64():
    """TorchVecEnv.logprob_mlp after its own rollouts, against torch's log_softmax + gather and Normal.log_prob in float64 from the same weights: within
    logprob_ref.NET64_BOUND (test_logprob_host.py: 4 x the restatement's measured distance from the float64 network)"""
    torch = pytest.importorskip("torch")
    from modurl_gym_amd.torch_env import TorchVecEnv
    K = 16
    for family, kind, widths, act in (("cartpole", mg.CARTPOLE, (64, 64), "tanh_fast"), ("pendulum", mg.PENDULUM, (64,), "relu")):
        env = TorchVecEnv(kind, N, seed=2024)
        obs0 = env.reset().clone()
        w = R.actor(family, widths)[1]
        tw = [torch.from_numpy(x) for x in w]
        if family == "cartpole":
            acts, obs, *_ = env.rollout_mlp2(*tw, K, activation=act, head="sample", seed=5, call=1)
            logp = env.logprob_mlp(tw, obs0, obs, acts, activation=act)
        else:
            acts, obs, *_ = env.rollout_mlp_gauss(*tw, K, SIGMA, 5, 1, activation=act)
            logp = env.logprob_mlp(tw, obs0, obs, acts, activation=act, sigma=SIGMA)
        env.check()
        assert logp.shape == (K, N) and logp.dtype == torch.float32 and logp.device == obs.device
        f = torch.relu if act == "relu" else torch.tanh
        x = torch.cat([obs0[None], obs[:-1]]).double().transpose(1, 2)   # [K, n, D]
        ws = [t.double().to(x.device) for t in tw]
        for k in range(0, len(ws) - 2, 2):
            x = f(x @ ws[k].T + ws[k + 1])
        s = x @ ws[-2].T + ws[-1]   # [K, n, A]
        if family == "cartpole":
            ref = torch.log_softmax(s, -1).gather(-1, acts.long()[..., None])[..., 0]
            head = R.SAMPLE
        else:
            ref = torch.distributions.Normal(s[..., 0], SIGMA).log_prob(acts.double())
            head = R.GAUSS
        err = float((logp.double() - ref).abs().max())
        print(f"{family}: largest |logp - torch float64| = {err:.3g}, bound {R.NET64_BOUND[head]:.3g}")
        assert err <= R.NET64_BOUND[head]
        # and word for word the restatement
        h = [t.cpu().numpy() for t in (obs0, obs, acts, logp)]
        exp = R.logprob_mlp(R.packed(w), *R.dims(family), widths, {"relu": R.RELU, "tanh_fast": R.TANH_FAST}[act], h[0], h[1], h[2], SIGMA)
        assert same_words(h[3], exp.view(F))
        env.close()
