"""mgym_rollout_mlp_sample (include/mgym.h): softmax-sampled actions inside the CartPole / MountainCar rollout kernels and LunarLander's sampling policy
kernel, by the scheme of test_gpu_mlp_policy.py.  The reference for the actions is the host-compiled header's scores (tests/native/policy_check.cpp,
pinned to the documented arithmetic by test_mlp_policy_host.py) on the observation each env holds before the step, then the Python restatement of the
documented draw (tests/mlp_sample_ref.py); the reference for everything else is a second handle stepped with those actions.  Whole words, no tolerance."""
import numpy as np
import pytest

import modurl_gym_amd as mg
from families import KIND
import mlp_sample_ref as R
from glibc_f32 import glibc_has_fdlibm_expm1f
from mlp_policy_ref import FAMILIES, RELU, TANH, n_floats
from policy_header import GREEDY, check_lib, header_actions
from mlp_ref import normal_weights, packed
from words import same

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not glibc_has_fdlibm_expm1f(), reason="this glibc's expm1f is not the fdlibm one that mg_expm1f restates")]

ACT_NAME = {RELU: "relu", TANH: "tanh"}
IN_SCALE = {"cartpole": (2.0, 1.0, 8.0, 1.0), "mountain_car": (2.0, 40.0), "lunar_lander": (2.0, 2.0, 2.0, 2.0, 3.0, 2.0, 2.0, 2.0)}
# weight seeds, chosen on the CPU (the oracle stepped under the host-compiled header's scores and the restated draw) so that in every case below that uses
# them every action of the family occurs and at least one drawn action differs from the argmax of the same scores — asserted again on the GPU's outputs
SEEDS = {
    ("cartpole", 1, RELU): 0, ("cartpole", 1, TANH): 0, ("cartpole", 7, RELU): 0, ("cartpole", 7, TANH): 0, ("cartpole", 64, RELU): 0, ("cartpole", 64, TANH): 0,
    ("mountain_car", 1, RELU): 0, ("mountain_car", 1, TANH): 0, ("mountain_car", 7, RELU): 0, ("mountain_car", 7, TANH): 0, ("mountain_car", 64, RELU): 0, ("mountain_car", 64, TANH): 0,
    ("lunar_lander", 7, RELU): 0, ("lunar_lander", 7, TANH): 0, ("lunar_lander", 64, RELU): 0, ("lunar_lander", 64, TANH): 0,
}
POLICY_SEED = 0xC0FFEE1234
ENV_SEED = 11


def weights(fam, H, act):
    """nn.Linear-layout float32 weights (w1 [H, D], b1 [H], w2 [A, H], b2 [A]) from the family's seed"""
    D, A, _ = FAMILIES[fam]
    return normal_weights(np.random.default_rng(2000 + SEEDS[(fam, H, act)]), D, A, H, IN_SCALE[fam], b2_scale=0.3)


def make(fam, n, auto_reset, limit=0, seed=ENV_SEED, base=0):
    extra = {"enable_wind": True} if fam == "lunar_lander" else {}
    return mg.VecEnv(KIND[fam], n, seed=seed, auto_reset=auto_reset, max_episode_steps=limit, env_id_base=base, **extra)


@pytest.fixture(scope="module")
def header():
    check_lib()   # compiled once, before the first GPU call
    return header_actions


def header_scores(header, D, A, act, H, policy, obs):
    """scores [A, n] and argmax actions of the host-compiled header for an SoA observation [D, n]"""
    acts, sc = header(D, A, 1, act, GREEDY, (H,), policy, obs)
    return sc, acts


def run_case(header, fam, n, H, act, auto_reset, limit=0, base=0, K=24, calls=(0, 1)):
    D, A, _ = FAMILIES[fam]
    w = weights(fam, H, act)
    pol = packed(w)
    env, loop = make(fam, n, auto_reset, limit, base=base), make(fam, n, auto_reset, limit, base=base)
    launches = env.info().get("rollout_persistent_launches")
    obs = loop.reset()
    assert same(env.reset(), obs)
    g = base + np.arange(n, dtype=np.uint64)
    seen, off_argmax = set(), 0
    for call in calls:
        assert same(env.observation(), obs)   # the first step of a call uses the handle's current observation
        acts, gobs, grew, gdone, gtrunc = env.rollout_mlp_sample(*w, K, POLICY_SEED, call, activation=ACT_NAME[act])
        for t in range(K):
            s, amax = header_scores(header, D, A, act, H, pol, obs)
            a = R.draw(s, R.words(POLICY_SEED, call, g, t))[0]
            assert np.array_equal(acts[t], a), f"call {call} step {t}: actions"
            o, r, d, tr = loop.step(a)
            for got, exp, nm in zip((gobs[t], grew[t], gdone[t], gtrunc[t]), (o, r, d, tr), ("obs", "reward", "done", "truncated")):
                assert same(got, exp), f"call {call} step {t}: {nm}"
            seen |= set(int(v) for v in np.unique(acts[t]))      # (from the GPU's own outputs)
            off_argmax += int((acts[t] != amax).sum())
            obs = o
    assert same(env.get_state(), loop.get_state())
    if limit:
        assert np.array_equal(env.elapsed_steps(), loop.elapsed_steps())
    assert env.episode_count() == loop.episode_count()
    assert env.info().get("rollout_persistent_launches") == launches   # (LunarLander: this source never runs the persistent launch)
    env.close(); loop.close()
    assert seen == set(range(A)), f"every action occurs: {seen}"
    assert off_argmax > 0, "at least one drawn action is not the argmax: this is not mgym_rollout_mlp"


def classic_cases():
    out = []
    for fam in ("cartpole", "mountain_car"):
        for ni, n in enumerate((4, 1028)):   # one lane; one full block of the rollout kernel (256 lanes x 4 envs) plus one lane
            for ci, (H, act) in enumerate((H, act) for H in (1, 7, 64) for act in (RELU, TANH)):
                auto_reset = bool((ni + ci) % 2)
                limit = 25 if fam == "mountain_car" and (ci // 2 + ni) % 2 == 0 else 0   # MountainCar: both the time-limited and the plain instantiation
                out.append(pytest.param(fam, n, H, act, auto_reset, limit, 0, id=f"{fam}-n{n}-H{H}-{ACT_NAME[act]}-{'auto' if auto_reset else 'manual'}-limit{limit}"))
    out.append(pytest.param("cartpole", 1028, 7, RELU, True, 0, 4096, id="cartpole-n1028-H7-relu-auto-base4096"))
    out.append(pytest.param("mountain_car", 1028, 7, TANH, True, 25, 4096, id="mountain_car-n1028-H7-tanh-auto-limit25-base4096"))
    return out


@pytest.mark.parametrize("fam,n,H,act,auto_reset,limit,base", classic_cases())
def test_classic_rollout_equals_the_restated_draw_and_a_stepping_loop(header, fam, n, H, act, auto_reset, limit, base):
    run_case(header, fam, n, H, act, auto_reset, limit, base)


@pytest.mark.parametrize("n", [37, 300])   # a partial block, not a multiple of 4; two blocks of the policy kernel
@pytest.mark.parametrize("H,act", [(7, RELU), (7, TANH), (64, RELU), (64, TANH)])
def test_lunar_rollout_equals_the_restated_draw_and_a_stepping_loop(header, n, H, act):
    run_case(header, "lunar_lander", n, H, act, True, K=16)


def test_lunar_rollout_ignores_the_persistent_mlp_knob(header, monkeypatch):
    """MGYM_LL_ROLLOUT_MLP=1 at create sends mgym_rollout_mlp through the persistent launch; this entry point stays K x (policy kernel, step)"""
    monkeypatch.setenv("MGYM_LL_ROLLOUT_MLP", "1")
    run_case(header, "lunar_lander", 300, 7, TANH, True, K=16, base=8)


@pytest.mark.parametrize("fam", ["cartpole", "lunar_lander"])
def test_constant_policy_frequencies_follow_the_softmax(fam):
    """the CPU test's distribution check on the GPU's actions: they are the restatement's words, hence within its 5 standard deviations"""
    D, A, _ = FAMILIES[fam]
    env = make(fam, R.DIST_N, True)
    env.reset()
    acts = env.rollout_mlp_sample(*R.constant_policy(D, A), R.DIST_K, R.DIST_SEED, R.DIST_CALL)[0]
    env.close()
    assert np.array_equal(acts, R.dist_actions(A))
    assert R.dist_deviation(acts, A) <= 5.0


@pytest.mark.parametrize("fam", ["cartpole", "mountain_car", "lunar_lander"])
def test_call_word_sharding_and_the_uniform_count(fam):
    D, A, _ = FAMILIES[fam]
    n, K = 512, 8
    w = R.constant_policy(D, A)

    def fresh(count=n, base=0):
        e = make(fam, count, True, base=base)
        e.reset()
        return e

    one = fresh()
    a3 = one.rollout_mlp_sample(*w, K, 77, 3)[0]
    a4 = one.rollout_mlp_sample(*w, K, 77, 4)[0]
    a3_again = one.rollout_mlp_sample(*w, K, 77, 3)[0]
    assert np.array_equal(a3, a3_again) and not np.array_equal(a3, a4)          # a pure function of (seed, call, g, t) under a constant policy
    assert not np.array_equal(one.rollout_mlp_sample(*w, K, 78, 3)[0], a3)
    lo, hi = fresh(n // 2), fresh(n // 2, n // 2)                                 # two handles of n / 2 reproduce one of n
    assert np.array_equal(np.concatenate([lo.rollout_mlp_sample(*w, K, 77, 3)[0], hi.rollout_mlp_sample(*w, K, 77, 3)[0]], axis=1), a3)
    for e in (one, lo, hi):
        e.close()
    # uniform_calls is untouched: uniform rollouts draw what they draw without a sampling call in between
    plain, mixed = fresh(), fresh()
    u0 = plain.rollout_uniform(5, K)[0]
    u1 = plain.rollout_uniform(5, K)[0]
    assert np.array_equal(mixed.rollout_uniform(5, K)[0], u0)
    mixed.rollout_mlp_sample(*w, K, 77, 3)
    assert np.array_equal(mixed.rollout_uniform(5, K)[0], u1) and not np.array_equal(u0, u1)
    plain.close(); mixed.close()


def test_torch_rollout_mlp_sample_equals_vecenv():
    torch = pytest.importorskip("torch")
    fam, n = "cartpole", 1028
    te = mg.TorchVecEnv(KIND[fam], n, seed=31, auto_reset=True)
    ve = make(fam, n, True, seed=31)
    te.reset()
    ve.reset()
    w = weights(fam, 7, TANH)
    got = te.rollout_mlp_sample(*(torch.from_numpy(x) for x in w), 16, 9, call=2, activation="tanh")
    torch.cuda.synchronize()
    exp = ve.rollout_mlp_sample(*w, 16, 9, call=2, activation="tanh")
    for g, e, nm in zip(got, exp, ("actions", "obs", "reward", "done", "truncated")):
        g = g.cpu().numpy()
        g = g.view(np.uint32) if g.dtype == np.int32 else g.astype(np.uint8) if g.dtype == np.bool_ else g
        assert same(g, e), nm
    ve.close()


def test_bad_arguments_are_reported_before_any_launch():
    L = mg.envs.L
    w = weights("cartpole", 7, RELU)
    pol = packed(w)

    def bad(env, what, *args):
        with pytest.raises(mg.MgymError) as ei:
            env.rollout_mlp_sample_device(*args)
        assert ei.value.status == L.ERR_BAD_ARG and str(ei.value).split(": ", 1)[1].startswith("mgym_rollout_mlp_sample:") and what in str(ei.value), (what, str(ei.value))

    env = make("cartpole", 8, False)
    env.reset()
    before = env.get_state()
    bad(env, "policy", None, 7, "relu", 1, 0, 4)
    bad(env, "hidden", pol, 0, "relu", 1, 0, 4)
    bad(env, "hidden", pol, 65, "relu", 1, 0, 4)
    bad(env, "activation", pol, 7, 2, 1, 0, 4)
    bad(env, "K", pol, 7, "relu", 1, 0, -1)
    outs = [mg.DeviceArray((4, 8), np.uint32), mg.DeviceArray((4, 4, 8), np.float32), mg.DeviceArray((4, 8 + 4), np.float32)]
    bad(env, "aligned", pol, 7, "relu", 1, 0, 4, outs[0], outs[1], outs[2].ptr + 4)   # a misaligned reward pointer
    env.sync()
    assert same(env.get_state(), before)                   # nothing ran
    env.close()
    for kw, what in (({"n": 6}, "multiple of 4"), ({"n": 8, "base": 2}, "env_id_base")):
        e = make("cartpole", kw["n"], False, base=kw.get("base", 0))
        e.reset()
        before = e.get_state()
        bad(e, what, pol, 7, "relu", 1, 0, 4)
        e.sync()
        assert same(e.get_state(), before)
        e.close()
    ll = make("lunar_lander", 5, False, base=6)
    ll.reset()
    before = ll.get_state()
    bad(ll, "env_id_base", packed(weights("lunar_lander", 7, RELU)), 7, "relu", 1, 0, 4)
    ll.sync()
    assert same(ll.get_state(), before)
    ll.close()
    mcc = make("mountain_car_continuous", 8, False)
    mcc.reset()
    before = mcc.get_state()
    D, A = mcc.mlp_dims()
    bad(mcc, "MountainCarContinuous", np.zeros(n_floats(D, A, 7), np.float32), 7, "relu", 1, 0, 4)
    mcc.sync()
    assert same(mcc.get_state(), before)
    mcc.close()
