"""The one policy-rollout entry of every family (Env::rollout_policy behind mgym_rollout_uniform / _linear / _mlp / _mlp_sample / _mlp_gauss / _mlp2): what
the entry points share must not leak between them.
  1. The handle's count of uniform calls (a Philox counter word of the policy stream) moves only with uniform calls that launch.
  2. Every rejection names the entry point that was called.
  3. The C ABI's own rejections keep their order and their text."""
import numpy as np
import pytest

import modurl_gym_amd as mg
from device_buffers import CallBuffers
from families import BY_KIND, CLASSIC as CLASSIC_NAMES, KIND
from words import same

pytestmark = pytest.mark.gpu

L = mg.envs.L
CLASSIC = {name: KIND[name] for name in CLASSIC_NAMES}
N, K = 8, 4
SEEDS = (11, 12)


def linear_policy(env):
    return np.random.default_rng(3).uniform(-1, 1, BY_KIND[env.kind].lin).astype(np.float32)


def mlp_weights(env, H=2):
    D, A = env.mlp_dims()
    r = np.random.default_rng(4)
    return tuple(r.uniform(-1, 1, s).astype(np.float32) for s in ((H, D), (H,), (A, H), (A,)))


def rejected(call):
    """call() must fail with ERR_BAD_ARG -> the engine's message"""
    with pytest.raises(mg.MgymError) as ei:
        call()
    assert ei.value.status == L.ERR_BAD_ARG, str(ei.value)
    return L.load().mgym_last_error().decode()


def other_sources(env):
    """one linear and one hidden-layer rollout: they advance the state, never the uniform count"""
    env.rollout_linear(linear_policy(env), K)
    env.rollout_mlp(*mlp_weights(env), K)


def uniform_twice(env):
    return [env.rollout_uniform(s, K) for s in SEEDS]


def check_counter(kind, misaligned):
    env = mg.VecEnv(kind, N, seed=7)
    env.reset()
    env.rollout_uniform_device(SEEDS[0], 0)                      # K = 0: nothing launches
    if misaligned:
        o = CallBuffers(N, env.obs_dim, np.uint32, K, mis=4)     # the reward pointer 4 bytes off its alignment
        rejected(lambda: env.rollout_uniform_device(SEEDS[0], K, *o.pointers()))
    other_sources(env)
    got = uniform_twice(env)
    env.close()

    fresh = mg.VecEnv(kind, N, seed=7)                           # the same state, and its first and second uniform call
    fresh.reset()
    other_sources(fresh)
    exp = uniform_twice(fresh)
    fresh.close()
    for c, (g, e) in enumerate(zip(got, exp)):
        for a, b, nm in zip(g, e, ("actions", "obs", "reward", "done", "truncated")):
            assert same(a, b), f"uniform call {c}: {nm}"

    plain = mg.VecEnv(kind, N, seed=7)                           # no other source at all: the drawn actions do not depend on the state
    plain.reset()
    for c, (g, e) in enumerate(zip(got, uniform_twice(plain))):
        assert same(g[0], e[0]), f"uniform call {c}: actions against a handle that made uniform calls only"
    plain.close()


@pytest.mark.parametrize("fam", list(CLASSIC) + ["lunar_lander"])
def test_uniform_call_counter_moves_only_with_calls_that_launch(fam):
    if fam == "lunar_lander":
        check_counter(mg.LUNARLANDER, misaligned=False)          # (no alignment rejection in this family)
    else:
        check_counter(CLASSIC[fam], misaligned=True)


@pytest.mark.parametrize("fam", list(CLASSIC))
def test_every_rejection_names_its_entry_point(fam):
    def entry_points(env, o):
        out = o.pointers()
        policy, H = env.pack_mlp(*mlp_weights(env))
        D, A = env.mlp_dims()
        r = np.random.default_rng(5)
        policy2, H1, H2 = env.pack_mlp2(*(r.uniform(-1, 1, s) for s in ((3, D), (3,), (5, 3), (5,), (A, 5), (A,))))
        if env.action_is_float:                                  # the family's drawing entry point and head
            draw = ("mgym_rollout_mlp_gauss", lambda: env.rollout_mlp_gauss_device(policy, H, "relu", 0.5, SEEDS[0], 0, K, *out))
        else:
            draw = ("mgym_rollout_mlp_sample", lambda: env.rollout_mlp_sample_device(policy, H, "relu", SEEDS[0], 0, K, *out))
        return (("mgym_rollout_uniform", lambda: env.rollout_uniform_device(SEEDS[0], K, *out)),
                ("mgym_rollout_linear", lambda: env.rollout_linear_device(linear_policy(env), K, *out)),
                ("mgym_rollout_mlp", lambda: env.rollout_mlp_device(policy, H, "relu", K, *out)),
                draw,
                ("mgym_rollout_mlp2", lambda: env.rollout_mlp2_device(policy2, H1, H2, "relu", "greedy", 0.0, SEEDS[0], 0, K, *out)),
                ("mgym_rollout_mlp2", lambda: env.rollout_mlp2_device(policy2, H1, H2, "relu", "gauss" if env.action_is_float else "sample", 0.5, SEEDS[0], 0, K, *out)))

    for n in (6, N):                                             # n_envs no multiple of 4; a reward pointer off its 16-byte alignment
        env = mg.VecEnv(CLASSIC[fam], n, seed=7)
        env.reset()
        before = env.get_state()
        for api, call in entry_points(env, CallBuffers(n, env.obs_dim, np.uint32, K, mis=4 if n == N else 0)):
            msg = rejected(call)
            assert msg.startswith(api + ":"), (api, msg)
            assert "multiple of 4" in msg, msg
            assert ("below 2^30" in msg) == (fam == "cartpole"), msg
        env.sync()
        assert same(env.get_state(), before)                     # nothing ran
        env.close()


def test_abi_rejections_keep_their_order_and_text():
    """The C ABI's own argument checks, called through the ctypes prototypes (the Python wrappers' checks out of the way) with two faults at once: which
    one is reported, and its full text — the name of the entry point that was called, ": ", and the literal given here.  Nothing launches; every
    handle's state stays what it was.  (The Pendulum handle with env_id_base = 2 is there for the checks that precede env_id_base in the Gaussian forms.)"""
    import ctypes as C
    lib = L.load()
    P = (C.c_float * 8192)()                                     # a policy that is not NULL (nothing reads it)
    NAN, RELU, TANH, SAMPLE, GAUSS = float("nan"), L.ACT_RELU, L.ACT_TANH, L.HEAD_SAMPLE, L.HEAD_GAUSS
    PHILOX = "(one Philox block serves 4 consecutive global env ids)"
    cp, pd = (mg.VecEnv(k, N, seed=7, auto_reset=True) for k in (mg.CARTPOLE, mg.PENDULUM))
    cp2, pd2 = (mg.VecEnv(k, N, seed=7, auto_reset=True, env_id_base=2) for k in (mg.CARTPOLE, mg.PENDULUM))
    envs = (cp, pd, cp2, pd2)
    before = []
    for env in envs:
        env.reset()
        before.append(env.get_state())

    def refused(env, name, lead, text):
        st = getattr(lib, "mgym_rollout_" + name)(env._h, *lead, None, None, None, None, None)
        assert st == L.ERR_BAD_ARG, (name, lead, st)
        assert lib.mgym_last_error().decode() == "mgym_rollout_" + name + ": " + text, (name, lead)

    # the leading arguments of each entry point with every fault it can carry at once (NULL policy, widths, activation 2, head 3, sigma) and the given K
    def every_fault(K):
        return (("uniform", cp2, (1, K)), ("linear", cp, (None, K)), ("mlp", cp, (None, 0, 2, K)), ("mlp_sample", pd, (None, 0, 2, 1, 0, K)),
                ("mlp_gauss", cp, (None, 0, 2, NAN, 1, 0, K)), ("mlp2", cp2, (None, 0, 65, 2, 3, -1.0, 1, 0, K)))

    for name, env, lead in every_fault(-1):                      # K < 0 before a NULL policy, a family refusal and env_id_base
        refused(env, name, lead, "K < 0")
    bufs = [mg.DeviceArray((1, env.obs_dim, N), np.float32) for env in envs]
    for env, buf in zip(envs, bufs):
        env.set_final_obs_out_device(buf, 1)
    for name, env, lead in every_fault(2):                       # then the final-observation channel's steps_cap
        refused(env, name, lead, "K = 2 exceeds steps_cap = 1 of mgym_set_final_obs_out")
    for env in envs:
        env.set_final_obs_out_device(None)

    refused(cp, "mlp", (None, 0, 2, 1), "policy is NULL")
    refused(cp, "mlp", (P, 0, 2, 1), "hidden must be between 1 and 64")
    refused(cp, "mlp", (P, 3, 2, 1), "activation must be MGYM_ACT_RELU, MGYM_ACT_TANH or MGYM_ACT_TANH_FAST")
    refused(cp, "linear", (None, 1), "policy is NULL")

    refused(pd, "mlp_sample", (None, 0, 2, 1, 0, 1), "Pendulum has no discrete actions to draw from (a Gaussian head is not implemented)")
    refused(cp2, "mlp_sample", (None, 0, 2, 1, 0, 1), "policy is NULL")
    refused(cp2, "mlp_sample", (P, 0, 2, 1, 0, 1), "hidden must be between 1 and 64")
    refused(cp2, "mlp_sample", (P, 3, 2, 1, 0, 1), "activation must be MGYM_ACT_RELU, MGYM_ACT_TANH or MGYM_ACT_TANH_FAST")
    refused(cp2, "mlp_sample", (P, 3, RELU, 1, 0, 1), "env_id_base must be a multiple of 4 " + PHILOX)

    refused(cp, "mlp_gauss", (None, 0, 2, NAN, 1, 0, 1), "CartPole has discrete actions: use mgym_rollout_mlp_sample")
    refused(pd, "mlp_gauss", (None, 0, 2, NAN, 1, 0, 1), "policy is NULL")
    refused(pd, "mlp_gauss", (P, 65, 2, NAN, 1, 0, 1), "hidden must be between 1 and 64")
    refused(pd, "mlp_gauss", (P, 3, 2, NAN, 1, 0, 1), "activation must be MGYM_ACT_RELU, MGYM_ACT_TANH or MGYM_ACT_TANH_FAST")
    refused(pd, "mlp_gauss", (P, 3, RELU, NAN, 1, 0, 1), "sigma must be finite and >= 0")
    refused(pd2, "mlp_gauss", (P, 3, RELU, NAN, 1, 0, 1), "sigma must be finite and >= 0")
    refused(pd2, "mlp_gauss", (P, 3, RELU, float("inf"), 1, 0, 1), "sigma must be finite and >= 0")
    refused(pd2, "mlp_gauss", (P, 3, RELU, 0.5, 1, 0, 1), "env_id_base must be a multiple of 4 " + PHILOX)

    refused(pd2, "mlp2", (None, 0, 65, TANH, 3, -1.0, 1, 0, 1), "policy is NULL")
    refused(pd2, "mlp2", (P, 0, 65, TANH, 3, -1.0, 1, 0, 1), "hidden1 must be between 1 and 64")
    refused(pd2, "mlp2", (P, 3, 65, TANH, 3, -1.0, 1, 0, 1), "hidden2 must be between 1 and 64")
    refused(pd2, "mlp2", (P, 3, 5, TANH, 3, -1.0, 1, 0, 1), "activation MGYM_ACT_TANH is not offered with two hidden layers (the exact tanh would be nearly all of the "
                                                            "launch): use MGYM_ACT_TANH_FAST or MGYM_ACT_RELU")
    refused(pd2, "mlp2", (P, 3, 5, 2, 3, -1.0, 1, 0, 1), "activation must be MGYM_ACT_RELU or MGYM_ACT_TANH_FAST")
    refused(pd2, "mlp2", (P, 3, 5, RELU, 3, -1.0, 1, 0, 1), "head must be MGYM_HEAD_GREEDY, MGYM_HEAD_SAMPLE or MGYM_HEAD_GAUSS")
    refused(pd2, "mlp2", (P, 3, 5, RELU, SAMPLE, -1.0, 1, 0, 1), "head MGYM_HEAD_SAMPLE: Pendulum has no discrete actions to draw from (use MGYM_HEAD_GAUSS)")
    refused(cp2, "mlp2", (P, 3, 5, RELU, GAUSS, -1.0, 1, 0, 1), "head MGYM_HEAD_GAUSS: CartPole has discrete actions (use MGYM_HEAD_SAMPLE)")
    refused(pd2, "mlp2", (P, 3, 5, RELU, GAUSS, -1.0, 1, 0, 1), "sigma must be finite and >= 0")
    refused(pd2, "mlp2", (P, 3, 5, RELU, GAUSS, 0.5, 1, 0, 1), "env_id_base must be a multiple of 4 for a drawing head " + PHILOX)
    refused(cp2, "mlp2", (P, 3, 5, RELU, SAMPLE, -1.0, 1, 0, 1), "env_id_base must be a multiple of 4 for a drawing head " + PHILOX)

    refused(cp2, "uniform", (1, 1), "env_id_base must be a multiple of 4 (policy bits are keyed per 4 consecutive global env ids)")

    for env, b in zip(envs, before):
        env.sync()
        assert same(env.get_state(), b)                          # nothing ran
        env.close()
