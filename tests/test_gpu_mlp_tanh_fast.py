"""MGYM_ACT_TANH_FAST through mgym_rollout_mlp, mgym_rollout_mlp_sample and mgym_rollout_mlp_gauss on every family that has them.  The reference for the
actions is the restatement of include/mgym.h (tests/tanh_fast_ref.py as the hidden activation inside the fmaf chains of tests/mlp_ref.py, then the argmax, the
categorical draw of tests/mlp_sample_ref.py or the Gaussian draw of tests/mlp_gauss_ref.py) evaluated on the observation each environment holds before the
step; the reference for everything else is a second handle stepped with the actions the call wrote.  Whole words, no tolerance.

Shapes: 260 environments are 65 lanes of four — one full wave and a single lane of the next — and 4 are one lane; K = 5 with max_episode_steps = 3 puts the
time limit and its fused resets inside the call (CartPole has its own limit of 500: states are imported near it and beyond the angle threshold)."""
import numpy as np
import pytest

import modurl_gym_amd as mg
from device_buffers import FinalBuf
from families import CLASSIC, KIND
import mlp_ref as M
import tanh_fast_ref as T
from glibc_f32 import tanhf
from mlp_ref import packed
from words import bits, same

pytestmark = pytest.mark.gpu

F = np.float32
K, LIMIT = 5, 3
ENV_SEED, POLICY_SEED, CALL, SIGMA = 17, 0xFA57C0DE77, 9, 0.4
BASE = (1 << 32) - 8   # the global ids straddle 2^32 (a multiple of 4)
IN_SCALE = {"cartpole": (1.0, 1.0, 8.0, 1.0), "mountain_car": (2.0, 40.0), "mountain_car_continuous": (2.0, 40.0), "pendulum": (1.0, 1.0, 0.3),
            "acrobot": (1.0, 1.0, 1.0, 1.0, 0.3, 0.2), "lunar_lander": (2.0, 2.0, 2.0, 2.0, 3.0, 2.0, 2.0, 2.0)}
FORM_NAME = {T.ARGMAX: "mlp", T.SAMPLE: "mlp_sample", T.GAUSS: "mlp_gauss"}
ROLLOUT_CASES = [(fam, form, H, n) for fam in CLASSIC for form in ((T.ARGMAX, T.GAUSS) if M.FAMILIES[fam][1] == 1 else (T.ARGMAX, T.SAMPLE))
                 for H, n in ((1, 260), (5, 260), (64, 260), (5, 4))]


def weights(fam, H, form):
    D, A, _ = M.FAMILIES[fam]
    rng = np.random.default_rng(7000 + 100 * list(KIND).index(fam) + 10 * form + H)
    return M.normal_weights(rng, D, A, H, IN_SCALE[fam], w2_scale=2.0)


def make(fam, n, auto_reset=True, base=BASE, **kw):
    limit = 0 if fam in ("cartpole", "lunar_lander") else LIMIT
    return mg.VecEnv(KIND[fam], n, seed=ENV_SEED, auto_reset=auto_reset, max_episode_steps=limit, env_id_base=base, **kw)


def prepare(env, fam):
    """reset; CartPole: some environments a step or two short of its 500-step limit, some beyond the angle threshold, so that endings of both kinds and
    their resets fall inside the K steps (the other families: max_episode_steps = 3)"""
    env.reset()
    if fam == "cartpole":
        blob = env.get_state().copy()
        w = blob.view(np.uint32)
        idx = np.arange(env.n)
        near = idx % 4 != 3
        w[4, near] = (496 + idx % 4)[near]                   # truncated at steps 3, 2, 1 of the call
        blob[2, idx % 8 == 7] = 0.3                          # beyond 12 degrees: done at the first step
        env.set_state(blob)


def call(env, form, w, activation="tanh_fast", K=K):
    if form == T.ARGMAX:
        return env.rollout_mlp(*w, K, activation=activation)
    if form == T.SAMPLE:
        return env.rollout_mlp_sample(*w, K, POLICY_SEED, CALL, activation=activation)
    return env.rollout_mlp_gauss(*w, K, SIGMA, POLICY_SEED, CALL, activation=activation)


def check_against_restatement_and_steps(fam, form, H, got, obs, stepper, twin=None):
    """every action word against the restatement on the observation held before the step; obs, reward and flags against mgym_step fed actions_out.
    -> the final observations [(t, finished mask, twin obs)] when a handle without auto-reset is given"""
    D, A, _ = M.FAMILIES[fam]
    pol = packed(weights(fam, H, form))
    acts, gobs, grew, gdone, gtrunc = got
    n = acts.shape[1]
    g = np.uint64(BASE) + np.arange(n, dtype=np.uint64)
    finals = []
    for t in range(acts.shape[0]):
        exp, _ = T.policy_actions(form, pol, D, A, H, obs, SIGMA, POLICY_SEED, CALL, g, t)
        bad = np.nonzero(bits(acts[t]) != exp)[0]
        assert bad.size == 0, f"step {t}: {bad.size} of {n} actions differ; env {bad[0]}: device {bits(acts[t])[bad[0]]:#x}, restatement {int(exp[bad[0]]):#x}"
        if twin is not None:
            twin.set_state(stepper.get_state())
            if fam != "cartpole":
                twin.set_elapsed_steps(stepper.elapsed_steps())
            finals.append(twin.step(acts[t])[0].copy())
        o, r, d, tr = stepper.step(acts[t])
        for x, e, nm in zip((gobs[t], grew[t], gdone[t], gtrunc[t]), (o, r, d, tr), ("obs", "reward", "done", "truncated")):
            assert same(x, e), f"step {t}: {nm}"
        obs = gobs[t]
    return finals


@pytest.mark.parametrize("fam,form,H,n", ROLLOUT_CASES, ids=[f"{fam}-{FORM_NAME[form]}-H{H}-n{n}" for fam, form, H, n in ROLLOUT_CASES])
def test_rollout_equals_the_restatement_and_a_stepping_loop(fam, form, H, n):
    w = weights(fam, H, form)
    env, stepper = make(fam, n), make(fam, n)
    prepare(env, fam), prepare(stepper, fam)
    obs = env.observation()
    assert same(obs, stepper.observation())
    got = call(env, form, w)
    assert got[0].shape == (K, n) and got[1].shape == (K, M.FAMILIES[fam][0], n)
    check_against_restatement_and_steps(fam, form, H, got, obs, stepper)
    fin = got[3].astype(bool) | got[4].astype(bool)
    assert fin.any() and not fin.all(), "endings (and their fused resets) fall inside the call, and not everywhere"
    assert same(env.get_state(), stepper.get_state()) and env.episode_count() == stepper.episode_count()
    if fam != "cartpole":
        assert np.array_equal(env.elapsed_steps(), stepper.elapsed_steps())
    env.close(), stepper.close()


@pytest.mark.parametrize("fam", CLASSIC)
def test_final_observation_channel(fam):
    """one case per family with mgym_set_final_obs_out set: everything else as with the channel unset, the finals those of a handle without auto-reset"""
    form = T.GAUSS if M.FAMILIES[fam][1] == 1 else T.SAMPLE
    H, n, D = 5, 260, M.FAMILIES[fam][0]
    w = weights(fam, H, form)
    env, stepper, twin = make(fam, n), make(fam, n), make(fam, n, auto_reset=False)
    prepare(env, fam), prepare(stepper, fam), twin.reset()
    obs = env.observation()
    fb = FinalBuf(K + 1, D, n)
    env.set_final_obs_out_device(fb.ptr, K + 1)
    got = call(env, form, w)
    finals = check_against_restatement_and_steps(fam, form, H, got, obs, stepper, twin)
    fin = got[3].astype(bool) | got[4].astype(bool)
    assert fin.sum() >= 8
    fb.check(finals, fin, fam)
    env.set_final_obs_out_device(None)
    env.close(), stepper.close(), twin.close()


# ---- LunarLander: K x (policy kernel, mgym_step) only -----------------------------------------------------------------------------------------------
LL_N, LL_K, LL_BASE = 67, 4, 8


def ll_make(monkeypatch, knob):
    env_vars = {"MGYM_LL_ROLLOUT_MIN_K": "8", "MGYM_LL_ROLLOUT_MLP": "1"} if knob else {}
    for k, v in env_vars.items():
        monkeypatch.setenv(k, v)   # read when the handle is created
    env = mg.VecEnv(mg.LUNARLANDER, LL_N, seed=ENV_SEED, enable_wind=True, auto_reset=True, env_id_base=LL_BASE)
    for k in env_vars:
        monkeypatch.delenv(k)
    return env


def launches(env):
    return int(env.info()["rollout_persistent_launches"])


@pytest.mark.parametrize("form", [T.ARGMAX, T.SAMPLE], ids=["mlp", "mlp_sample"])
def test_lunar_lander_equals_restated_policy_and_steps(monkeypatch, form):
    fam, H = "lunar_lander", 7
    w = weights(fam, H, form)
    pol = packed(w)
    env, stepper = ll_make(monkeypatch, False), ll_make(monkeypatch, False)
    obs = stepper.reset()
    assert same(env.reset(), obs)
    got = call(env, form, w, K=LL_K)
    g = np.uint64(LL_BASE) + np.arange(LL_N, dtype=np.uint64)
    seen = set()
    for t in range(LL_K):
        exp, _ = T.policy_actions(form, pol, 8, 4, H, obs, 0.0, POLICY_SEED, CALL, g, t)
        assert np.array_equal(got[0][t], exp), f"step {t}: actions"
        seen |= set(exp.tolist())
        o, r, d, tr = stepper.step(exp)
        for x, e, nm in zip((got[1][t], got[2][t], got[3][t], got[4][t]), (o, r, d, tr), ("obs", "reward", "done", "truncated")):
            assert same(x, e), f"step {t}: {nm}"
        obs = o
    assert len(seen) >= 2
    assert same(env.get_state(), stepper.get_state())
    assert launches(env) == 0
    env.close(), stepper.close()


def test_lunar_lander_stays_k_steps_under_the_persistent_knob(monkeypatch):
    """with MGYM_LL_ROLLOUT_MLP=1 and K = 16 >= MGYM_LL_ROLLOUT_MIN_K the exact tanh runs inside the persistent launch; this activation does not, and
    rollout_persistent_launches does not move — the same words as a handle without the knob"""
    fam, H, K16 = "lunar_lander", 7, 16
    w = weights(fam, H, T.ARGMAX)
    knob, plain = ll_make(monkeypatch, True), ll_make(monkeypatch, False)
    assert same(knob.reset(), plain.reset())
    state0 = knob.get_state()
    a = knob.rollout_mlp(*w, K16, activation="tanh_fast")
    assert launches(knob) == 0
    b = plain.rollout_mlp(*w, K16, activation="tanh_fast")
    assert all(same(x, y) for x, y in zip(a, b)) and launches(plain) == 0
    knob.rollout_mlp_sample(*w, K16, POLICY_SEED, CALL, activation="tanh_fast")
    assert launches(knob) == 0
    knob.set_state(state0)
    knob.rollout_mlp(*w, K16, activation="tanh")   # the knob is live on this handle: the exact tanh moves the count
    assert launches(knob) >= 1
    knob.close(), plain.close()


# ---- the discrete families: a policy whose action turns on the activation's last bit --------------------------------------------------------------
DISCRETE = ["cartpole", "mountain_car", "acrobot", "lunar_lander"]


@pytest.mark.parametrize("form", [T.ARGMAX, T.SAMPLE], ids=["mlp", "mlp_sample"])
@pytest.mark.parametrize("fam", DISCRETE)
def test_discrete_action_turns_on_the_last_bit_of_the_activation(fam, form):
    """In the rollouts above a discrete family shows its activation only through an action index, which the exact tanh would nearly always share.  Here one
    hidden unit feeds s_0 = 2^27 (h - h_fast(e)) and s_1 = 0 for a pivot environment e whose glibc tanhf lies one spacing below mg_tanhf_fast: the
    restatement gives s_0 = 0 and action 0 at e (a tie; for the draw u_e < 1/2), and with tanhf in its place s_0 <= -8 and action 1.  The device must give 0:
    a launch that ran the exact-tanh instantiation of the source would not."""
    import mlp_sample_ref as S
    D, A, _ = M.FAMILIES[fam]
    n = 260
    env = make(fam, n, enable_wind=True) if fam == "lunar_lander" else make(fam, n)
    env.reset()
    env.rollout_uniform(5, 12)   # a dozen random steps spread the states (Acrobot's reset observations are nearly alike)
    obs = env.observation()
    g = np.uint64(BASE) + np.arange(n, dtype=np.uint64)
    u = (S.words(POLICY_SEED, CALL, g, 0) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    b1 = np.array([0.9], F)
    for trial in range(16):   # the first hidden unit of a fixed sequence under which some environment separates the two activations
        w1 = np.random.default_rng(9100 + 100 * DISCRETE.index(fam) + trial).normal(0, 1, (1, D)).astype(F)
        pre = np.full(n, b1[0], F)
        for q in range(D):
            pre = T.fmaf(w1[0, q], obs[q], pre)
        h_fast, h_exact = T.tanh_fast(pre), tanhf(pre)
        cand = np.flatnonzero((h_exact < h_fast) & (h_fast >= 0.5) & (h_fast < 0.99) & (u > 0.05) & (u < 0.5))
        if cand.size:
            break
    assert cand.size, "no environment of this population separates the two activations under any of the 16 hidden units"
    e = int(cand[0])
    gain = F(2.0 ** 27)
    w2, b2 = np.zeros((A, 1), F), np.full(A, -1000.0, F)
    w2[0, 0], b2[0], b2[1] = gain, -(gain * h_fast[e]), 0.0
    w = (w1, b1, w2, b2)
    pol = packed(w)
    fast, s_fast = T.policy_actions(form, pol, D, A, 1, obs, 0.0, POLICY_SEED, CALL, g, 0)
    exact, s_exact = T.policy_actions(form, pol, D, A, 1, obs, 0.0, POLICY_SEED, CALL, g, 0, activation=tanhf)
    assert s_fast[0][e] == 0.0 and s_exact[0][e] <= -8.0 and fast[e] == 0 and exact[e] == 1   # the policy separates the activations at e
    got = call(env, form, w, K=1)
    assert int(got[0][0][e]) == 0, "the action of the exact tanh at the pivot environment"
    assert np.array_equal(got[0][0], fast)
    env.close()


# ---- the bindings and the argument checks --------------------------------------------------------------------------------------------------------
def test_torch_vecenv_accepts_tanh_fast_and_equals_vecenv():
    torch = pytest.importorskip("torch")
    fam, H, n = "pendulum", 5, 260
    te = mg.TorchVecEnv(KIND[fam], n, seed=ENV_SEED, auto_reset=True, env_id_base=BASE, max_episode_steps=LIMIT)
    ve = make(fam, n)
    te.reset(), ve.reset()
    w = weights(fam, H, T.GAUSS)
    tw = [torch.from_numpy(x) for x in w]
    for got, exp in ((te.rollout_mlp_gauss(*tw, K, SIGMA, POLICY_SEED, call=CALL, activation="tanh_fast"), call(ve, T.GAUSS, w)),
                     (te.rollout_mlp(*tw, K, activation="tanh_fast"), call(ve, T.ARGMAX, w))):
        torch.cuda.synchronize()
        for x, e, nm in zip(got, exp, ("actions", "obs", "reward", "done", "truncated")):
            x = x.cpu().numpy()
            assert same(x.astype(np.uint8) if x.dtype == np.bool_ else x, e), nm
    ve.close()
    tc = mg.TorchVecEnv(mg.CARTPOLE, n, seed=ENV_SEED, auto_reset=True)
    vc = mg.VecEnv(mg.CARTPOLE, n, seed=ENV_SEED, auto_reset=True)
    tc.reset(), vc.reset()
    w = weights("cartpole", H, T.SAMPLE)
    got = tc.rollout_mlp_sample(*[torch.from_numpy(x) for x in w], K, POLICY_SEED, call=CALL, activation="tanh_fast")
    torch.cuda.synchronize()
    exp = vc.rollout_mlp_sample(*w, K, POLICY_SEED, CALL, activation="tanh_fast")
    for x, e, nm in zip(got, exp, ("actions", "obs", "reward", "done", "truncated")):
        x = x.cpu().numpy()
        assert same(x.astype(np.uint8) if x.dtype == np.bool_ else x, e), nm
    vc.close()


def test_activation_value_3_and_the_name_are_the_same_and_2_stays_unknown():
    L = mg.envs.L
    assert L.ACT_TANH_FAST == 3
    fam, H, n = "cartpole", 5, 8
    w = weights(fam, H, T.ARGMAX)
    pol = packed(w)
    env = make(fam, n)
    env.reset()
    st = env.get_state()
    by_name = env.rollout_mlp(*w, K, activation="tanh_fast")
    env.set_state(st)
    by_value = env.rollout_mlp(*w, K, activation=3)
    assert all(same(x, y) for x, y in zip(by_name, by_value))
    for fn, args in ((env.rollout_mlp_device, (pol, H, 2, K)), (env.rollout_mlp_device, (pol, H, 4, K)), (env.rollout_mlp_sample_device, (pol, H, 2, 1, 0, K))):
        with pytest.raises(mg.MgymError) as ei:
            fn(*args)
        assert ei.value.status == L.ERR_BAD_ARG and "activation" in str(ei.value) and "MGYM_ACT_TANH_FAST" in str(ei.value)
    with pytest.raises(mg.MgymError):
        env.rollout_mlp(*w, K, activation="tanh_quick")
    env.close()


def test_entry_points_a_family_lacks_refuse_activation_3_with_their_existing_messages():
    L = mg.envs.L

    def bad(fn, what, *args):
        with pytest.raises(mg.MgymError) as ei:
            fn(*args)
        assert ei.value.status == L.ERR_BAD_ARG and what in str(ei.value), (what, str(ei.value))

    for fam, name in (("mountain_car_continuous", "MountainCarContinuous"), ("pendulum", "Pendulum")):
        env = make(fam, 8)
        env.reset()
        before = env.get_state()
        bad(env.rollout_mlp_sample_device, f"mgym_rollout_mlp_sample: {name} has no discrete actions to draw from", packed(weights(fam, 5, T.ARGMAX)), 5, "tanh_fast", 1, 0, 4)
        env.sync()
        assert same(env.get_state(), before)
        env.close()
    for fam, name in (("cartpole", "CartPole"), ("mountain_car", "MountainCar"), ("acrobot", "Acrobot"), ("lunar_lander", "LunarLander")):
        env = mg.VecEnv(KIND[fam], 8, seed=ENV_SEED)
        env.reset()
        before = env.get_state()
        bad(env.rollout_mlp_gauss_device, f"mgym_rollout_mlp_gauss: {name} has discrete actions: use mgym_rollout_mlp_sample", packed(weights(fam, 5, T.ARGMAX)), 5, 3, SIGMA, 1, 0, 4)
        env.sync()
        assert same(env.get_state(), before)
        env.close()


def test_captured_tanh_fast_rollout_replays_like_the_eager_call():
    fam, H, n = "cartpole", 64, 260
    D = 4
    cap, eag = make(fam, n), make(fam, n)
    assert same(cap.reset(), eag.reset())
    w = weights(fam, H, T.ARGMAX)
    pol = packed(w)
    bufs = [mg.DeviceArray((K, n), np.uint32), mg.DeviceArray((K, D, n), np.float32), mg.DeviceArray((K, n), np.float32),
            mg.DeviceArray((K, n), np.uint8), mg.DeviceArray((K, n), np.uint8)]
    g = cap.graph_capture(lambda: cap.rollout_mlp_device(pol, H, "tanh_fast", K, *bufs))
    pol[:] = 0.0   # the graph carries the weights it was captured with
    try:
        cap.graph_launch(g)
        cap.sync()
        exp = eag.rollout_mlp(*w, K, activation="tanh_fast")
        for b, e, nm in zip(bufs, exp, ("actions", "obs", "reward", "done", "truncated")):
            assert same(b.numpy().reshape(e.shape), e), nm
        assert same(cap.get_state(), eag.get_state())
    finally:
        cap.graph_destroy(g)
    cap.close(), eag.close()
