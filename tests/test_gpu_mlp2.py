"""mgym_rollout_mlp2 (include/mgym.h): the two-hidden-layer policy inside the classic families' rollout kernels and LunarLander's policy kernel.  The reference
for the actions is modurl_gym_amd/csrc/mlp2_policy.h itself, compiled for the host (tests/native/policy_check.cpp; tests/test_mlp2_host.py pins that build to the
documented arithmetic), applied to the observation each env holds before the step; the reference for everything else is a second handle stepped with those
actions.  Every comparison is of whole words: no tolerance anywhere."""
import numpy as np
import pytest

import modurl_gym_amd as mg
from device_buffers import FinalBuf, twin_steps
from families import KIND
import mlp2_ref as R
import mlp_ref as M
import policy_header as P
from words import bits, same

pytestmark = pytest.mark.gpu

F = np.float32
ACT_NAME = {R.RELU: "relu", R.TANH_FAST: "tanh_fast"}
HEAD_NAME = {R.GREEDY: "greedy", R.SAMPLE: "sample", R.GAUSS: "gauss"}
# what a unit of each observation component is worth to the first layer, sized to the reset observations (CartPole's are within 0.05 of 0, MountainCar's position
# within 0.1 of -0.5, Acrobot's angles within 0.1 of 0)
IN_SCALE = {"cartpole": (20, 20, 20, 20), "mountain_car": (30, 40), "mountain_car_continuous": (30, 40), "pendulum": (1, 1, 1), "acrobot": (1, 10, 1, 10, 10, 10),
            "lunar_lander": (2, 2, 2, 2, 3, 2, 2, 2)}
# where the reset observations sit: the first layer's bias is drawn around it (b1 - W1 c), so that units change sign within the reset observations.  MountainCar's
# are one coordinate in [-0.6, -0.4]: with b1 around 0 every unit keeps one sign over that interval and the scores are nearly linear in the position.
CENTER = {"mountain_car": (-0.5, 0.0), "mountain_car_continuous": (-0.5, 0.0), "lunar_lander": (0.0, 1.41, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)}
# weight seeds, chosen on the CPU: the smallest seed under which, on the family's reset observations (the oracle's under ENV_SEED for CartPole, MountainCar and
# LunarLander, which the engine equals word for word; draws as the reset makes them for Pendulum and Acrobot), units of both layers lie on both sides of zero, the
# host-compiled header's greedy head takes every action (both signs of the force) and every action's softmax probability is at least 0.03 on average — facts the main
# run asserts again on the GPU's outputs, for every family, head and shape.
SEEDS = {("cartpole", 64, 64, R.RELU): 0, ("cartpole", 64, 64, R.TANH_FAST): 0, ("cartpole", 3, 5, R.RELU): 0, ("cartpole", 1, 1, R.RELU): 6,
         ("mountain_car", 64, 64, R.RELU): 0, ("mountain_car", 64, 64, R.TANH_FAST): 0, ("mountain_car", 3, 5, R.RELU): 9, ("mountain_car", 1, 1, R.RELU): 14,
         ("mountain_car_continuous", 64, 64, R.RELU): 1, ("mountain_car_continuous", 64, 64, R.TANH_FAST): 1, ("mountain_car_continuous", 3, 5, R.RELU): 2,
         ("mountain_car_continuous", 1, 1, R.RELU): 1,
         ("pendulum", 64, 64, R.RELU): 0, ("pendulum", 64, 64, R.TANH_FAST): 0, ("pendulum", 3, 5, R.RELU): 2, ("pendulum", 1, 1, R.RELU): 2,
         ("acrobot", 64, 64, R.RELU): 7, ("acrobot", 64, 64, R.TANH_FAST): 2, ("acrobot", 3, 5, R.RELU): 18, ("acrobot", 1, 1, R.RELU): 651,
         ("lunar_lander", 64, 64, R.RELU): 2, ("lunar_lander", 64, 64, R.TANH_FAST): 0, ("lunar_lander", 3, 5, R.RELU): 23, ("lunar_lander", 1, 1, R.RELU): 258}
SHAPE_ACT = (((64, 64), R.RELU), ((64, 64), R.TANH_FAST), ((3, 5), R.RELU), ((1, 1), R.RELU))
K, CALLS, LIMIT = 6, 2, 4
ENV_SEED, POLICY_SEED, SIGMA = 11, 0x1234567811, 0.5


def heads(fam):
    return (R.GREEDY, R.GAUSS) if R.FAMILIES[fam][2] else (R.GREEDY, R.SAMPLE)


def weights(fam, H1, H2, act, seed=None):
    D, A, _ = R.FAMILIES[fam]
    seed = SEEDS[(fam, H1, H2, act)] if seed is None else seed
    w = list(R.normal_weights(np.random.default_rng(1000 + seed), D, A, H1, H2, IN_SCALE[fam], w3_scale=3.0, b3_scale=0.3))
    if fam in CENTER:
        w[1] = (w[1] - w[0] @ np.array(CENTER[fam], F)).astype(F)
    return tuple(w)


def make(fam, n, auto_reset=True, limit=0, seed=ENV_SEED, **kw):
    extra = {"enable_wind": True} if fam == "lunar_lander" else {}
    return mg.VecEnv(KIND[fam], n, seed=seed, auto_reset=auto_reset, max_episode_steps=limit, **extra, **kw)


def call(env, w, k, act, head, c=0):
    return env.rollout_mlp2(*w, k, activation=ACT_NAME[act], head=HEAD_NAME[head], sigma=SIGMA, seed=POLICY_SEED, call=c)


def header(fam, w, H1, H2, act, head, obs, c, t):
    D, A, _ = R.FAMILIES[fam]
    return P.header_actions(D, A, 2, act, head, (H1, H2), R.packed(w), obs, SIGMA, POLICY_SEED, c, 0, t)[0]


def forward64(w, obs, act):
    f = (lambda x: np.maximum(x, 0)) if act == R.RELU else np.tanh
    pre1 = w[0].astype(np.float64) @ obs.astype(np.float64) + w[1].astype(np.float64)[:, None]
    return pre1, w[2].astype(np.float64) @ f(pre1) + w[3].astype(np.float64)[:, None]


def lunar_header(fam, w, H1, H2, act, head, obs, c, t):
    """LunarLander takes any n: the header's four-per-lane form wants a multiple of 4, so the observation is padded with copies of its last column"""
    n = obs.shape[1]
    pad = (-n) % 4
    o = np.concatenate([obs, np.repeat(obs[:, -1:], pad, axis=1)], axis=1) if pad else obs
    return header(fam, w, H1, H2, act, head, o, c, t)[:n]


def run_case(fam, n, H1, H2, act, head):
    D, A, cont = R.FAMILIES[fam]
    w = weights(fam, H1, H2, act)
    limit = 0 if fam == "cartpole" else LIMIT
    env, loop = make(fam, n, True, limit), make(fam, n, True, limit)
    obs = loop.reset()
    assert same(env.reset(), obs)
    seen = dict(actions=set(), pos1=0, neg1=0, pos2=0, neg2=0, fpos=0, fneg=0, trunc=0)
    hdr = lunar_header if fam == "lunar_lander" else header
    for c in range(CALLS):
        assert same(env.observation(), obs)   # the first step of a call uses the handle's current observation
        acts, gobs, grew, gdone, gtrunc = call(env, w, K, act, head, c)
        for t in range(K):
            a = hdr(fam, w, H1, H2, act, head, obs, c, t)
            assert np.array_equal(bits(acts[t]), a), f"call {c} step {t}: actions"
            pre1, pre2 = forward64(w, obs, act)
            seen["pos1"] += int((pre1 > 1e-3).sum()); seen["neg1"] += int((pre1 < -1e-3).sum())
            seen["pos2"] += int((pre2 > 1e-3).sum()); seen["neg2"] += int((pre2 < -1e-3).sum())
            if cont:
                seen["fpos"] += int((a.view(F) > 0).sum()); seen["fneg"] += int((a.view(F) < 0).sum())
            else:
                seen["actions"] |= set(int(v) for v in np.unique(a))
            o, r, d, tr = loop.step(a.view(F) if cont else a)
            for g, e, nm in zip((gobs[t], grew[t], gdone[t], gtrunc[t]), (o, r, d, tr), ("obs", "reward", "done", "truncated")):
                assert same(g, e), f"call {c} step {t}: {nm}"
            seen["trunc"] += int(tr.sum())
            obs = o
    assert same(env.get_state(), loop.get_state())
    if limit:
        assert np.array_equal(env.elapsed_steps(), loop.elapsed_steps())
    assert env.episode_count() == loop.episode_count()
    env.close(); loop.close()
    return seen


def main_cases():
    out = []
    for fam in R.FAMILIES:
        for head in heads(fam):
            for (H1, H2), act in SHAPE_ACT:
                for n in (1028, 4) + ((1027,) if fam == "lunar_lander" else ()):   # four waves and one more lane of the 4-per-lane kernels; one lane
                    out.append(pytest.param(fam, n, H1, H2, act, head, id=f"{fam}-{HEAD_NAME[head]}-{H1}x{H2}-{ACT_NAME[act]}-n{n}"))
    return out


@pytest.mark.parametrize("fam,n,H1,H2,act,head", main_cases())
def test_rollout_equals_the_header_and_a_stepping_loop(fam, n, H1, H2, act, head):
    seen = run_case(fam, n, H1, H2, act, head)
    print(fam, n, H1, H2, act, head, seen)
    if n < 1027:
        return
    D, A, cont = R.FAMILIES[fam]
    if fam != "cartpole":
        assert seen["trunc"] >= n * (K * CALLS // LIMIT - 1), "the time limit truncates, and resets, inside the launch"
    assert min(seen["pos1"], seen["neg1"], seen["pos2"], seen["neg2"]) > 0, "hidden units of both layers take both signs"
    assert (seen["fpos"] > 0 and seen["fneg"] > 0) if cont else seen["actions"] == set(range(A)), seen


@pytest.mark.parametrize("fam", ("cartpole", "pendulum"))
def test_identity_middle_layer_equals_the_one_layer_entry_points(fam):
    """ReLU, W2 = I, b2 = +0: every output word of rollout_mlp2 is rollout_mlp's, and with the same (seed, call) rollout_mlp_sample's / rollout_mlp_gauss's"""
    D, A, cont = R.FAMILIES[fam]
    n, H, k = 1028, 7, 8
    one = M.normal_weights(np.random.default_rng(77), D, A, H, IN_SCALE[fam], w2_scale=3.0)
    two = R.identity_middle(one, H)
    for head in heads(fam):
        a, b = make(fam, n, True, 0 if fam == "cartpole" else LIMIT), make(fam, n, True, 0 if fam == "cartpole" else LIMIT)
        assert same(a.reset(), b.reset())
        got = call(a, two, k, R.RELU, head, 3)
        if head == R.GREEDY:
            exp = b.rollout_mlp(*one, k)
        elif head == R.SAMPLE:
            exp = b.rollout_mlp_sample(*one, k, POLICY_SEED, 3)
        else:
            exp = b.rollout_mlp_gauss(*one, k, SIGMA, POLICY_SEED, 3)
        for g, e, nm in zip(got, exp, ("actions", "obs", "reward", "done", "truncated")):
            assert same(g, e), f"{HEAD_NAME[head]}: {nm}"
        assert same(a.get_state(), b.get_state())
        a.close(); b.close()


@pytest.mark.parametrize("act", (R.RELU, R.TANH_FAST))
@pytest.mark.parametrize("fam", ("mountain_car_continuous", "pendulum"))
def test_signed_zero_reaches_actions_out(fam, act):
    D, A, _ = R.FAMILIES[fam]
    env = make(fam, 1028, True, LIMIT)
    env.reset()
    acts = call(env, R.signed_zero_policy(D, act), 3, act, R.GREEDY)[0]
    assert np.all(bits(acts) == 0x80000000), np.unique(bits(acts))
    env.close()


def test_back_to_back_calls_each_use_their_own_weights():
    """two eager calls with different weights on one stream, nothing between them: the second call's pack is stored behind the first call's launch"""
    fam, n, k = "cartpole", 1028, 5
    D, A, _ = R.FAMILIES[fam]
    env, loop = make(fam, n), make(fam, n)
    obs = loop.reset()
    assert same(env.reset(), obs)
    ws = [weights(fam, 64, 64, R.RELU, seed=0), weights(fam, 3, 5, R.RELU, seed=5)]
    outs = [[mg.DeviceArray((k, n), np.uint32), mg.DeviceArray((k, D, n), F), mg.DeviceArray((k, n), F), mg.DeviceArray((k, n), np.uint8), mg.DeviceArray((k, n), np.uint8)] for _ in ws]
    for w, o in zip(ws, outs):
        pol, H1, H2 = env.pack_mlp2(*w)
        env.rollout_mlp2_device(pol, H1, H2, "relu", "greedy", 0.0, 0, 0, k, *o)
    env.sync()
    for i, (w, o) in enumerate(zip(ws, outs)):
        acts = o[0].numpy().reshape(k, n)
        for t in range(k):
            a = header(fam, w, w[0].shape[0], w[2].shape[0], R.RELU, R.GREEDY, obs, 0, t)
            assert np.array_equal(acts[t], a), f"call {i} step {t}"
            obs = loop.step(a)[0]
    assert same(env.get_state(), loop.get_state())
    env.close(); loop.close()


def test_captured_call_freezes_the_weights():
    fam, n, k = "cartpole", 1028, 6
    D, A, _ = R.FAMILIES[fam]
    cap, loop = make(fam, n, seed=29), make(fam, n, seed=29)
    obs = loop.reset()
    assert same(cap.reset(), obs)
    w = weights(fam, 64, 64, R.TANH_FAST)
    pol, H1, H2 = cap.pack_mlp2(*w)
    bufs = [mg.DeviceArray((k, n), np.uint32), mg.DeviceArray((k, D, n), F), mg.DeviceArray((k, n), F), mg.DeviceArray((k, n), np.uint8), mg.DeviceArray((k, n), np.uint8)]
    g = cap.graph_capture(lambda: cap.rollout_mlp2_device(pol, H1, H2, "tanh_fast", "sample", 0.0, POLICY_SEED, 2, k, *bufs))
    pol[:] = 0.0   # the caller's array may change after the capture: the graph carries the weights it was captured with
    try:
        for rep in range(2):
            cap.graph_launch(g)
            cap.sync()
            acts = bufs[0].numpy().reshape(k, n)
            for t in range(k):   # the captured weights, seed and call word on the state the replay finds
                a = header(fam, w, 64, 64, R.TANH_FAST, R.SAMPLE, obs, 2, t)
                assert np.array_equal(acts[t], a), f"replay {rep} step {t}"
                obs = loop.step(a)[0]
            assert same(cap.get_state(), loop.get_state())
    finally:
        cap.graph_destroy(g)
    cap.close(); loop.close()


@pytest.mark.parametrize("fam,head", (("mountain_car", R.SAMPLE), ("pendulum", R.GAUSS)))
def test_final_observations_under_rollout_mlp2(fam, head):
    """the channel of mgym_set_final_obs_out: where a step finished, the words a twin handle without auto-reset returns as obs from the same state and action"""
    D, A, cont = R.FAMILIES[fam]
    n, k = 1028, 6
    w = weights(fam, 3, 5, R.RELU)
    env, ref, twin = make(fam, n, True, LIMIT), make(fam, n, True, LIMIT), make(fam, n, False, LIMIT)
    assert same(env.reset(), ref.reset())
    twin.reset()
    fin = FinalBuf(k, D, n)
    env.set_final_obs_out_device(fin, k)
    with pytest.raises(mg.MgymError) as ei:
        call(env, w, k + 1, R.RELU, head)
    assert ei.value.status == mg.envs.L.ERR_BAD_ARG and "mgym_rollout_mlp2" in str(ei.value) and "steps_cap" in str(ei.value)
    acts, gobs, grew, gdone, gtrunc = call(env, w, k, R.RELU, head, 1)
    outs, tobs, tdone, ttrunc = twin_steps(ref, twin, acts)
    for t, exp in enumerate(outs):
        for g, e, nm in zip((gobs[t], grew[t], gdone[t], gtrunc[t]), exp, ("obs", "reward", "done", "truncated")):
            assert same(g, e), f"step {t}: {nm}"
    fin.check(tobs, tdone | ttrunc, f"{fam} mlp2")
    assert (tdone | ttrunc).sum() >= n
    env.set_final_obs_out_device(None)
    env.close(); ref.close(); twin.close()


def test_errors_are_reported_before_any_launch():
    L = mg.envs.L
    w = weights("cartpole", 3, 5, R.RELU)

    def check(env, what, *args, **kw):
        before = env.get_state()
        with pytest.raises(mg.MgymError) as ei:
            env.rollout_mlp2_device(*args, **kw)
        msg = str(ei.value)
        assert ei.value.status == L.ERR_BAD_ARG and "mgym_rollout_mlp2:" in msg and what in msg, (what, msg)
        env.sync()
        assert same(env.get_state(), before)

    env = make("cartpole", 8, False)
    env.reset()
    pol, H1, H2 = env.pack_mlp2(*w)
    ok = dict(policy=pol, hidden1=3, hidden2=5, activation="relu", head="greedy", sigma=0.0, seed=1, call=0, K=4)
    check(env, "policy", **{**ok, "policy": None})
    for h in (0, 65, -3):
        check(env, "hidden1", **{**ok, "hidden1": h})
        check(env, "hidden2", **{**ok, "hidden2": h})
    for a in ("tanh", 2, -1, 4):
        check(env, "activation", **{**ok, "activation": a})
    for h in (3, -1):
        check(env, "head", **{**ok, "head": h})
    check(env, "MGYM_HEAD_GAUSS", **{**ok, "head": "gauss"})
    check(env, "K", **{**ok, "K": -1})
    with pytest.raises(mg.envs.PolicyShapeError):
        env.rollout_mlp2(w[0], w[1], w[2][:, :2], w[3], w[4], w[5], 4)
    with pytest.raises(mg.envs.PolicyShapeError):
        env.rollout_mlp2_device(pol[:-1], 3, 5, "relu", "greedy", 0.0, 0, 0, 4)
    env.close()
    for fam in ("mountain_car", "acrobot", "lunar_lander"):
        e = make(fam, 8, False)
        e.reset()
        p, h1, h2 = e.pack_mlp2(*weights(fam, 3, 5, R.RELU))
        check(e, "MGYM_HEAD_GAUSS", p, h1, h2, "relu", "gauss", 0.5, 1, 0, 4)
        e.close()
    for fam in ("mountain_car_continuous", "pendulum"):
        e = make(fam, 8, False)
        e.reset()
        p, h1, h2 = e.pack_mlp2(*weights(fam, 3, 5, R.RELU))
        check(e, "MGYM_HEAD_SAMPLE", p, h1, h2, "relu", "sample", 0.5, 1, 0, 4)
        for sigma in (float("nan"), float("inf"), -0.5):
            check(e, "sigma", p, h1, h2, "relu", "gauss", sigma, 1, 0, 4)
        e.rollout_mlp2_device(p, h1, h2, "relu", "greedy", float("nan"), 1, 0, 2)   # sigma is ignored by the heads that do not use it
        e.sync()
        e.close()
    odd = make("cartpole", 8, False, env_id_base=2)   # a drawing head keys one Philox block per 4 consecutive global env ids
    odd.reset()
    check(odd, "env_id_base", pol, 3, 5, "relu", "sample", 0.0, 1, 0, 4)
    odd.rollout_mlp2_device(pol, 3, 5, "relu", "greedy", 0.0, 1, 0, 2)
    odd.sync()
    odd.close()
    six = make("cartpole", 6, False)                  # the fused form: n_envs a multiple of 4
    six.reset()
    check(six, "multiple of 4", pol, 3, 5, "relu", "greedy", 0.0, 1, 0, 4)
    six.close()


def test_torch_rollout_mlp2_equals_vecenv():
    torch = pytest.importorskip("torch")
    fam, n = "acrobot", 1028
    te = mg.TorchVecEnv(KIND[fam], n, seed=31, auto_reset=True, max_episode_steps=LIMIT)
    ve = make(fam, n, True, LIMIT, seed=31)
    te.reset()
    ve.reset()
    w = weights(fam, 64, 64, R.TANH_FAST)
    got = te.rollout_mlp2(*(torch.from_numpy(x) for x in w), 6, activation="tanh_fast", head="sample", seed=POLICY_SEED, call=4)
    torch.cuda.synchronize()
    exp = ve.rollout_mlp2(*w, 6, activation="tanh_fast", head="sample", seed=POLICY_SEED, call=4)
    for g, e, nm in zip(got, exp, ("actions", "obs", "reward", "done", "truncated")):
        g = g.cpu().numpy()
        g = g.view(np.uint32) if g.dtype == np.int32 else g.astype(np.uint8) if g.dtype == np.bool_ else g
        assert same(g, e), nm
    ve.close()
