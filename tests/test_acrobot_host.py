"""No-GPU check of the Acrobot-v1 lines the kernels run: modurl_gym_amd/csrc/acrobot_step.h compiled for the host by tests/native/acrobot_check.cpp
(g++ -O2 -ffp-contract=off -fno-fast-math) against the word-exact restatement of include/mgym.h in tests/acrobot_ref.py — every output word equal.
256 envs x 64 steps with max_episode_steps = 7 and the fused auto-reset: 9 truncations and resets per environment."""
import subprocess

import numpy as np
import pytest

import acrobot_ref as R
from glibc_f32 import glibc_has_fdlibm_expm1f
from mlp_policy_ref import mlp_ref

F = np.float32
N, STEPS, LIMIT = 256, 64, 7
needs_fdlibm = pytest.mark.skipif(not glibc_has_fdlibm_expm1f(), reason="this glibc's expm1f is not the fdlibm one that mg_expm1f restates")


def table_actions(seed=3):
    return np.random.default_rng(seed).integers(0, 3, (STEPS, N)).astype(np.uint32)


def mlp_weights(H, seed=0):
    """weights that see the small sines and velocities of an arm a few steps from its reset: those inputs scaled up, the two cosines (near 1) taken
    out of the hidden bias"""
    rng = np.random.default_rng(40 + H + seed)
    w1 = rng.normal(0, 1.0, (H, 6)) * np.array([1.0, 10.0, 1.0, 10.0, 10.0, 10.0])
    b1 = rng.normal(0, 0.3, H) - w1[:, 0] - w1[:, 2]
    return np.concatenate([w1.ravel(), b1, rng.normal(0, 2.0 / np.sqrt(H), 3 * H), np.zeros(3)]).astype(F)


@pytest.mark.parametrize("seed", [0, 0x1234567811])
def test_reset_and_action_table_steps_equal_the_restatement(seed):
    kw = dict(seed=seed, env_id_base=1024, limit=LIMIT, auto_reset=True, actions=table_actions())
    got, exp = R.header_run(N, STEPS, **kw), R.ref_run(N, STEPS, **kw)
    R.assert_same_run(got, exp, f"seed {seed:#x}")
    assert got["finished"] == 9 * N and np.all(got["trunc"].sum(axis=0) == 9) and np.all(got["elapsed"] == STEPS - 9 * LIMIT) and not got["done"].any()
    assert np.all(got["state"][4] == 10)   # the episode number: the first reset and nine fused ones
    # the reset draws: four values in [-0.1, 0.1), all different, the trig words those of the angles
    st0 = R.reset_draw(seed, np.uint64(1024) + np.arange(N, dtype=np.uint64), np.zeros(N, np.uint32))
    assert all(np.abs(v).max() < 0.1 and len(np.unique(v)) > N // 2 for v in st0)
    assert R.same_words(got["obs0"], np.stack([R.cosf(st0[0]), R.sinf(st0[0]), R.cosf(st0[1]), R.sinf(st0[1]), st0[2], st0[3]]))
    assert np.all(got["reward"] == -1)


def test_limit_off_limit_without_reset_and_the_largest_limit():
    for limit, auto in ((0, True), (5, False), (65535, True)):
        kw = dict(seed=9, limit=limit, auto_reset=auto, actions=table_actions(4))
        got = R.header_run(N, STEPS, **kw)
        R.assert_same_run(got, R.ref_run(N, STEPS, **kw), f"limit {limit}")
        if limit == 5:   # no reset: truncated stays up from the fifth step on, the count goes on
            assert np.all(got["trunc"][:4] == 0) and np.all(got["trunc"][4:] == 1) and np.all(got["elapsed"] == STEPS)
        if limit == 0:   # a handle without a limit does not count
            assert not got["trunc"].any() and not got["elapsed"].any()


def test_uniform_policy_draws_equal_the_restatement():
    for call in (0, 1, 5):
        kw = dict(seed=2, env_id_base=4096, limit=LIMIT, auto_reset=True, policy=R.POL_UNIFORM, policy_seed=0xABCDEF12345, call=call)
        got = R.header_run(N, STEPS, **kw)
        R.assert_same_run(got, R.ref_run(N, STEPS, **kw), f"uniform call {call}")
        share = np.bincount(got["actions"].ravel(), minlength=3) / got["actions"].size
        assert got["actions"].max() == 2 and np.all(np.abs(share - 1 / 3) < 0.02)
    g = np.arange(8, dtype=np.uint64)
    assert [R.uniform_actions(1, 0, g, t).tolist() for t in range(8)] != [R.uniform_actions(1, 1, g, t).tolist() for t in range(8)]


def test_linear_policy_equals_the_restatement():
    rng = np.random.default_rng(17)
    swing = np.zeros(21, F)   # push with the first link's velocity once it is fast enough, else no torque
    swing[[4, 13, 18]] = -10.0, 0.3, 10.0
    pols = [swing, np.zeros(21, F), np.concatenate([np.full(7, 1e30), np.full(7, -1e30), rng.normal(0, 1, 7)]).astype(F)]
    pols[1][[6, 13, 20]] = 1.0   # three equal scores everywhere: the first wins
    for i, pol in enumerate(pols):
        kw = dict(seed=6, limit=LIMIT, auto_reset=True, policy=R.POL_LINEAR, weights=pol)
        got = R.header_run(N, STEPS, **kw)
        R.assert_same_run(got, R.ref_run(N, STEPS, **kw), f"linear {i}")
        if i == 0:
            assert len(np.unique(got["actions"])) == 3
        if i == 1:
            assert not got["actions"].any()


@pytest.mark.parametrize("act", [R.RELU, R.TANH])
@pytest.mark.parametrize("H", [1, 33, 64])
def test_mlp_policy_equals_the_restatement(H, act):
    w = mlp_weights(H)
    kw = dict(seed=8, limit=LIMIT, auto_reset=True, policy=R.POL_MLP_TANH if act == R.TANH else R.POL_MLP_RELU, weights=w, hidden=H)
    got = R.header_run(N, STEPS, **kw)
    R.assert_same_run(got, R.ref_run(N, STEPS, **kw), f"mlp H = {H} act {act}")
    assert H == 1 or len(np.unique(got["actions"])) >= 2   # a policy that really depends on the observation (one unit's largest output weight may be action 0's)
    # the chains are those of tests/mlp_ref.py: its one-observation form (mlp_policy_ref.mlp_ref) on the first observations
    for i in range(0, N, 37):
        word, _, _ = mlp_ref(6, 3, 0, act, H, w, got["obs0"][:, i])
        assert word == int(got["actions"][0, i])


@needs_fdlibm
@pytest.mark.parametrize("act", [R.RELU, R.TANH])
@pytest.mark.parametrize("H", [1, 33, 64])
def test_sampled_mlp_policy_equals_the_restatement(H, act):
    w = mlp_weights(H, 1)
    kw = dict(seed=8, env_id_base=8, limit=LIMIT, auto_reset=True, policy=R.POL_MLP_TANH_SAMPLE if act == R.TANH else R.POL_MLP_RELU_SAMPLE, weights=w, hidden=H,
              policy_seed=0x5EED5EED5, call=3)
    got = R.header_run(N, STEPS, **kw)
    R.assert_same_run(got, R.ref_run(N, STEPS, **kw), f"mlp_sample H = {H} act {act}")
    greedy = R.header_run(N, STEPS, **dict(kw, policy=R.POL_MLP_TANH if act == R.TANH else R.POL_MLP_RELU))
    assert len(np.unique(got["actions"])) == 3 and (got["actions"][0] != greedy["actions"][0]).any()   # drawn, not the argmax


def imported(th1, th2, w1, w2):
    cols = [np.resize(np.array(v, F), N) for v in (th1, th2, w1, w2)]
    return np.stack([R.words_of(c) for c in cols] + [np.arange(N, dtype=np.uint32)])


def test_imported_states_that_terminate_at_once():
    """th1 = pi, th2 = 0: the arm points straight up, and the first step (whatever the action) reports done with reward 0; then the fused reset"""
    st = imported([np.pi], [0.0], [0.0], [0.0])
    for auto in (True, False):
        kw = dict(seed=1, limit=LIMIT, auto_reset=auto, actions=table_actions(11), state=st)
        got, exp = R.header_run(N, STEPS, **kw), R.ref_run(N, STEPS, **kw)
        R.assert_same_run(got, exp, f"upright, auto_reset {auto}")
        assert np.all(got["done"][0] == 1) and np.all(got["reward"][0] == 0) and np.all(got["trunc"][0] == 0)
        assert R.same_words(got["obs0"][0], R.cosf(st[0].view(F))) and R.same_words(got["obs0"][1], R.sinf(st[0].view(F)))   # the trig words of the imported angle
        if auto:
            assert np.all(np.abs(got["obs"][0][4:]) < 0.1) and np.all(got["elapsed"] == (STEPS - 1) % LIMIT)   # reset at step 0, then every 7 steps
        else:
            assert got["done"][1:].any() and not got["done"][1:].all()   # stepped on, the arm falls: done is recomputed, not sticky


def test_imported_states_that_never_settle_and_leave_the_fast_range():
    """velocities beyond the clamps, angles far outside [-pi, pi] (taken as they are: the table reduction serves the stage angles), the largest floats"""
    st = imported([2.0, 1e6, -3.1415927, 1000.0, 0.0, 119.9, -120.5], [-1.0, -12345.678, 0.0, -0.0, 3.1415927, -125.0, 0.3], [13.0, -12.0, 1.0, 1e30, -12.566371, 40.0, 0.0],
                  [-29.0, 28.0, -1.0, -1e30, 28.274334, -90.0, 1e-30])
    for limit in (0, LIMIT):
        kw = dict(seed=1, limit=limit, auto_reset=bool(limit), actions=table_actions(12), state=st)
        got = R.header_run(N, STEPS, **kw)
        R.assert_same_run(got, R.ref_run(N, STEPS, **kw), f"never settle, limit {limit}")
        o = got["obs"][:, :, np.arange(N) % 7 != 3]   # (1e30 velocities give infinities inside the stages: NaNs, next test)
        assert np.all(np.abs(o[:, 4]) <= R.V1) and np.all(np.abs(o[:, 5]) <= R.V2) and (np.abs(o[0, 4]) == R.V1).any() and (np.abs(o[0, 5]) == R.V2).any()


def test_an_infinity_a_nan_and_an_invalid_action_return_and_equal_the_restatement():
    inf, nan = np.inf, np.nan
    st = imported([inf, 0.5, 0.1, 0.2, -inf, 0.3], [0.25, nan, 0.1, 0.2, 0.0, 0.3], [1.0, 0.0, inf, 0.0, 0.0, nan], [0.0, 1.0, 0.0, -inf, 0.0, 0.0])
    acts = table_actions(13)
    acts[0, 5], acts[3, 100], acts[6, 7], acts[2, 30] = 3, 0xFFFFFFFF, 3, 1 << 31   # invalid; the third on a step that truncates
    for auto in (True, False):
        kw = dict(seed=1, limit=LIMIT, auto_reset=auto, actions=acts, state=st)
        got, exp = R.header_run(N, STEPS, **kw), R.ref_run(N, STEPS, **kw)
        R.assert_same_run(got, exp, f"non-finite, auto_reset {auto}")
        assert got["bad"] and np.isnan(got["obs"][0]).any() and not got["done"][0].any()   # NaNs never terminate
        assert R.same_words(got["obs"][0][:, 5], got["obs0"][:, 5]) and got["reward"][0, 5] == 0 and got["trunc"][0, 5] == 0   # the refused step leaves the observation
        assert got["trunc"][6, 7] == 1   # the count advances on a refused step too (the MountainCar rule)
        if not auto:
            assert np.isnan(got["state"][:4].view(F)[:, 0]).all()   # an infinite angle poisons the whole state and stays
    kw = dict(seed=1, limit=0, actions=table_actions(14), state=st)
    R.assert_same_run(R.header_run(N, STEPS, **kw), R.ref_run(N, STEPS, **kw), "non-finite, no limit")


def test_program_runs_its_scenario():
    """the stand-alone program (what a sanitizer build runs) goes through every policy; its first table case is reproducible from here"""
    exe = R.check_program()
    out = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout.splitlines()
    assert len(out) == 9 and all(line.startswith(f"case {i} ") for i, line in enumerate(out))
    fields = [dict(zip(line.split()[2::2], (int(v) for v in line.split()[3::2]))) for line in out]
    assert [f["bad"] for f in fields] == [1, 0, 0, 0, 0, 0, 0, 1, 1]          # the invalid action of the table is seen by the table cases alone
    assert all(f["finished"] == 9 * N for f in fields[:7]) and fields[7]["done"] > 0
    rs, vals = 12345, []
    for _ in range(STEPS * N):
        rs = (rs * 1664525 + 1013904223) & 0xFFFFFFFF
        vals.append((rs >> 8) % 3)
    acts = np.array(vals, np.uint32).reshape(STEPS, N)
    acts[0, 5] = 3
    exp = R.ref_run(N, STEPS, seed=0x1234567811, env_id_base=1024, limit=LIMIT, auto_reset=True, actions=acts)
    total = lambda a: int(R.words_of(a).astype(np.uint64).sum())
    assert fields[0]["obs0"] == total(exp["obs0"]) and fields[0]["obs"] == total(exp["obs"]) and fields[0]["reward"] == total(exp["reward"])
    assert fields[0]["truncated"] == int(exp["trunc"].sum()) and fields[0]["state"] == int(exp["state"].astype(np.uint64).sum())


def test_abi_knows_the_kind_without_a_gpu():
    """spec, defaults and the configuration error are decided before the first HIP call"""
    import ctypes as C

    import modurl_gym_amd as mg
    from modurl_gym_amd import _lib as L
    s = mg.get_spec(mg.ACROBOT)
    assert mg.ACROBOT == 6 and (s.obs_dim, s.n_actions, s.action_is_float, s.state_cols) == (6, 3, 0, 5)
    assert list(s.obs_high[:6]) == [1.0, 1.0, 1.0, 1.0, float(R.V1), float(R.V2)] and list(s.obs_low[:6]) == [-1.0, -1.0, -1.0, -1.0, -float(R.V1), -float(R.V2)]
    cfg = L.Config()
    assert L.load().mgym_default_config(mg.ACROBOT, C.byref(cfg)) == L.OK
    assert (cfg.kind, cfg.max_episode_steps, cfg.struct_size) == (6, 0, C.sizeof(L.Config)) and L.load().mgym_abi_version() == 4
    for unknown in (5, 7, -1):   # 5 is not assigned
        assert L.load().mgym_default_config(unknown, C.byref(cfg)) == L.ERR_BAD_ARG
    spec = L.Spec()
    assert L.load().mgym_get_spec(5, C.byref(spec)) == L.ERR_BAD_ARG
    with pytest.raises(mg.BadConfigError):
        mg.VecEnv(mg.ACROBOT, 4, max_episode_steps=70000)
    assert mg.envs.KIND_NAMES[mg.ACROBOT] == "AcrobotV1" and mg.AcrobotV1.KIND == mg.ACROBOT
