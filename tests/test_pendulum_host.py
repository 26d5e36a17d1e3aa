"""No-GPU check of the Pendulum-v1 lines the kernels run: modurl_gym_amd/csrc/pendulum_step.h compiled for the host by tests/native/pendulum_check.cpp
(g++ -O2 -ffp-contract=off -fno-fast-math) against the word-exact restatement of include/mgym.h in tests/pendulum_ref.py — every output word equal.
256 envs x 64 steps with max_episode_steps = 7 and the fused auto-reset: 9 truncations and resets per environment."""
import subprocess

import numpy as np
import pytest

import pendulum_ref as R
from mlp_policy_ref import mlp_ref

F = np.float32
N, STEPS, LIMIT = 256, 64, 7


def table_actions(seed=3):
    rng = np.random.default_rng(seed)
    return rng.uniform(-2.5, 2.5, (STEPS, N)).astype(F)


def mlp_weights(H, seed=0):
    rng = np.random.default_rng(40 + H + seed)
    return np.concatenate([rng.normal(0, 1.5, H * 3), rng.normal(0, 0.5, H), rng.normal(0, 2.0 / np.sqrt(H), H), rng.normal(0, 0.3, 1)]).astype(F)


@pytest.mark.parametrize("seed", [0, 0x1234567811])
def test_reset_and_action_table_steps_equal_the_restatement(seed):
    kw = dict(seed=seed, env_id_base=1024, limit=LIMIT, auto_reset=True, actions=table_actions())
    got, exp = R.header_run(N, STEPS, **kw), R.ref_run(N, STEPS, **kw)
    R.assert_same_run(got, exp, f"seed {seed:#x}")
    assert got["finished"] == 9 * N and np.all(got["trunc"].sum(axis=0) == 9) and np.all(got["elapsed"] == STEPS - 9 * LIMIT)
    assert np.all(got["state"][2] == 10)   # the episode number: the first reset and nine fused ones
    assert np.all(np.abs(got["obs0"][2]) <= 1) and len(np.unique(got["obs0"][0])) > N // 2   # thdot ~ U[-1, 1), angles all different
    assert (np.abs(exp["actions"]) > 2).any()   # torques beyond the clamp were fed


def test_other_gravity_and_no_limit():
    for g, limit, auto in ((9.81, 0, True), (0.0, 5, False), (-3.5, 65535, True)):
        kw = dict(seed=9, g=g, limit=limit, auto_reset=auto, actions=table_actions(4))
        got = R.header_run(N, STEPS, **kw)
        R.assert_same_run(got, R.ref_run(N, STEPS, **kw), f"g = {g}, limit {limit}")
        if limit == 5:   # no reset: truncated stays up from the fifth step on, the count goes on
            assert np.all(got["trunc"][:4] == 0) and np.all(got["trunc"][4:] == 1) and np.all(got["elapsed"] == STEPS)
        if limit == 0:   # a handle without a limit does not count
            assert not got["trunc"].any() and not got["elapsed"].any()


def test_uniform_policy_draws_equal_the_restatement():
    for call in (0, 1, 5):
        kw = dict(seed=2, env_id_base=4096, limit=LIMIT, auto_reset=True, policy=R.POL_UNIFORM, policy_seed=0xABCDEF12345, call=call)
        got = R.header_run(N, STEPS, **kw)
        R.assert_same_run(got, R.ref_run(N, STEPS, **kw), f"uniform call {call}")
        a = got["actions"]
        assert a.min() >= -2 and a.max() < 2 and np.all(a * F(2 ** 22) == np.round(a * F(2 ** 22)))   # multiples of 2^-22 in [-2, 2)
        assert abs(float(a.mean())) < 0.05 and len(np.unique(a)) > a.size // 2
    assert R.words_of(R.uniform_actions(1, 0, np.arange(4, dtype=np.uint64), 0)).tolist() != R.words_of(R.uniform_actions(1, 1, np.arange(4, dtype=np.uint64), 0)).tolist()


def test_linear_policy_equals_the_restatement():
    for pol in ((-2.0, 3.0, -1.0, 0.25), (0.0, 0.0, 0.0, 5.0), (1e30, -1e30, 1.0, 0.0)):
        kw = dict(seed=6, limit=LIMIT, auto_reset=True, policy=R.POL_LINEAR, weights=np.array(pol, F))
        R.assert_same_run(R.header_run(N, STEPS, **kw), R.ref_run(N, STEPS, **kw), f"linear {pol}")


@pytest.mark.parametrize("act", [R.RELU, R.TANH])
@pytest.mark.parametrize("H", [1, 33, 64])
def test_mlp_policy_equals_the_restatement(H, act):
    w = mlp_weights(H)
    kw = dict(seed=8, limit=LIMIT, auto_reset=True, policy=R.POL_MLP_TANH if act == R.TANH else R.POL_MLP_RELU, weights=w, hidden=H)
    got = R.header_run(N, STEPS, **kw)
    R.assert_same_run(got, R.ref_run(N, STEPS, **kw), f"mlp H = {H} act {act}")
    assert len(np.unique(got["actions"])) > N   # a policy that really depends on the observation
    # the chains are those of tests/mlp_ref.py: its one-observation form (mlp_policy_ref.mlp_ref) on the first observations
    obs0 = got["obs0"]
    for i in range(0, N, 37):
        word, _, _ = mlp_ref(3, 1, 1, act, H, w, obs0[:, i])
        assert word == int(R.words_of(got["actions"][0, i:i + 1])[0])


def imported_state():
    th = np.array([R.BIG_TH[i % len(R.BIG_TH)] for i in range(N)], F)
    thdot = ((np.arange(N) % 17) - 8).astype(F)
    return np.stack([R.words_of(th), R.words_of(thdot), np.arange(N, dtype=np.uint32)])


def test_imported_large_angles_and_a_nan_action():
    st = imported_state()
    acts = table_actions(11)
    acts[0, 5], acts[3, 100], acts[6, 7] = np.nan, np.nan, np.nan   # the last one on a step that truncates
    acts[1, 9], acts[1, 10] = np.inf, -np.inf
    for auto in (True, False):
        kw = dict(seed=1, limit=LIMIT, auto_reset=auto, actions=acts, state=st)
        got, exp = R.header_run(N, STEPS, **kw), R.ref_run(N, STEPS, **kw)
        R.assert_same_run(got, exp, f"imported, auto_reset {auto}")
        assert got["bad"]
        # cos and sin of the imported words are glibc's, and the refused step leaves the observation and gives reward 0
        assert R.same_words(got["obs0"][0], R.cosf(st[0].view(F))) and R.same_words(got["obs0"][1], R.sinf(st[0].view(F)))
        assert R.same_words(got["obs"][0][:, 5], got["obs0"][:, 5]) and got["reward"][0, 5] == 0 and got["trunc"][0, 5] == 0
        assert got["trunc"][6, 7] == 1   # the count advances on a refused step too (the MountainCar rule)
        # +-inf clamp: the same words as +-2
        a2 = acts.copy()
        a2[1, 9], a2[1, 10] = 2.0, -2.0
        again = R.header_run(N, STEPS, **dict(kw, actions=a2))
        assert R.same_words(again["obs"][1], got["obs"][1]) and R.same_words(again["reward"][1], got["reward"][1])
    kw = dict(seed=1, limit=0, actions=table_actions(12), state=st)   # no limit: th keeps growing from +-1e6
    R.assert_same_run(R.header_run(N, STEPS, **kw), R.ref_run(N, STEPS, **kw), "imported, no limit")


def test_program_runs_its_scenario():
    """the stand-alone program (what a sanitizer build runs) goes through every policy; its table cases are reproducible from here"""
    exe = R.check_program()
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == 7 and all(line.startswith(f"case {i} ") for i, line in enumerate(out))
    fields = [dict(zip(line.split()[2::2], (int(v) for v in line.split()[3::2]))) for line in out]
    assert [f["bad"] for f in fields] == [1, 0, 0, 0, 0, 1, 1]          # the NaN action of the table is seen by the table cases alone
    assert all(f["finished"] == 9 * N for f in fields[:5]) and fields[6]["finished"] == 0
    # case 0 from the restatement: the program's generator, restated
    rs, vals = 12345, []
    for _ in range(STEPS * N):
        rs = (rs * 1664525 + 1013904223) & 0xFFFFFFFF
        vals.append(rs >> 8)
    acts = (np.array(vals, np.uint32).astype(F) * F(5.0 / 16777216.0) - F(2.5)).reshape(STEPS, N)
    acts[0, 5] = np.nan
    exp = R.ref_run(N, STEPS, seed=0x1234567811, env_id_base=1024, limit=LIMIT, auto_reset=True, actions=acts)
    nan_free = lambda a: int(R.words_of(a).astype(np.uint64).sum())
    assert fields[0]["obs0"] == nan_free(exp["obs0"]) and fields[0]["obs"] == nan_free(exp["obs"]) and fields[0]["reward"] == nan_free(exp["reward"])
    assert fields[0]["truncated"] == int(exp["trunc"].sum()) and fields[0]["state"] == int(exp["state"].astype(np.uint64).sum())


def test_abi_knows_the_kind_without_a_gpu():
    """spec, defaults and the two configuration errors are decided before the first HIP call"""
    import ctypes as C

    import modurl_gym_amd as mg
    from modurl_gym_amd import _lib as L
    s = mg.get_spec(mg.PENDULUM)
    assert mg.PENDULUM == 4 and (s.obs_dim, s.n_actions, s.action_is_float, s.state_cols) == (3, 0, 1, 3) and (s.action_low, s.action_high) == (-2.0, 2.0)
    assert list(s.obs_high[:3]) == [1.0, 1.0, 8.0] and list(s.obs_low[:3]) == [-1.0, -1.0, -8.0]
    cfg = L.Config()
    assert L.load().mgym_default_config(mg.PENDULUM, C.byref(cfg)) == L.OK
    assert (cfg.kind, cfg.gravity, cfg.max_episode_steps, cfg.struct_size) == (4, 10.0, 0, C.sizeof(L.Config)) and L.load().mgym_abi_version() == 4
    assert L.load().mgym_default_config(5, C.byref(cfg)) == L.ERR_BAD_ARG
    for kw in (dict(gravity=float("inf")), dict(gravity=float("nan")), dict(max_episode_steps=70000)):
        with pytest.raises(mg.BadConfigError):
            mg.VecEnv(mg.PENDULUM, 4, **kw)
    assert mg.envs.KIND_NAMES[mg.PENDULUM] == "PendulumV1" and mg.PendulumV1.KIND == mg.PENDULUM
