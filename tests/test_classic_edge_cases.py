"""No-GPU checks of the edge cases of tests/classic_edge_cases.py: the builders' own guarantees, the host-compiled Pendulum and Acrobot headers against
the restatements on them (finite and non-finite sets, two steps, without a limit and with limit 1 and the fused auto-reset), and the evidence that
the denormal cases would notice a build that flushes: run with the x86 flush-to-zero and denormals-are-zero bits set, the very same header disagrees
with the restatement."""
import numpy as np
import pytest

import acrobot_ref as AR
import classic_edge_cases as E
import pendulum_ref as PR
from oracle import oracle as ora

F = np.float32
BUILDERS = {"pendulum": (E.pendulum_cases, 3, F), "acrobot": (E.acrobot_cases, 5, np.uint32), "mountain_car": (lambda: E.mountain_car_cases(False), 3, np.uint32),
            "mountain_car_continuous": (lambda: E.mountain_car_cases(True), 3, F), "cartpole": (E.cartpole_cases, 7, np.uint32),
            "pendulum-non_finite": (lambda: E.non_finite_cases("pendulum"), 3, F), "acrobot-non_finite": (lambda: E.non_finite_cases("acrobot"), 5, np.uint32),
            "mountain_car_continuous-non_finite": (lambda: E.non_finite_cases("mountain_car_continuous"), 3, F)}


@pytest.mark.parametrize("name", list(BUILDERS))
def test_builder_guarantees(name):
    """the presence assertions live in the builders (they run on every call that is not cached); here: the form, and that the order is deterministic"""
    build, cols, act_dtype = BUILDERS[name]
    blob, a = build()
    n = blob.shape[1]
    assert blob.dtype == np.uint32 and blob.shape == (cols, n) and a.shape == (n,) and a.dtype == act_dtype
    assert 0 < n <= 65536 and n % 1024 == 0
    assert np.array_equal(blob[-1], np.arange(n))   # the episode column
    fresh = getattr(build, "__wrapped__", None)
    if fresh is not None:   # built again from nothing: the same words
        blob2, a2 = fresh()
        assert np.array_equal(blob, blob2) and np.array_equal(a.view(np.uint32), a2.view(np.uint32))


def test_case_lists_hold_what_the_issue_names():
    has = lambda lst, v: bool((E.words(lst) == E.words([v])[0]).any())
    for v in (0.0, -0.0, 1e-45, -1e-40, 1.1754944e-38, 120.0, np.nextafter(F(120), F(0)), -1e30, 2.0 ** 24, E.FLT_MAX, -E.FLT_MAX, E.PI_F, -E.TWO_PI_F):
        assert has(E.PD_TH, F(v)), v
    for v in (8.0, np.nextafter(F(8), F(9)), -7.9, 1e-20, 100.0, -3e38):
        assert has(E.PD_THDOT, F(v)), v
    for v in (2.0, np.nextafter(F(-2), F(-3)), np.inf, -np.inf, 1e30, 3e38, -0.0):
        assert has(E.PD_TORQUE, F(v)), v
    for v in (119.0, -120.0, 1e6, -1e30, 2 * np.pi / 3):
        assert has(E.AB_TH1, F(v)), v
    assert has(E.AB_TH2, F(-12345.678)) and has(E.AB_W1, E.V1) and has(E.AB_W1, F(1e30)) and has(E.AB_W2, -E.V2) and has(E.AB_W2, F(-29))
    assert has(E.MC_POS, F(-1.2)) and has(E.MC_POS, F(0.6) - F(0.07)) and has(E.MC_VEL, F(-0.03)) and has(E.MCC_FORCE, F(-np.inf))
    assert has(E.CP_X, F(-2.4)) and has(E.CP_THETA, E.CP_THETA_THR) and has(E.CP_THETA, F(119.99)) and has(E.CP_VEL, F(1e30))
    assert float(E.CP_THETA_THR) == pytest.approx(12 * 2 * np.pi / 360, rel=1e-6)


def test_oracle_evaluates_its_families_cases():
    for kind, (blob, a), cfgs in ((ora.MOUNTAINCAR, E.mountain_car_cases(False), [dict(goal_velocity=g) for g in E.MC_GOAL_VELOCITIES]),
                                  (ora.MOUNTAINCAR_CONT, E.mountain_car_cases(True), [dict(goal_velocity=g) for g in E.MC_GOAL_VELOCITIES]),
                                  (ora.MOUNTAINCAR_CONT, E.non_finite_cases("mountain_car_continuous"), [{}]),
                                  (ora.CARTPOLE, E.cartpole_cases(), [dict(sutton_barto_reward=sb, is_euler=eu) for sb, eu in E.CP_CONFIGS])):
        for cfg in cfgs:
            obs, rew, done, trunc = E.oracle_step(kind, blob, a, **cfg)
            assert obs.shape[1] == blob.shape[1] and set(np.unique(done)) <= {0, 1} and set(np.unique(trunc)) <= {0, 1}


def two_steps(a):
    """the case actions, then a rotation of them"""
    return np.stack([a, np.roll(a, 7)])


RUNS = [dict(limit=0, auto_reset=False), dict(limit=1, auto_reset=True)]


@pytest.mark.parametrize("run", RUNS, ids=["no_limit", "limit1_auto_reset"])
@pytest.mark.parametrize("cases", ["finite", "non_finite"])
def test_pendulum_header_equals_the_restatement(cases, run):
    blob, a = E.pendulum_cases() if cases == "finite" else E.non_finite_cases("pendulum")
    n = blob.shape[1]
    kw = dict(seed=77, actions=two_steps(a), state=blob, **run)
    got, exp = PR.header_run(n, 2, **kw), PR.ref_run(n, 2, **kw)
    PR.assert_same_run(got, exp, f"pendulum {cases} {run}")
    assert got["finished"] == (2 * n if run["limit"] else 0)
    if cases == "finite":   # the other gravities on the subset
        sub = E.pendulum_gravity_subset()
        for g in (0.0, -3.5):
            kw = dict(seed=77, g=g, actions=np.ascontiguousarray(two_steps(a)[:, sub]), state=np.ascontiguousarray(blob[:, sub]), **run)
            PR.assert_same_run(PR.header_run(len(sub), 2, **kw), PR.ref_run(len(sub), 2, **kw), f"pendulum g = {g} {run}")


@pytest.mark.parametrize("run", RUNS, ids=["no_limit", "limit1_auto_reset"])
@pytest.mark.parametrize("cases", ["finite", "non_finite"])
def test_acrobot_header_equals_the_restatement(cases, run):
    blob, a = E.acrobot_cases() if cases == "finite" else E.non_finite_cases("acrobot")
    n = blob.shape[1]
    kw = dict(seed=78, actions=two_steps(a), state=blob, **run)
    got, exp = AR.header_run(n, 2, **kw), AR.ref_run(n, 2, **kw)
    AR.assert_same_run(got, exp, f"acrobot {cases} {run}")
    if run["limit"]:
        assert got["finished"] == 2 * n   # (every observation is a reset's)
    else:
        assert np.isnan(got["obs"][0]).any(axis=0).sum() >= (n // 3 if cases == "non_finite" else 1000)


def differing_cases(got, exp, keys):
    bad = np.zeros(got["reward"].shape[-1], bool)
    for k in keys:
        g, e = np.ascontiguousarray(got[k], F), np.ascontiguousarray(exp[k], F)
        d = ~((g.view(np.uint32) == e.view(np.uint32)) | (np.isnan(g) & np.isnan(e)))
        bad |= d.reshape(-1, d.shape[-1]).any(axis=0)
    return bad


def test_denormal_cases_notice_a_flushing_build():
    """The host-compiled header with denormals flushed (inputs read as zero, results written as zero) is what a device build that flushes would
    compute.  It must disagree with the restatement on the edge cases, on words that the denormal cases produce; without the bits it agrees (above)."""
    blob, a = E.pendulum_cases()
    n = blob.shape[1]
    kw = dict(seed=77, actions=a[None, :], state=blob)
    exp = PR.ref_run(n, 1, **kw)
    PR.assert_same_run(PR.header_run(n, 1, **kw), exp, "pendulum, not flushed")
    bad = differing_cases(PR.header_run(n, 1, flush=True, **kw), exp, ("obs", "reward"))
    tiny_out = E.is_denormal(exp["reward"][0]) | E.is_denormal(exp["obs"][0]).any(axis=0)
    assert bad.sum() >= 100 and (bad & tiny_out).sum() >= 16
    blob, a = E.acrobot_cases()
    n = blob.shape[1]
    kw = dict(seed=78, actions=a[None, :], state=blob)
    exp = AR.ref_run(n, 1, **kw)
    AR.assert_same_run(AR.header_run(n, 1, **kw), exp, "acrobot, not flushed")
    bad = differing_cases(AR.header_run(n, 1, flush=True, **kw), exp, ("obs",))
    assert bad.sum() >= 16
    # the flag is restored: a run after the flushed one agrees again
    AR.assert_same_run(AR.header_run(n, 1, **kw), exp, "acrobot, after the flushed run")
