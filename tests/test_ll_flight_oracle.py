"""The CPU oracle's airborne LunarLander step against the float64 reference of the step (tests/ll_flight_ref.py), no GPU.

Every other LunarLander test compares implementations that were written from one understanding of Box2D and of
lunar_lander.rs with each other; this one compares them with a restatement of the definitions in numpy: three bodies, two
revolute joints with limit and motor, gravity, wind, the engine impulses, observation and reward.  The cases, the protocol
and the conditions on them are in tests/ll_flight_cases.py; the bounds and where they come from in tests/ll_flight_ref.py.

tests/test_ll_host.py proves the kernel source compiled for the host equal to the oracle bit for bit, so what holds for the
oracle here holds for that source (ll_free.h, ll_world.h, ll_env.h) too; tests/test_gpu_ll_flight.py runs the same checks on
the engine's three free-flight paths."""
import numpy as np
import pytest

import ll_flight_cases as FC
import ll_flight_ref as R
from oracle import oracle as ora


def oracle(name, n, **kw):
    g, wind, wp, tp = FC.PARAMS[name]
    return ora.OracleVec(ora.LUNARLANDER, n, gravity=g, enable_wind=wind, wind_power=wp, turbulence_power=tp, **kw)


def test_cases_cover_every_solver_branch_and_stay_airborne():
    blob, actions, disp, kind = FC.cases()
    n = blob.shape[1]
    assert n >= 4096 + 16 * (len(FC.CLASSES) - 1) and n % 64 != 0
    assert all((actions == a).mean() > 0.2 for a in range(4))
    for name in FC.PARAMS:
        traj = FC.trajectory(name)                 # asserts the activity counts and the airborne condition
        print(name, traj["counts"], "lowest vertex %.3f" % traj["lowest"].min())
    # the hand-built classes reach what they were built for
    first = {k: v[0] for k, v in FC.trajectory("calm")["flags"].items()}
    cls = lambda c: kind == FC.CLASSES.index(c)
    assert first["translation_clamp"][cls("fast_150")].all() and first["rotation_clamp"][cls("spin_100")].all()
    assert first["motor_clamp"][cls("leg_spin_600")].sum() >= 8 and first["angular_clamp"][cls("far_outside")].all()
    k = cls("at_limits")
    for j in range(2):
        joint = blob[6 * (1 + j) + 2, k].astype(np.float64) - blob[2, k]
        assert np.minimum(np.abs(joint - R.LOWER[j]), np.abs(joint - R.UPPER[j])).max() < 1e-6


@pytest.mark.parametrize("name", list(FC.PARAMS))
def test_oracle_steps_match_the_float64_reference(name):
    """(a) reset_deterministic(), set_state(cases), T steps: all 18 pose / velocity words, observation, reward, done and leg
    flags after every step, wind off, wind on and near the builder's ends"""
    FC.check_against_reference(oracle(name, FC.cases()[0].shape[1]), name, f"oracle {name}")


def test_oracle_dispersion_matches_the_float64_reference():
    """(b) the engines' dispersion terms, which deterministic mode ignores: the difference between two handles that differ in the
    dispersion override only, and both handles' words after reset() + set_state + one step"""
    n = FC.cases()[0].shape[1]
    FC.check_dispersion_differential(lambda: oracle("wind", n, seed=7), "oracle")


def test_reference_conserves_momentum():
    """the reference against a closed form it was not written from: the joints are internal, so without wind the craft's
    momentum changes by M g h per step plus the engine's impulse (:994-997, :1039-1042), whatever the solver does"""
    blob, _, _, _ = FC.cases()
    keep = ~FC.clamp_mask()                        # (Box2D's clamps rescale velocities: not conservative)
    ref = R.FlightRef(blob[:, keep])
    for action in (0, 2, 1, 3):
        P0 = (R.MASS[None, :, None] * ref.v).sum(1)
        tip = np.stack([np.sin(ref.a[:, 0]), np.cos(ref.a[:, 0])], -1)
        ref.step(np.full(ref.n, action))
        P1 = (R.MASS[None, :, None] * ref.v).sum(1)
        J = {0: 0.0, 2: R.MAIN_ENGINE_POWER * R.MAIN_Y * np.stack([-tip[:, 0], tip[:, 1]], -1)}.get(action)
        if J is None:                              # side engine: -0.6 (side . direction 12 / 30) along (side.x, -side.y)
            J = R.SIDE_ENGINE_POWER * (action - 2) * 12.0 / 30.0 * np.stack([tip[:, 1], tip[:, 0]], -1)
        assert np.abs(P1 - P0 - J - np.array([0.0, R.MASS.sum() * ref.gravity * R.H])).max() < 1e-12
