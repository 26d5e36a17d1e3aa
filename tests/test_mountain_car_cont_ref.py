"""MountainCarContinuous: one step of the CPU oracle (the f32 semantics the kernels are tied to word for word) against gymnasium's step in float64
(tests/mountain_car_cont_ref.py), from the same f32 state.  No GPU: tests/test_gpu_classic_edges.py ties the device to the oracle.

Cases: per goal velocity (0, 0.03) 262 144 seeded states, nine tenths uniform over the box [-1.2, 0.6] x [-0.07, 0.07] and a tenth within 0.005 of
the wall and of the goal position with velocities within 0.002 of 0, +-0.07 and the goal velocity, forces uniform in [-1.5, 1.5]; plus the cases of
classic_edge_cases.mountain_car_cases(True) whose force lies in [-1.5, 1.5] (the others give an infinite or 1e59 reward, where no bound is meant).

Bounds: 4 x the worst deviations measured on the seeded cases (the factor is for platform libm differences in cosf) — measured 6.36e-8 (position:
half an ulp of a position above 1), 4.18e-9 (velocity: half an ulp of a speed above 0.0625, plus the position's share through cos), 3.83e-6 (reward:
half an ulp of 100 on terminating steps).  done must be equal wherever the float64 p' is at least 2e-7 from 0.45 and v' at least 5e-8 from the goal
velocity (or v' is the wall's exact 0); the excluded share of the seeded cases is at most 0.1 %, and on them no flag differs at all.

The step has two discontinuities, and the builder's cases sit on them by construction (a stepped position one float from -1.2 or 0.45): the wall
zeroes a negative velocity, and termination adds 100 to the reward.  The f32 word -1.2f is not float64's -1.2, so on those cases the two steps may
take different sides.  The position is compared on every case; the velocity where both steps or neither hit the wall, the reward where done agrees:
on every seeded case, and on the builder's cases outside the 2e-7 band of the two positions."""
import numpy as np
import pytest

import classic_edge_cases as E
from mountain_car_cont_ref import step_f64
from oracle import oracle as ora

F = np.float32
N_SEEDED = 262144
MEASURED = dict(position=6.36e-8, velocity=4.18e-9, reward=3.83e-6)
BOUND = {k: 4 * v for k, v in MEASURED.items()}


def seeded_cases(goal_velocity):
    rng = np.random.default_rng(450 + int(goal_velocity * 100))
    p = rng.uniform(-1.2, 0.6, N_SEEDED)
    v = rng.uniform(-0.07, 0.07, N_SEEDED)
    near = N_SEEDED // 10
    p[:near] = rng.choice([-1.2, 0.45, 0.6], near) + rng.uniform(-0.005, 0.005, near)
    v[:near] = rng.choice([0.0, 0.07, -0.07, goal_velocity], near) + rng.uniform(-0.002, 0.002, near)
    a = rng.uniform(-1.5, 1.5, N_SEEDED)
    return np.clip(p, -1.2, 0.6).astype(F), np.clip(v, -0.07, 0.07).astype(F), a.astype(F)


def builder_cases():
    blob, a = E.mountain_car_cases(True)
    keep = np.abs(a) <= 1.5
    return blob[0].view(F)[keep], blob[1].view(F)[keep], a[keep]


def compare(p, v, a, goal_velocity):
    """-> (worst deviations, done flags that differ outside the band, share of cases inside the band)"""
    blob = np.stack([E.words(p), E.words(v), np.zeros(len(p), np.uint32)])
    obs, rew, done, trunc = E.oracle_step(ora.MOUNTAINCAR_CONT, blob, a, goal_velocity=goal_velocity)
    p64, v64, term, rew64 = step_f64(p, v, a, F(goal_velocity))
    assert not trunc.any()
    clear = ((np.abs(p64 - 0.45) >= 2e-7) & (np.abs(v64 - float(F(goal_velocity))) >= 5e-8)) | (v64 == 0.0)
    differ = done.astype(bool) != term
    wall64, wall32 = (p64 == -1.2) & (v64 == 0.0), (obs[0] == F(-1.2)) & (obs[1] == 0)
    same_wall, same_done = wall64 == wall32, ~differ
    worst = dict(position=float(np.abs(obs[0] - p64).max()), velocity=float(np.abs(obs[1] - v64)[same_wall].max()),
                 reward=float(np.abs(rew - rew64)[same_done].max()))
    off_band = (np.abs(p64 + 1.2) >= 2e-7) & (np.abs(p64 - 0.45) >= 2e-7)
    sides = int((~same_wall & off_band).sum()) + int((~same_done & off_band & clear).sum())   # different sides of a discontinuity away from it: none
    return worst, int((differ & clear).sum()) + sides, 1.0 - float(clear.mean()), int(term.sum()), int(differ.sum()) + int((~same_wall).sum())


@pytest.mark.parametrize("goal_velocity", E.MC_GOAL_VELOCITIES)
@pytest.mark.parametrize("cases", ["seeded", "builder"])
def test_oracle_step_is_within_the_recorded_bounds_of_the_float64_step(cases, goal_velocity):
    p, v, a = seeded_cases(goal_velocity) if cases == "seeded" else builder_cases()
    worst, wrong, excluded, terminated, differ = compare(p, v, a, goal_velocity)
    print(f"{cases} goal_velocity {goal_velocity}: n {len(p)} worst {worst} terminated {terminated} done or wall differs {differ} ({wrong} outside the band), excluded share {excluded:.2e}")
    assert terminated >= 100 and (np.abs(a) > 1).any()
    for k, b in BOUND.items():
        assert worst[k] <= b, f"{k}: {worst[k]:.3e} above {b:.3e}"
    assert wrong == 0
    if cases == "seeded":
        assert excluded <= 1e-3 and differ == 0
