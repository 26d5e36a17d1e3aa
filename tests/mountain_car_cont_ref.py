"""gymnasium's MountainCarContinuous-v0 step in float64, for tests/test_mountain_car_cont_ref.py.  No test here.

step_f64 is the text of gymnasium/envs/classic_control/continuous_mountain_car.py (Continuous_MountainCarEnv.step; gymnasium is not a dependency),
vectorised over numpy float64 arrays: power 0.0015, max_speed 0.07, positions in [-1.2, 0.6], goal_position 0.45."""
import numpy as np

MIN_ACTION, MAX_ACTION = -1.0, 1.0
MIN_POSITION, MAX_POSITION = -1.2, 0.6
MAX_SPEED, GOAL_POSITION, POWER = 0.07, 0.45, 0.0015


def step_f64(p, v, a, goal_velocity):
    """-> (p', v', terminated, reward) of one step from position p, velocity v under action a (unclipped), all float64 arrays"""
    p, v, a = (np.asarray(x, np.float64) for x in (p, v, a))
    force = np.minimum(np.maximum(a, MIN_ACTION), MAX_ACTION)
    v = v + (force * POWER - 0.0025 * np.cos(3 * p))
    v = np.where(v > MAX_SPEED, MAX_SPEED, v)
    v = np.where(v < -MAX_SPEED, -MAX_SPEED, v)
    p = p + v
    p = np.where(p > MAX_POSITION, MAX_POSITION, p)
    p = np.where(p < MIN_POSITION, MIN_POSITION, p)
    v = np.where((p == MIN_POSITION) & (v < 0), 0.0, v)
    terminated = (p >= GOAL_POSITION) & (v >= goal_velocity)
    reward = np.where(terminated, 100.0, 0.0) - np.power(a, 2) * 0.1
    return p, v, terminated, reward
