"""No-GPU check of the f32 DEFINITION of Pendulum-v1 (include/mgym.h, restated word for word in tests/pendulum_ref.py) against gymnasium's float64
step (pendulum_ref.step_f64), one step from identical f32 inputs.

The bounds come from half-ulp rounding of each operation at these magnitudes (|th| <= 4 pi + 0.4 < 16: ulp 2^-20; |thdot| <= 8; reward magnitude
< 32: ulp 2^-19; PI_F - pi = 8.7e-8, TWO_PI_F - 2 pi = 1.7e-7 over at most two wraps) with roughly 2-5x headroom — they are not fitted to what
the code gives.  The reward is continuous across the wrap at an = +-pi, so an f32 angle that wraps where the f64 one does not stays inside its bound."""
import math

import numpy as np

import pendulum_ref as R

F = np.float32
BOUND_THDOT, BOUND_TH, BOUND_TRIG, BOUND_REWARD = 2e-6, 4e-6, 5e-6, 5e-5


def grid():
    rng = np.random.default_rng(5)
    th = list(np.linspace(-4 * math.pi, 4 * math.pi, 97)) + list(rng.uniform(-4 * math.pi, 4 * math.pi, 200))
    for k in (-3, -1, 1, 3):   # within 1e-6 of the odd multiples of pi, both sides, and the nearest floats themselves
        for d in (-1e-6, -3e-7, 0.0, 3e-7, 1e-6):
            th.append(k * math.pi + d)
        c = F(k * math.pi)
        th += [float(np.nextafter(c, F(100))), float(np.nextafter(c, F(-100)))]
    th += [0.0, -0.0, 1e-7, -1e-7]
    thdot = [-8.0, -7.999999, -1.0, -1e-3, 0.0, 1e-3, 0.37, 1.0, 7.999999, 8.0] + list(rng.uniform(-8, 8, 6))
    a = [-2.5, -2.0000002, -2.0, -1.9999999, -0.5, 0.0, 0.3, 1.9999999, 2.0, 2.0000002, 2.5] + list(rng.uniform(-2.5, 2.5, 4))
    T, D, A = np.meshgrid(np.array(th, F), np.array(thdot, F), np.array(a, F), indexing="ij")
    return T.ravel(), D.ravel(), A.ravel()


def test_one_f32_step_stays_within_rounding_of_the_float64_step():
    th, thdot, a = grid()
    assert th.size > 50000 and th.min() >= F(-4 * math.pi) and th.max() <= F(4 * math.pi)
    for g in (0.0, 9.81, 10.0):
        th2, thdot2, reward, nan = R.step_words(th, thdot, a, F(1.5) * F(g))
        assert not nan.any()
        cs, sn = R.cosf(th2), R.sinf(th2)
        exp = np.array([R.step_f64(float(t), float(d), float(u), float(F(g))) for t, d, u in zip(th, thdot, a)])
        worst = {k: float(np.max(np.abs(v.astype(np.float64) - exp[:, i]))) for i, (k, v) in enumerate((("th", th2), ("thdot", thdot2), ("cos", cs), ("sin", sn), ("reward", reward)))}
        print(f"g = {g}: worst |f32 - f64| {worst}")
        assert worst["thdot"] <= BOUND_THDOT and worst["th"] <= BOUND_TH and worst["cos"] <= BOUND_TRIG and worst["sin"] <= BOUND_TRIG, (g, worst)
        assert worst["reward"] <= BOUND_REWARD, (g, worst)
        assert reward.max() <= 0.0 and reward.min() >= R.REWARD_MIN - 1e-4, (g, float(reward.min()), float(reward.max()))
        # both clamp edges really occur: the torque beyond +-2 and the speed at +-8
        assert (np.abs(thdot2) == F(8)).any() and (np.abs(a) > F(2)).any()


def test_the_wrap_is_taken_on_either_side_of_an_odd_multiple_of_pi():
    """the angle cost just below and just above pi differs by less than the bound although `an` jumps from +pi to -pi"""
    c = F(math.pi)
    below, above = np.nextafter(c, F(0)), np.nextafter(c, F(4))
    th = np.array([below, c, above], F)
    _, _, reward, _ = R.step_words(th, np.zeros(3, F), np.zeros(3, F), F(15))
    assert np.all(np.abs(reward.astype(np.float64) + math.pi ** 2) <= BOUND_REWARD), reward
