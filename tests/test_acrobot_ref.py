"""No-GPU check of the f32 DEFINITION of Acrobot-v1 (include/mgym.h, restated word for word in tests/acrobot_ref.py) against gymnasium's float64
step (acrobot_ref.step_f64), one step from identical f32 inputs.

Two bands: SLOW, |w1| <= 0.4 pi and |w2| <= 0.9 pi, where a policy lives (a tenth of the velocity box), and FULL, the whole velocity box
|w1| <= 4 pi, |w2| <= 9 pi, where the accelerations reach hundreds of rad/s^2 and one RK4 step amplifies an f32 rounding of a stage by dt * dF/dy.
The bounds are FOUR TIMES the worst per-component deviation the numpy restatement shows against step_f64 over this file's grid (DESIGN.md 5d records
the measured figures; the factor is for the one-ulp freedom between sinf implementations and for grid sampling) — measured from the restatement, not
from the kernels' header, which must equal the restatement exactly (tests/test_acrobot_host.py).  Angles are compared on the circle (an f32 angle
may wrap where the float64 one, a hair short of pi, does not).  `done` must agree wherever the float64 margin |-cos th1 - cos(th1 + th2) - 1|
exceeds MARGIN = 3 x the band's angle bound + 1e-6: the margin moves by at most 2 |d th1| + |d th2|, and its f32 evaluation from the
observation's words (five operations on values below 2, half an ulp of 2^-22 each, over trig words half an ulp of 2^-24 off) adds under 1e-6."""
import math

import numpy as np

import acrobot_ref as R

F = np.float32
PI = math.pi
# worst |f32 - f64| of the restatement over this grid (angles th1', th2'; velocities w1', w2'), measured once: see the docstring and DESIGN.md 5d
WORST = {"slow": (5.4e-7, 5.7e-7, 4.3e-7, 6.6e-7), "full": (1.13e-5, 1.39e-5, 1.22e-3, 3.03e-3)}
BOUND = {band: tuple(4.0 * v for v in w) for band, w in WORST.items()}


def circle(d):
    return np.abs((d + PI) % (2 * PI) - PI)


def random_states(band, count=20000, seed=11):
    rng = np.random.default_rng(seed + (band == "slow"))
    k = 0.1 if band == "slow" else 1.0
    return [rng.uniform(-PI, PI, count).astype(F), rng.uniform(-PI, PI, count).astype(F), rng.uniform(-4 * PI * k, 4 * PI * k, count).astype(F),
            rng.uniform(-9 * PI * k, 9 * PI * k, count).astype(F), rng.integers(0, 3, count).astype(np.uint32)]


def edge_states(band):
    """both wrap edges of both angles (the step carries the angle across +-pi, or lands within a few ulp of it) and both velocity clamps"""
    k = 0.1 if band == "slow" else 1.0
    rows = []
    near = [PI - d for d in (0.0, 1e-7, 3e-7, 1e-6, 1e-3, 0.05, 0.2)]
    for s in (1.0, -1.0):
        for x in near:
            for w in (0.0, 0.3, 1.0, -0.3):
                for a in (0, 1, 2):
                    rows.append((s * x, 0.3, s * w, -0.2, a))      # th1 at the edge
                    rows.append((0.4, s * x, 0.1, s * w, a))       # th2 at the edge
    if band == "full":
        for s in (1.0, -1.0):
            for th1 in (-2.0, -0.7, 0.0, 0.9, 2.5):
                for th2 in (-1.5, 0.0, 1.2):
                    for a in (0, 1, 2):
                        for v in (4 * PI, 4 * PI - 1e-3, 4 * PI - 0.3):
                            rows.append((th1, th2, s * v, 0.5, a))          # w1 at its clamp
                        for v in (9 * PI, 9 * PI - 1e-3, 9 * PI - 0.3):
                            rows.append((th1, th2, 0.5, s * v, a))          # w2 at its clamp
    r = np.array(rows, np.float64)
    st = [np.clip(r[:, 0], -PI, PI).astype(F), np.clip(r[:, 1], -PI, PI).astype(F), np.clip(r[:, 2], -4 * PI * k, 4 * PI * k).astype(F),
          np.clip(r[:, 3], -9 * PI * k, 9 * PI * k).astype(F), r[:, 4].astype(np.uint32)]
    return st


def surface_states(count=64, seed=21):
    """states whose NEXT state lies within a few ulp of the termination surface, on either side: th1 is bisected between a start that does not
    terminate and one that does (by the restatement's own flag) down to neighbouring floats, then -3 .. +3 ulp around the pair"""
    rng = np.random.default_rng(seed)
    th2 = rng.uniform(-0.5, 0.5, count).astype(F)
    w1, w2 = rng.uniform(-1.0, 1.0, count).astype(F), rng.uniform(-2.0, 2.0, count).astype(F)
    a = rng.integers(0, 3, count).astype(np.uint32)
    lo, hi = np.full(count, 1.0, F), np.full(count, 3.0, F)   # hanging-ish (tip below the bar) .. upright-ish (tip above it)
    done = lambda th1: R.step_words(th1, th2, w1, w2, a)[5].astype(bool)
    ok = ~done(lo) & done(hi)
    assert ok.sum() > count // 2
    for _ in range(40):
        mid = ((lo.astype(np.float64) + hi.astype(np.float64)) / 2).astype(F)
        d = done(mid)
        lo, hi = np.where(d, lo, mid).astype(F), np.where(d, mid, hi).astype(F)
    out = [[], [], [], [], []]
    for k in range(-3, 4):
        x = lo.copy()
        for _ in range(abs(k)):
            x = np.nextafter(x, F(10.0 if k > 0 else -10.0)).astype(F)
        for lst, v in zip(out, (x[ok], th2[ok], w1[ok], w2[ok], a[ok])):
            lst.append(v)
    return [np.concatenate(v) for v in out]


def deviations(st):
    th1, th2, w1, w2, a = st
    g = R.step_words(th1, th2, w1, w2, a)
    e = R.step_f64(*(v.astype(np.float64) for v in (th1, th2, w1, w2)), a)
    dev = [circle(g[0].astype(np.float64) - e[0]), circle(g[1].astype(np.float64) - e[1]), np.abs(g[2] - e[2]), np.abs(g[3] - e[3])]
    return g, e, dev


def check_band(band):
    st = [np.concatenate(v) for v in zip(random_states(band), edge_states(band))]
    g, e, dev = deviations(st)
    worst = tuple(float(d.max()) for d in dev)
    print(f"{band}: {st[0].size} states, worst |f32 - f64| th1' {worst[0]:.3g} th2' {worst[1]:.3g} w1' {worst[2]:.3g} w2' {worst[3]:.3g}; bounds {BOUND[band]}")
    assert not g[6].any() and all(np.isfinite(v).all() for v in g[:4])
    for k in range(4):
        assert worst[k] <= BOUND[band][k], (band, k, worst[k], BOUND[band][k])
    margin = 3.0 * max(BOUND[band][:2]) + 1e-6
    clear = np.abs(e[5]) > margin
    assert np.array_equal(g[5][clear].astype(bool), e[4][clear]) and clear.mean() > 0.99
    assert np.array_equal(g[4], np.where(g[5], F(0), F(-1)))   # the reward follows the flag
    return st, g, e


def test_slow_band_stays_within_rounding_of_the_float64_step():
    st, g, e = check_band("slow")
    assert (np.abs(st[2]) <= F(0.4 * PI)).all() and (np.abs(st[3]) <= F(0.9 * PI)).all()
    # the wrap really happened on both sides of both angles: the raw float64 sum left [-pi, pi]
    for k in (0, 1):
        moved = np.abs(g[k].astype(np.float64) - st[k]) > 5.0
        assert (moved & (st[k] > 0)).any() and (moved & (st[k] < 0)).any()


def test_full_velocity_box_stays_within_rounding_of_the_float64_step():
    st, g, e = check_band("full")
    assert (np.abs(g[2]) == R.V1).any() and (g[2] == -R.V1).any() and (g[3] == R.V2).any() and (g[3] == -R.V2).any()   # both clamps, both signs
    assert g[5].any() and e[4].any()   # terminating steps occur


def test_done_agrees_next_to_the_termination_surface_wherever_the_margin_is_clear():
    st = surface_states()
    g, e, dev = deviations(st)
    margin = 3.0 * max(BOUND["slow"][:2]) + 1e-6
    near = np.abs(e[5]) < 1e-5
    print(f"surface: {st[0].size} states, {int(near.sum())} with |float64 margin| < 1e-5, smallest {float(np.abs(e[5]).min()):.3g}; done on {int(g[5].sum())}")
    assert near.mean() > 0.9 and g[5].any() and not g[5].all()   # within a few ulp of the surface, on either side
    for k in range(4):
        assert float(dev[k].max()) <= BOUND["slow"][k]
    clear = np.abs(e[5]) > margin
    assert np.array_equal(g[5][clear].astype(bool), e[4][clear])
