"""Airborne LunarLander cases for the float64 step reference (tests/ll_flight_ref.py): 4 096 seeded states plus hand-built
classes at the solver's edges, T = 12 steps with all four actions drawn per step, and the reference's trajectories of them,
computed once per parameter set and shared by tests/test_ll_flight_oracle.py and tests/test_gpu_ll_flight.py.

Asserted here, with the reference alone and without excluding a case: every activity flag of the reference is set in at least 32
case-steps (the three clamps in at least 8 each), and every case stays airborne (lowest polygon vertex >= 7.0, above every
possible terrain vertex of 6.6 and the fat AABBs) over the whole trajectory, at every parameter set."""
import copy
import functools

import numpy as np

import ll_flight_ref as R

T = 12
N_SEEDED = 4096
PER_CLASS = 16
CLASSES = ("seeded", "at_limits", "far_outside", "leg_spin_600", "fast_150", "angle_near_pi", "dispersion_corners", "spin_100")
CLAMP_CLASSES = ("leg_spin_600", "fast_150", "spin_100")
MIN_Y = 7.0

# (gravity, enable_wind, wind_power, turbulence_power); the last is near the builder's ends (gravity in (-12, 0), :292-296)
PARAMS = {"calm": (-10.0, False, 15.0, 1.5), "wind": (-10.0, True, 15.0, 1.5), "ends": (-11.9, True, 19.5, 1.95)}


def _assemble(rng, n, x, y, angle, lv, lw, joint, offset, rel_v, rel_w):
    """blob words 0..17 [18, n] float32: legs hung on the lander's origin by their anchors, origin displaced by `offset`"""
    b = np.zeros((18, n))
    b[0], b[1], b[2], b[3], b[4], b[5] = x, y, angle, lv[0], lv[1], lw
    for j in range(2):
        la = angle + joint[j]
        anchor = R.rot(la, R.ANCHOR_B[j])
        r = 6 * (1 + j)
        b[r], b[r + 1], b[r + 2] = x - anchor[:, 0] + offset[j][0], y - anchor[:, 1] + offset[j][1], la
        b[r + 3], b[r + 4], b[r + 5] = lv[0] + rel_v[j][0], lv[1] + rel_v[j][1], lw + rel_w[j]
    return b.astype(np.float32)


def _draw(rng, n, **over):
    u = lambda lo, hi: rng.uniform(lo, hi, n)
    d = dict(x=u(4.0, 16.0), y=u(10.5, 14.0), angle=u(-0.6, 0.6), lv=[u(-3.0, 3.0), u(-3.0, 3.0)], lw=u(-1.5, 1.5),
             joint=[u(R.LOWER[j] - 0.3, R.UPPER[j] + 0.3) for j in range(2)], rel_w=[u(-2.0, 2.0) for _ in range(2)],
             rel_v=[[u(-0.3, 0.3), u(-0.3, 0.3)] for _ in range(2)])
    rad, phi = [u(0.0, 0.05) for _ in range(2)], [u(0.0, 2 * np.pi) for _ in range(2)]
    d["offset"] = [[rad[j] * np.cos(phi[j]), rad[j] * np.sin(phi[j])] for j in range(2)]
    d.update(over)
    return _assemble(rng, n, **d)


@functools.lru_cache(None)
def cases():
    """-> blob [18, n] f32, actions [T, n] u32, dispersion [2, n] f32, kind [n] (index into CLASSES); n is no multiple of 64"""
    rng = np.random.default_rng(20250)
    m = PER_CLASS
    u = lambda lo, hi: rng.uniform(lo, hi, m)
    pm = lambda: rng.choice([-1.0, 1.0], m)
    blobs = [_draw(rng, N_SEEDED)]
    # legs exactly at each limit (as exactly as f32 angles allow): both lower, both upper, mixed
    at = [np.where(np.arange(m) % 2 == 0, R.LOWER[0], R.UPPER[0]), np.where(np.arange(m) // 2 % 2 == 0, R.LOWER[1], R.UPPER[1])]
    blobs.append(_draw(rng, m, joint=at, angle=np.zeros(m)))
    # both legs far outside: past slop + 8 degrees, up to 1.2 rad
    s0, s1 = pm(), pm()
    far = [np.where(s0 < 0, R.LOWER[0] - u(0.4, 1.2), R.UPPER[0] + u(0.4, 1.2)), np.where(s1 < 0, R.LOWER[1] - u(0.4, 1.2), R.UPPER[1] + u(0.4, 1.2))]
    blobs.append(_draw(rng, m, joint=far))
    # a leg at +-600 rad/s relative to the lander
    blobs.append(_draw(rng, m, rel_w=[pm() * 600.0 * (np.arange(m) % 3 != 1), pm() * 600.0 * (np.arange(m) % 3 != 0)]))
    # 150 m/s: along +-x it leaves the viewport (done, reward -100), upwards and diagonally up it only hits the clamp
    th = np.where(np.arange(m) % 4 == 0, 0.0, np.where(np.arange(m) % 4 == 1, np.pi, np.where(np.arange(m) % 4 == 2, 0.5 * np.pi, 0.25 * np.pi)))
    x0 = np.where(np.arange(m) % 4 == 0, u(14.6, 15.4), np.where(np.arange(m) % 4 == 1, u(4.6, 5.4), u(8.0, 12.0)))
    blobs.append(_draw(rng, m, x=x0, lv=[150.0 * np.cos(th), 150.0 * np.sin(th)]))
    # lander angle near +-pi
    blobs.append(_draw(rng, m, angle=pm() * (np.pi - u(-0.05, 0.05))))
    # side engines both ways (the actions below) with the dispersion at its corners
    blobs.append(_draw(rng, m))
    # the whole craft spinning at +-100 rad/s: h w = 2 > pi / 2 on all three bodies
    sp = pm() * u(90.0, 120.0)
    blobs.append(_draw(rng, m, lw=sp, lv=[u(-1.0, 1.0), u(0.0, 2.0)], rel_w=[np.zeros(m)] * 2, rel_v=[[np.zeros(m)] * 2] * 2))
    blob = np.concatenate(blobs, 1)
    kind = np.concatenate([np.full(b.shape[1], k) for k, b in enumerate(blobs)])
    n = blob.shape[1]
    assert n % 64 != 0 and len(blobs) == len(CLASSES)
    actions = rng.integers(0, 4, (T, n)).astype(np.uint32)
    disp = rng.uniform(-1.0, 1.0, (2, n)).astype(np.float32)
    k = kind == CLASSES.index("dispersion_corners")
    actions[:, k] = np.where(np.arange(m) % 2 == 0, 1, 3)[None, :]
    actions[1::3, k] = 2
    disp[:, k] = np.stack([np.where(np.arange(m) // 2 % 2 == 0, -1.0, 1.0), np.where(np.arange(m) // 4 % 2 == 0, -1.0, 1.0)])
    for a in (blob, actions, disp, kind):
        a.setflags(write=False)
    return blob, actions, disp, kind


def clamp_mask():
    kind = cases()[3]
    return np.isin(kind, [CLASSES.index(c) for c in CLAMP_CLASSES])


@functools.lru_cache(None)
def trajectory(name):
    """The reference's T steps of every case at PARAMS[name] -> dict of read-only arrays: words [T, 18, n], obs [T, 8, n],
    reward [T, n], done [T, n], flags {name: [T, n]}, lowest [T + 1, n].  Asserts the module's two conditions."""
    blob, actions, _, kind = cases()
    g, wind, wp, tp = PARAMS[name]
    ref = R.FlightRef(blob, gravity=g, enable_wind=wind, wind_power=wp, turbulence_power=tp)
    out = dict(words=[], obs=[], reward=[], done=[], lowest=[ref.lowest_y], flags={k: [] for k in R.FLAGS})
    for t in range(T):
        obs, rew, done = ref.step(actions[t])
        out["words"].append(ref.words()), out["obs"].append(obs), out["reward"].append(rew), out["done"].append(done)
        out["lowest"].append(ref.lowest_y)
        for k in R.FLAGS:
            out["flags"][k].append(ref.flags[k])
    res = {k: np.array(v) for k, v in out.items() if k != "flags"}
    res["flags"] = {k: np.array(v) for k, v in out["flags"].items()}
    for a in list(res["flags"].values()) + [v for k, v in res.items() if k != "flags"]:
        a.setflags(write=False)
    counts = {k: int(v.sum()) for k, v in res["flags"].items()}
    for k, c in counts.items():
        need = 8 if k in ("angular_clamp", "translation_clamp", "rotation_clamp") else 32
        assert c >= need, f"{name}: activity flag {k} set in {c} case-steps, need {need}: {counts}"
    assert res["lowest"].min() >= MIN_Y, f"{name}: case {np.argmin(res['lowest'].min(0))} comes down to {res['lowest'].min()}"
    fast_x = (kind == CLASSES.index("fast_150")) & (np.abs(blob[3]) > 100.0)
    assert res["done"][-1][fast_x].all() and (res["reward"][-1][fast_x] == -100.0).all() and fast_x.sum() >= 8
    res["counts"] = counts
    return res


def group_errors(words, obs, reward, t, traj, mask):
    """worst absolute deviation per group of R.GROUPS at step t over the cases of mask"""
    dw = np.abs(words[:18].astype(np.float64) - traj["words"][t])[:, mask]
    pose, vel = [0, 1, 2], [3, 4, 5]
    leg_pose, leg_vel = [6, 7, 8, 12, 13, 14], [9, 10, 11, 15, 16, 17]
    return dict(lander_pose=dw[pose].max(), lander_vel=dw[vel].max(), leg_pose=dw[leg_pose].max(), leg_vel=dw[leg_vel].max(),
                obs=np.abs(obs.astype(np.float64) - traj["obs"][t])[:, mask].max(),
                reward=np.abs(reward.astype(np.float64) - traj["reward"][t])[mask].max())


def start_blob(env):
    """the handle's own blob after reset_deterministic() with the cases' 18 pose / velocity words in place"""
    s = env.get_state().copy()
    s[:18] = cases()[0]
    return s


def check_against_reference(env, name, what, measure=None, rollout=False):
    """(a): env (oracle or engine, freshly built for PARAMS[name] with n = the number of cases) does reset_deterministic(),
    set_state(cases) and T steps; every word, the observation, the reward and the flags against the reference after every step.
    rollout: one env.rollout(actions) call; the blob is then compared at the end only.  Returns the per-step outputs."""
    blob, actions, _, _ = cases()
    traj = trajectory(name)
    clamp = clamp_mask()
    env.reset_deterministic()
    env.set_state(start_blob(env))
    outs, fails = [], []
    if rollout:
        ro = env.rollout(actions)
    for t in range(T):
        obs, rew, done, trunc = [x[t] for x in ro] if rollout else env.step(actions[t])
        state = env.get_state() if (not rollout or t == T - 1) else None
        outs.append((np.array(obs), np.array(rew), np.array(done), np.array(trunc), state))
        assert np.array_equal(done.astype(bool), traj["done"][t]), f"{what} step {t}: done differs at {np.nonzero(done.astype(bool) != traj['done'][t])[0][:5]}"
        assert not trunc.any() and (obs[6:8] == 0).all(), f"{what} step {t}: truncated or leg flags set"
        if state is not None:
            assert (state[18:21] == 0).all() and (state[21] == 1).all(), f"{what} step {t}: leg / game-over / awake flags"
        w = state if state is not None else traj["words"][t]       # (nothing to compare inside a rollout)
        for mask, bound, store in ((~clamp, R.BOUND, "MEASURED"), (clamp, R.BOUND_CLAMP, "MEASURED_CLAMP")):
            err = group_errors(w, obs, rew, t, traj, mask)
            if measure is not None:
                for k, e in err.items():
                    measure[store][k] = max(measure[store][k], float(e))
            fails += [f"{what} step {t} {store[9:] or 'main'} {k}: {e:.3g} > {bound[k]:.3g}" for k, e in err.items() if not e <= bound[k]]
    assert measure is not None or not fails, "\n".join(fails[:12])
    return outs


def reset_pose(n):
    """blob words of reset() before its implicit step: lander at (W / 2, H), legs beside it at angle 0.05 i, all at rest
    (lunar_lander.rs:816-824, :868-869)"""
    f = np.float32
    x, y = R.VIEWPORT_W / R.SCALE / f(2.0), R.VIEWPORT_H / R.SCALE
    b = np.zeros((18, n), np.float32)
    b[0], b[1] = x, y
    for j, i in enumerate(R.SIGN):
        b[6 * (1 + j)], b[6 * (1 + j) + 1], b[6 * (1 + j) + 2] = x - f(i) * R.LEG_AWAY / R.SCALE, y, f(i) * f(0.05)
    return b


_AFTER_RESET = {}


def reference_after_reset(post, name):
    """The reference taken through reset()'s own first step (:845-849, :911), so that its joints hold the impulses the handle's
    joints hold: 180 sweeps do not forget a warm start (lander-to-leg mass ratio 68), and with other impulses the position sweeps
    would end at other counts than the handle's.  post: the handle's blob after reset().  The random force of reset() is not
    exported; it follows from the blob, the joints' impulses being internal: sum m v = h (F + M g + wind).
    -> (reference, worst deviation of its 18 words from post per group of R.GROUPS[:4])"""
    key = (name, post[:25].tobytes())
    if key not in _AFTER_RESET:
        g, wind, wp, tp = PARAMS[name]
        n = post.shape[1]
        wi, ti = post[23].view(np.int32).astype(np.int64), post[24].view(np.int32).astype(np.int64)
        r = R.FlightRef(reset_pose(n), gravity=g, enable_wind=wind, wind_power=wp, turbulence_power=tp, deterministic=False,
                        wind_idx=wi - wind, torque_idx=ti - wind)
        pw = post[:18].astype(np.float64)
        momentum = sum(R.MASS[k] * pw[6 * k + 3:6 * k + 5] for k in range(3)).T
        push = momentum / R.H - np.array([0.0, R.MASS.sum() * r.gravity])
        if wind:
            push[:, 0] -= r._gust(wi - 1) * r.wind_power
        assert np.abs(push).max() <= 1000.0 * (1 + 1e-5)          # INITIAL_RANDOM, :37
        r.step(np.zeros(n, np.int64), push=push)
        assert r.pos_sweeps.max() < R.POS_ITERS
        d = np.abs(r.words() - pw)
        err = dict(lander_pose=d[[0, 1, 2]].max(), lander_vel=d[[3, 4, 5]].max(), leg_pose=d[[6, 7, 8, 12, 13, 14]].max(),
                   leg_vel=d[[9, 10, 11, 15, 16, 17]].max())
        _AFTER_RESET[key] = (r, err)
    r, err = _AFTER_RESET[key]
    return copy.deepcopy(r), err


def check_dispersion_differential(make_env, what, measure=None):
    """(b): two seed-identical handles, wind on; both reset() and take the same set_state; one steps with the cases' dispersion
    override, the other with an override of zeros, one step with actions 1..3.  (first - second) over the 18 words against the
    reference's difference from the same imported state, wind_idx / torque_idx read from the exported blob.

    Two things the issue's protocol did not have.  The reference first takes reset()'s own step (reference_after_reset) instead
    of starting with zero impulses.  And where one of its "position sweeps solved" decisions comes within f32 rounding of the
    slop, it gives the outcome of either decision (FlightRef.step's exit_bias): one sweep more or less moves a leg by 1.7e-4, and
    no f32 implementation can be held to the float64 side of such a decision.  Every case is compared, with the nearest of the
    reference's admissible differences.  On top of the differential, both handles' words are held to the bounds of (a), which
    pins the dispersion, reset()'s step and the warm start absolutely."""
    blob, _, disp, _ = cases()
    n = blob.shape[1]
    clamp = clamp_mask()
    a, b = make_env(), make_env()
    a.reset(), b.reset()
    post = a.get_state().copy()
    assert np.array_equal(post.view(np.uint32), b.get_state().view(np.uint32))
    ref, reset_err = reference_after_reset(post, "wind")
    s = post.copy()
    s[:18] = blob
    s[18:20] = 0.0
    a.set_state(s), b.set_state(s)
    a.set_dispersion(disp), b.set_dispersion(np.zeros_like(disp))
    act = (1 + np.arange(n) % 3).astype(np.uint32)
    a.step(act), b.step(act)
    sa, sb = a.get_state(), b.get_state()
    got = sa[:18].astype(np.float64) - sb[:18].astype(np.float64)
    ref.set_words(blob)
    outs = {}
    for which, d in (("a", disp), ("b", np.zeros_like(disp))):
        for bias in (0, -1, 1):
            r = copy.deepcopy(ref)
            r.step(act, d, exit_bias=bias)
            outs[which, bias] = r.words()
    exp = outs["a", 0] - outs["b", 0]
    assert np.abs(exp[3:6]).max() > 1e-3          # the dispersion does move the lander's velocities
    err = np.min([np.abs(got - (outs["a", i] - outs["b", j])).max(0) for i in (0, -1, 1) for j in (0, -1, 1)], 0)    # [n]
    fails = [f"{what} reset step {k}: {e:.3g} > {R.BOUND[k]:.3g}" for k, e in reset_err.items() if not e <= R.BOUND[k]]
    for mask, bound, bound_abs, store in ((~clamp, R.BOUND_DIFF, R.BOUND, "MEASURED_DIFF"), (clamp, R.BOUND_DIFF_CLAMP, R.BOUND_CLAMP, "MEASURED_DIFF_CLAMP")):
        e = float(err[mask].max())
        if measure is not None:
            measure[store] = max(measure[store], e)
        if not e <= bound:
            fails.append(f"{what} {store[9:]}: {e:.3g} > {bound:.3g} at case {np.nonzero(mask)[0][np.argmax(err[mask])]}")
        for which, st in (("a", sa), ("b", sb)):
            dw = np.min([np.abs(st[:18].astype(np.float64) - outs[which, i]) for i in (0, -1, 1)], 0)[:, mask]
            ab = dict(lander_pose=dw[[0, 1, 2]].max(), lander_vel=dw[[3, 4, 5]].max(), leg_pose=dw[[6, 7, 8, 12, 13, 14]].max(),
                      leg_vel=dw[[9, 10, 11, 15, 16, 17]].max())
            if measure is not None:
                print(f"(b) handle {which} {store[14:] or 'main'} absolute:", {k: f"{v:.2e}" for k, v in ab.items()})
            fails += [f"{what} handle {which} absolute {k}: {v:.3g} > {bound_abs[k]:.3g}" for k, v in ab.items() if not v <= bound_abs[k]]
    if measure is not None:
        print("(b) reset step:", {k: f"{v:.2e}" for k, v in reset_err.items()})
    assert measure is not None or not fails, "\n".join(fails)
    return post, sa, sb


def _measure():
    """prints the figures behind ll_flight_ref.MEASURED*: the CPU oracle against the reference, wind off and wind on"""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import oracle as ora
    n = cases()[0].shape[1]
    m = dict(MEASURED=dict.fromkeys(R.GROUPS, 0.0), MEASURED_CLAMP=dict.fromkeys(R.GROUPS, 0.0), MEASURED_DIFF=0.0, MEASURED_DIFF_CLAMP=0.0)
    for name in ("calm", "wind"):
        g, wind, wp, tp = PARAMS[name]
        check_against_reference(ora.OracleVec(ora.LUNARLANDER, n, gravity=g, enable_wind=wind, wind_power=wp, turbulence_power=tp), name, name, measure=m)
        print(name, "activity counts", trajectory(name)["counts"], "lowest vertex", trajectory(name)["lowest"].min())
    g, wind, wp, tp = PARAMS["wind"]
    check_dispersion_differential(lambda: ora.OracleVec(ora.LUNARLANDER, n, seed=7, gravity=g, enable_wind=wind, wind_power=wp, turbulence_power=tp), "oracle", measure=m)
    for k in ("MEASURED", "MEASURED_CLAMP"):
        print(k, "= dict(" + ", ".join(f"{g}={v:.2e}" for g, v in m[k].items()) + ")")
    print(f"MEASURED_DIFF = {m['MEASURED_DIFF']:.2e}\nMEASURED_DIFF_CLAMP = {m['MEASURED_DIFF_CLAMP']:.2e}")


if __name__ == "__main__":
    import sys
    if "--measure" in sys.argv:
        _measure()
