"""Populations and action tables for the contact rules of tests/ll_contact_ref.py, shared by tests/test_ll_contact_oracle.py and
tests/test_gpu_ll_contact.py.

Two populations, 608 environments together (no multiple of 64):
  "det":    288 environments after reset_deterministic(), set_state spreading x over the helipad, both slopes and the two end
            chunks, tilting some and pushing some outwards;
  "seeded": 320 environments after a seeded reset() with wind on, env ids from ENV_ID_BASE.
The controllers are closed-loop, so the tables are produced by stepping the CPU oracle once per process: the actions are inputs,
not expectations.  T = 400 steps; an environment is checked up to and including its first ending.

coverage() asserts what the oracle's trajectories must contain, on those trajectories alone and excluding nothing, and that no
rule of the reference declines more than BAND_CAP of the checked case-steps."""
import functools
import os
import sys

import numpy as np

import ll_contact_ref as R

T = 400
N_DET, N_SEEDED = 288, 320
SEED, ENV_ID_BASE = 20251, 100_003
DET_CLASSES = ("gentle", "free_fall", "random", "leave", "late_brake", "slope")          # 48 each
SEEDED_CLASSES = ("gentle", "free_fall", "random", "leave", "late_brake")                # 64 each
POPULATIONS = {"det": dict(n=N_DET, wind=False, classes=DET_CLASSES), "seeded": dict(n=N_SEEDED, wind=True, classes=SEEDED_CLASSES)}
assert (N_DET + N_SEEDED) % 64 != 0


def kinds(pop):
    p = POPULATIONS[pop]
    return np.arange(p["n"]) % len(p["classes"])


def handle_args(pop):
    """keyword arguments of the handle (the oracle's and the engine's constructors take the same)"""
    return dict(seed=SEED, env_id_base=ENV_ID_BASE, enable_wind=True) if pop == "seeded" else dict(seed=SEED)


def det_start(blob):
    """the blob after reset_deterministic() with the craft moved rigidly: x spread per class, some tilted, the "leave" class
    placed near the viewport's sides and pushed outwards"""
    n = blob.shape[1]
    rng = np.random.default_rng(11)
    k = kinds("det")
    name = np.array(DET_CLASSES)[k]
    q = np.arange(n) // len(DET_CLASSES)                                   # 0 .. 47 within a class
    x = np.full(n, 10.0)
    tilt = np.zeros(n)
    vx = np.zeros(n)
    x = np.where(name == "gentle", rng.uniform(8.6, 11.4, n), x)
    ends = np.where(q % 2 == 0, rng.uniform(0.9, 1.9, n), rng.uniform(18.1, 19.1, n))
    x = np.where(name == "free_fall", np.where(q < 24, ends, rng.uniform(2.5, 17.5, n)), x)
    tilt = np.where(name == "free_fall", np.where(q % 3 == 0, rng.uniform(-0.5, 0.5, n), 0.0), tilt)
    x = np.where(name == "random", rng.uniform(2.0, 18.0, n), x)
    side = np.where(q % 2 == 0, -1.0, 1.0)
    x = np.where(name == "leave", 10.0 + side * rng.uniform(6.5, 8.5, n), x)
    vx = np.where(name == "leave", side * rng.uniform(3.0, 6.0, n), vx)
    x = np.where(name == "late_brake", rng.uniform(3.0, 17.0, n), x)
    tilt = np.where(name == "late_brake", np.where(q % 4 == 0, rng.uniform(-0.2, 0.2, n), 0.0), tilt)
    x = np.where(name == "slope", np.where(q % 2 == 0, rng.uniform(5.2, 7.6, n), rng.uniform(12.4, 14.8, n)), x)
    s = blob.astype(np.float64)
    cx, cy = s[0].copy(), s[1].copy()
    c, sn = np.cos(tilt), np.sin(tilt)
    for b in range(3):
        r = 6 * b
        dx, dy = s[r] - cx, s[r + 1] - cy
        s[r], s[r + 1] = x + c * dx - sn * dy, cy + sn * dx + c * dy
        s[r + 2] += tilt
        s[r + 3] += vx
    out = blob.copy()
    out[:18] = s[:18].astype(np.float32)
    return out


def controller(pop, t, blob, obs, rng, targets):
    """the action of every environment at step t from its blob and last observation"""
    p = POPULATIONS[pop]
    n = p["n"]
    name = np.array(p["classes"])[kinds(pop)]
    x, y, ang, vx, vy, w = (blob[k].astype(np.float64) for k in range(6))
    legs = (blob[18] + blob[19]) > 0
    a = np.zeros(n, np.uint32)
    # descent-rate controller: level the craft with the side engines, brake with the main engine below the target rate
    tilted = (np.abs(ang) > 0.05) | (np.abs(w) > 0.3)
    level = np.where(ang + 0.5 * w > 0, 3, 1)
    rate = np.where(tilted, level, np.where((vy < targets) & ~legs, 2, 0))
    # gymnasium's published heuristic (lunar_lander.py, heuristic()), for the seeded population: it also kills the drift
    o = obs.astype(np.float64)
    angle_targ = np.clip(o[0] * 0.5 + o[2] * 1.0, -0.4, 0.4)
    hover_targ = 0.55 * np.abs(o[0])
    angle_todo = (angle_targ - o[4]) * 0.5 - o[5] * 1.0
    hover_todo = (hover_targ - o[1]) * 0.5 - o[3] * 0.5
    angle_todo = np.where(legs, 0.0, angle_todo)
    hover_todo = np.where(legs, -o[3] * 0.5, hover_todo)
    heur = np.where((hover_todo > np.abs(angle_todo)) & (hover_todo > 0.05), 2, np.where(angle_todo < -0.05, 3, np.where(angle_todo > 0.05, 1, 0)))
    a = np.where(name == "gentle", heur if pop == "seeded" else rate, a)
    a = np.where(name == "slope", rate, a)
    a = np.where(name == "random", rng.integers(0, 4, n), a)
    # leave the viewport: det pushes with the side engine only; seeded leans outwards and holds its height with the main engine
    out_dir = np.where(x >= 10.0, 1.0, -1.0) if pop == "det" else np.where(np.arange(n) // len(p["classes"]) % 2 == 0, -1.0, 1.0)
    lean = -0.6 * out_dir                                  # leaning right (negative angle) pushes towards +x
    lean_todo = (lean - ang) * 0.5 - w * 0.5
    away = np.where(lean_todo < -0.05, 3, np.where(lean_todo > 0.05, 1, np.where(vy < 0.0, 2, 0)))
    away = np.where((np.arange(n) // len(p["classes"]) % 4 == 3), np.where(out_dir > 0, 1, 3), away)     # a quarter: side thrust only
    a = np.where(name == "leave", np.where(out_dir > 0, 1, 3) if pop == "det" else away, a)
    a = np.where(name == "late_brake", np.where((y < targets) & ~legs, np.where(tilted & (t % 2 == 0), level, 2), 0), a)
    return a.astype(np.uint32)


def _targets(pop):
    p = POPULATIONS[pop]
    n = p["n"]
    name = np.array(p["classes"])[kinds(pop)]
    q = np.arange(n) // len(p["classes"])
    per = n // len(p["classes"])
    t = np.full(n, -1.0)
    t = np.where(name == "gentle", -0.6 - 1.0 * q / (per - 1), t)          # descent rates -0.6 .. -1.6
    t = np.where(name == "slope", -0.5 - 0.6 * q / (per - 1), t)
    t = np.where(name == "late_brake", 4.6 + 2.4 * q / (per - 1), t)      # height at which the braking starts
    return t


def start(pop, env):
    """brings a fresh handle (oracle or engine) to the population's start and returns its first observation"""
    if pop == "det":
        env.reset_deterministic()
        s = det_start(np.array(env.get_state()))
        env.set_state(s)
        o, _ = R.observation(s)
        return np.concatenate([o, s[18:20].astype(np.float64)]).astype(np.float32)
    return np.array(env.reset())


def terrain_of(pop, blob):
    """the terrain of every environment's current episode, from the blob's episode column alone"""
    n = blob.shape[1]
    if pop == "det":
        return R.terrain(R.deterministic_heights(n))
    ep = blob[26].view(np.uint32).astype(np.int64) - 1
    return R.terrain(R.seeded_heights(SEED, ENV_ID_BASE + np.arange(n), ep))


@functools.lru_cache(None)
def build(pop):
    """steps the oracle through the population's T steps -> dict of read-only arrays: actions [T, n], blobs [T + 1, 27, n] (blobs[t]
    before step t), obs [T, 8, n], reward, done, trunc, alive [T, n]"""
    from oracle import oracle as ora
    p = POPULATIONS[pop]
    n = p["n"]
    ref = ora.OracleVec(ora.LUNARLANDER, n, **handle_args(pop))
    obs = start(pop, ref)
    rng = np.random.default_rng(5)
    targets = _targets(pop)
    out = dict(actions=[], blobs=[np.array(ref.get_state())], obs=[], reward=[], done=[], trunc=[])
    for t in range(T):
        a = controller(pop, t, out["blobs"][-1], obs, rng, targets)
        o, r, d, tr = (np.array(v) for v in ref.step(a, nthreads=8))
        obs = o
        out["actions"].append(a), out["obs"].append(o), out["reward"].append(r), out["done"].append(d), out["trunc"].append(tr)
        out["blobs"].append(np.array(ref.get_state()))
    res = {k: np.array(v) for k, v in out.items()}
    ended_before = np.cumsum(res["done"].astype(int), 0) - res["done"].astype(int) > 0
    res["alive"] = ~ended_before
    for v in res.values():
        v.setflags(write=False)
    return res


def run_rules(pop, traj, delta=None, **bounds):
    """the reference's rules over a trajectory of the population (the oracle's or the engine's) up to each first ending
    -> (violations {rule: [T, n]}, bands {rule: [T, n]}, figures)"""
    delta = R.DELTA if delta is None else delta
    alive, blobs = traj["alive"], traj["blobs"]
    tt, ii = np.nonzero(alive)
    cx, sy = terrain_of(pop, np.ascontiguousarray(blobs[0]))
    # every pose once: blobs[t] is the pre pose of step t, the post pose of step t - 1 and the one before step t + 1
    need = np.zeros((T + 1, alive.shape[1]), bool)
    need[:-1] |= alive
    need[1:] |= alive
    nt, ni = np.nonzero(need)
    slot = np.zeros(need.shape, int)
    slot[nt, ni] = np.arange(len(nt))
    geo = R.geometry(np.ascontiguousarray(blobs[nt, :, ni].T), (cx, sy[ni]))
    tq = np.maximum(tt - 1, 0)
    cut = lambda t: np.ascontiguousarray(blobs[t, :, ii].T)
    v, b, fig = R.check(cut(tt), cut(tt + 1), traj["actions"][tt, ii], np.ascontiguousarray(traj["obs"][tt, :, ii].T), traj["reward"][tt, ii],
                        traj["done"][tt, ii], traj["trunc"][tt, ii], POPULATIONS[pop]["wind"], (cx, sy[ii]), prev=cut(tq), has_prev=tt > 0,
                        geo=(R.take(geo, slot[tq, ii]), R.take(geo, slot[tt, ii]), R.take(geo, slot[tt + 1, ii])), delta=delta, **bounds)

    def full(x, fill=0):
        o = np.full(x.shape[:-1] + alive.shape, fill, x.dtype)
        o[..., tt, ii] = x
        return o
    viol, band = {k: full(x) for k, x in v.items()}, {k: full(x) for k, x in b.items()}
    leg_dist = full(fig["dpost"][1:], np.inf).transpose(1, 0, 2)
    viol["R6"], run = R.check_sleep(blobs[1:], traj["reward"], traj["done"], alive, leg_dist=leg_dist, delta=delta)
    band["R6"] = np.zeros(alive.shape, bool)
    # After the first ending the handle steps on (no auto-reset), and what is a function of one step alone still holds there: R1, R3,
    # R7 and R2's endings.  Only there can an environment be lost AND asleep (a wreck that has come to rest), the case that tells
    # -100 before +100.  R2's bound on the shaping's reward is not applied there: a craft that left the viewport falls without end
    # (y = -160, shaping -4000 after 250 steps), where one spacing of f32 exceeds the bound measured on episodes.
    at, ai = np.nonzero(~alive)
    va, _, _ = R.check(np.ascontiguousarray(blobs[at, :, ai].T), np.ascontiguousarray(blobs[at + 1, :, ai].T), traj["actions"][at, ai],
                       np.ascontiguousarray(traj["obs"][at, :, ai].T), traj["reward"][at, ai], traj["done"][at, ai], traj["trunc"][at, ai],
                       POPULATIONS[pop]["wind"], None, contact_rules=False, bound_reward=np.inf)
    for r in ("R1", "R2", "R3", "R7"):
        viol["after " + r] = np.zeros(alive.shape, bool)
        viol["after " + r][at, ai] = va[r]
        band["after " + r] = np.zeros(alive.shape, bool)
    fig = {k: x for k, x in fig.items()}
    fig.update(tt=tt, ii=ii, run=run)
    return viol, band, fig


@functools.lru_cache(None)
def oracle_rules(pop):
    """run_rules over the oracle's own trajectory, once per process"""
    return run_rules(pop, build(pop))


def report(pop, traj, viol, band, fig, limit=6):
    """the lines of an assertion message: per rule, the first violations outside its band"""
    lines = []
    for r in sorted(viol):
        bad = viol[r] & ~band[r] & (~traj["alive"] if r.startswith("after") else traj["alive"])
        if bad.any():
            at = np.argwhere(bad)[:limit]
            lines.append(f"{pop} {r}: {int(bad.sum())} violations, first (step, env): {at.tolist()}")
    return lines


@functools.lru_cache(None)
def coverage(pop=None):
    """what the oracle's trajectories of both populations contain, and the share of case-steps each rule declines"""
    c = dict(asleep=0, crash=0, out_of_bounds=0, only_leg0=0, only_leg1=0, bounce=0, gate=0, end_chunk0=0, end_chunk9=0, steps=0, legs_apart=0, lost_and_asleep=0)
    bands = {}
    for pop in POPULATIONS:
        tr = build(pop)
        al, post = tr["alive"], tr["blobs"][1:]
        end = al & tr["done"].astype(bool)
        go = post[:, 20] > 0.5
        oob = np.abs(tr["obs"][:, 0]) >= 1.0
        c["asleep"] += int((end & (tr["reward"] == 100.0)).sum())
        c["crash"] += int((end & go).sum())
        c["out_of_bounds"] += int((end & oob & ~go).sum())
        f0, f1 = post[:, 18] > 0.5, post[:, 19] > 0.5
        c["only_leg0"] += int((al & f0 & ~f1).sum())
        c["only_leg1"] += int((al & f1 & ~f0).sum())
        pre = tr["blobs"][:-1]
        c["bounce"] += int((al & (((pre[:, 18] > 0.5) & ~f0) | ((pre[:, 19] > 0.5) & ~f1))).sum())
        if POPULATIONS[pop]["wind"]:
            c["gate"] += int((al & ((pre[:, 18] > 0.5) | (pre[:, 19] > 0.5))).sum())
        x = post[:, 0]
        c["end_chunk0"] += int((end & go & (x >= 0.0) & (x < 2.0)).sum())
        c["end_chunk9"] += int((end & go & (x >= 18.0) & (x <= 20.0)).sum())
        c["steps"] += int(al.sum())
        c["lost_and_asleep"] += int((~al & go & ~(post[:, 21] > 0.5)).sum())
        viol, band, fig = oracle_rules(pop)
        # the body-to-flag mapping of R5: steps with the two legs on different sides of RADIUS, outside the band
        d1, d2 = fig["dpre"][1], fig["dpre"][2]
        c["legs_apart"] += int((((d1 <= R.RADIUS - R.DELTA) & (d2 >= R.RADIUS + R.DELTA)) | ((d2 <= R.RADIUS - R.DELTA) & (d1 >= R.RADIUS + R.DELTA))).sum())
        for r, b in band.items():
            bands[r] = bands.get(r, 0) + int((b & al).sum())
        bands = {r: b for r, b in bands.items() if not r.startswith("after")}
    need = dict(asleep=32, crash=32, out_of_bounds=32, only_leg0=32, only_leg1=32, bounce=32, gate=32, end_chunk0=8, end_chunk9=8, legs_apart=32, lost_and_asleep=32)
    short = {k: (c[k], v) for k, v in need.items() if c[k] < v}
    assert not short, f"coverage (have, need): {short}; all: {c}"
    share = {r: b / c["steps"] for r, b in bands.items()}
    assert max(share.values()) <= R.BAND_CAP, f"a rule declines more than {R.BAND_CAP:.0%} of the case-steps: {share}"
    return c, share


def _measure():
    """prints the figures behind ll_contact_ref's MEASURED_* constants: the CPU oracle against the reference"""
    worst_r, worst_sink = 0.0, 0.0
    for pop in POPULATIONS:
        tr = build(pop)
        viol, band, fig = run_rules(pop, tr, bound_reward=np.inf, bound_sink=np.inf)
        worst_r = max(worst_r, float(fig["reward_err"].max()))
        worst_sink = max(worst_sink, float(-fig["low_pre"].min()))
        print(pop, "lowest vertex per body (hull, leg 0, leg 1):", fig["low_pre"].min(1), "worst reward error", fig["reward_err"].max())
        for r in sorted(viol):
            bad = viol[r] & (~tr["alive"] if r.startswith("after") else tr["alive"])
            print(f"  {r}: {int(bad.sum())} violations, {int((bad & ~band[r]).sum())} outside the band; band holds {int((band[r] & tr['alive']).sum())} of {int(tr['alive'].sum())}")
        # delta: the leg-flag exceptions by distance from RADIUS
        for delta in (0.0005, 0.001, 0.0015, 0.002, 0.0025):
            v, b, _ = run_rules(pop, tr, delta=delta, bound_reward=np.inf, bound_sink=np.inf)
            print(f"  delta {delta}: R4 {int((v['R4'] & ~b['R4'] & tr['alive']).sum())} R5 {int((v['R5'] & ~b['R5'] & tr['alive']).sum())} outside the band")
        print("  R6 longest still run without an ending:", int(np.where(tr["alive"] & ~tr["done"].astype(bool), fig["run"], 0).max()))
    print(f"MEASURED_REWARD = {worst_r:.3e}\nMEASURED_SINK = {worst_sink:.4f}")
    try:
        print("coverage:", coverage())
    except AssertionError as e:
        print("coverage FAILS:", e)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if "--measure" in sys.argv:
        _measure()
