"""Edge-of-state-space cases for the classic families (CartPole, MountainCar, MountainCarContinuous, Pendulum, Acrobot), shared by
tests/test_classic_edge_cases.py (CPU), tests/test_mountain_car_cont_ref.py and tests/test_gpu_classic_edges.py.  numpy only; no test here.

One builder per family returns (state blob [state_cols, n] as uint32 words, actions [n]): a deterministic order, n <= 65 536 and a multiple of 1024
after padding with rest states.  Cases are products of per-column value lists with the FIRST column varying fastest, so that 64 consecutive
environments hold every angle class; where the full product is too large a seeded sample of it is taken and every pair of values from two different
columns is asserted present.  nb(v) is v and its two float32 neighbours; TINY is the denormals, the smallest normal and both zeros.

Every builder ends with assertions, on the reference alone (the restatements of tests/pendulum_ref.py and tests/acrobot_ref.py, the CPU oracle), that
what it exists for is present: each clamp on each side, each done / goal boundary on both sides and on the tie, denormal results, table-branch and
fast-branch lanes in one 64-env group, NaN results in the non-finite sets.  A grid that loses one of these fails here, on the CPU."""
import functools
import itertools
import math

import numpy as np

F = np.float32
PI_F, TWO_PI_F = F(3.14159274), F(6.28318548)
FLT_MAX = np.finfo(F).max
TINY = [F(1e-45), F(-1e-45), F(1e-40), F(-1e-40), F(1.1754944e-38), F(0.0), F(-0.0)]
INF, NAN = F(np.inf), F(np.nan)
TILE = 1024
NMAX = 65536
MIN_NORMAL = F(1.1754944e-38)


def words(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def nb(v):
    v = F(v)
    return [np.nextafter(v, F(-np.inf)), v, np.nextafter(v, F(np.inf))]


def pm(vals):
    """nb of +v and -v for every v"""
    return [x for v in vals for s in (1, -1) for x in nb(F(s) * F(v))]


def uniq(vals):
    """the values in order of first appearance, distinct as words (so +0 and -0 both stay)"""
    seen, out = set(), []
    for v in vals:
        w = int(words([v])[0])
        if w not in seen:
            seen.add(w)
            out.append(F(v))
    return np.array(out, F)


def product(cols):
    """full product as index columns [len(cols), N], the first column fastest"""
    grids = np.meshgrid(*[np.arange(len(c)) for c in cols], indexing="ij")
    return np.stack([g.ravel(order="F") for g in grids])


def pairwise_sample(cols, count, seed):
    """`count` seeded rows of the product of the columns (index form [len(cols), count]) in which every pair of values from two different columns
    occurs: asserted, not hoped for"""
    sizes = [len(c) for c in cols]
    total = math.prod(sizes)
    rng = np.random.default_rng(seed)
    flat = np.sort(rng.choice(total, size=min(count, total), replace=False))
    idx = np.stack(np.unravel_index(flat, sizes, order="F"))
    for i, j in itertools.combinations(range(len(cols)), 2):
        seen = np.zeros((sizes[i], sizes[j]), bool)
        seen[idx[i], idx[j]] = True
        assert seen.all(), f"columns {i} and {j}: {int((~seen).sum())} value pairs missing from the sample"
    return idx


def pad(cols, rest):
    """pad equal-length columns with the rest state up to the next multiple of TILE"""
    n = len(cols[0])
    m = -(-n // TILE) * TILE
    assert m <= NMAX
    return [np.concatenate([np.asarray(c), np.full(m - n, r, np.asarray(c).dtype)]) for c, r in zip(cols, rest)], n


def is_denormal(x):
    x = np.asarray(x, F)
    return (x != 0) & (np.abs(x) < MIN_NORMAL)


def mixed_groups(big):
    """number of 64-env groups that hold both table-branch (|angle| >= 120) and fast-branch lanes"""
    g = np.asarray(big, bool).reshape(-1, 64)
    return int((g.any(axis=1) & ~g.all(axis=1)).sum())


def blob_of(f32_cols, n):
    """f32 columns + the episode column (the env's index)"""
    return np.stack([words(c) for c in f32_cols] + [np.arange(n, dtype=np.uint32)])


# ---- Pendulum -------------------------------------------------------------------------------------------------------------------------
PD_TH = uniq(pm([0, PI_F, TWO_PI_F, F(3) * PI_F, 119.99, 120, 1e6, 2.0 ** 24, 1e30]) + TINY + [FLT_MAX, -FLT_MAX])
PD_THDOT = uniq(pm([0, 1, 7.9, 8]) + TINY + [F(1e-20), F(-1e-20), F(100), F(-3e38)])
PD_TORQUE = uniq(pm([0, 2]) + [INF, -INF, F(1e30), F(3e38)] + TINY)


@functools.lru_cache(None)
def pendulum_cases():
    """-> (blob [3, n], torques [n]); the full product, th fastest"""
    import pendulum_ref as R
    idx = product([PD_TH, PD_THDOT, PD_TORQUE])
    (th, thdot, a), real = pad([PD_TH[idx[0]], PD_THDOT[idx[1]], PD_TORQUE[idx[2]]], (F(0), F(0), F(0)))
    n = len(th)
    for g in (10.0, 0.0, -3.5):
        th2, thdot2, rew, nan = R.step_words(th, thdot, a, F(1.5) * F(g))
        assert not nan.any()
        with np.errstate(all="ignore"):
            raw = thdot + ((F(1.5) * F(g)) * R.sinf(th) + F(3.0) * np.clip(a, F(-2), F(2))) * F(0.05)
        # each clamp on each side, on the boundary and beyond it
        for s in (1, -1):
            assert (a == F(2 * s)).any() and (s * a > 2).any() and ((s * a < 2) & (s * a > 1.9)).any()
            assert ((thdot2 == F(8 * s)) & (s * raw > 8)).any() and ((thdot2 == F(8 * s)) & (raw == F(8 * s))).any()
            assert ((s * thdot2 < 8) & (s * thdot2 > 7.99)).any()
        assert is_denormal(rew).sum() >= 16 and is_denormal(th2).sum() >= 16 and is_denormal(thdot2).sum() >= 16
        assert (words(th2) == 0x80000000).any() and (words(rew) == 0x80000000).any()   # -0.0 as a result
        # the wrap of the cost's angle on either side of +-pi, and fmodf quotients far beyond 5
        assert (np.abs(th) > 1e6).sum() >= 1000 and np.isinf(th2).sum() == 0
        # the table branch and the fast branch in one 64-env group: of the imported angle and of the stepped one
        full = real - real % 64
        assert mixed_groups(np.abs(th[:full]) >= 120) == full // 64 and mixed_groups(np.abs(th2[:full]) >= 120) == full // 64
    blob = blob_of([th, thdot], n)
    for v in (blob, a):
        v.setflags(write=False)
    return blob, a


def pendulum_gravity_subset():
    """the 4096 cases stepped under g = 0 and g = -3.5 as well: a seeded choice, in case order"""
    n = pendulum_cases()[0].shape[1]
    return np.sort(np.random.default_rng(4096).choice(n, 4096, replace=False))


# ---- Acrobot --------------------------------------------------------------------------------------------------------------------------
V1, V2 = F(4 * math.pi), F(9 * math.pi)
AB_TH1 = uniq(pm([0, PI_F, F(math.pi / 2), F(2 * math.pi / 3), 119, 120]) + TINY + [F(1e6), F(-1e30)])
AB_TH2 = uniq(pm([0, PI_F]) + [F(math.pi / 2), F(-12345.678)] + TINY)
AB_W1 = uniq(pm([V1]) + [F(0), F(1), F(13)] + TINY + [F(1e30)])
AB_W2 = uniq(pm([V2]) + [F(0), F(1), F(-29)] + TINY)
AB_SEEDS, AB_SPAN = 320, 64   # threshold search: seeds, and floats taken on either side of each crossing
AB_GRID = NMAX - AB_SEEDS * (2 * AB_SPAN + 1) - 512


def acrobot_q(th1, th2, w1, w2, a):
    """the post-step termination word q = -c1' - (c1' c2' - s1' s2') of the restatement, and its done flag"""
    import acrobot_ref as R
    n1, n2, _, _, _, done, _ = R.step_words(th1, th2, w1, w2, a)
    c1, s1, c2, s2 = R.cosf(n1), R.sinf(n1), R.cosf(n2), R.sinf(n2)
    with np.errstate(all="ignore"):
        g2 = c1 * c2 - s1 * s2
        return (-c1) - g2, done


def acrobot_threshold_cases():
    """states whose post-step q is 1.0f or next to it: th1 bisected in [1.2, 2.4] on the restatement for seeded (th2, w1, w2, a), then the
    2 AB_SPAN + 1 floats around each crossing"""
    rng = np.random.default_rng(20)
    th2, w1, w2 = (rng.uniform(-0.5, 0.5, AB_SEEDS).astype(F) for _ in range(3))
    a = rng.integers(0, 3, AB_SEEDS).astype(np.uint32)
    lo, hi = np.full(AB_SEEDS, words([F(1.2)])[0], np.int64), np.full(AB_SEEDS, words([F(2.4)])[0], np.int64)   # positive floats: words are ordered
    as_f = lambda w: w.astype(np.uint32).view(F)
    above = lambda w: acrobot_q(as_f(w), th2, w1, w2, a)[0] > F(1)
    ok = ~above(lo) & above(hi)
    while ((hi - lo) > 1).any():
        mid = (lo + hi) // 2
        up = above(mid)
        hi, lo = np.where(up, mid, hi), np.where(up, lo, mid)
    k = np.arange(-AB_SPAN, AB_SPAN + 1, dtype=np.int64)
    th1 = as_f((hi[ok][:, None] + k[None, :]).ravel())
    rep = lambda v: np.repeat(v[ok], len(k))
    return th1, rep(th2), rep(w1), rep(w2), rep(a)


@functools.lru_cache(None)
def acrobot_cases():
    """-> (blob [5, n], actions [n] uint32): a pairwise-complete seeded sample of the product (th1 fastest), then the threshold cases"""
    import acrobot_ref as R
    cols = [AB_TH1, AB_TH2, AB_W1, AB_W2, np.arange(3)]
    idx = pairwise_sample(cols, AB_GRID, 21)
    grid = [AB_TH1[idx[0]], AB_TH2[idx[1]], AB_W1[idx[2]], AB_W2[idx[3]], idx[4].astype(np.uint32)]
    thr = acrobot_threshold_cases()
    n_grid = len(grid[0]) - len(grid[0]) % 64
    (th1, th2, w1, w2, a), real = pad([np.concatenate([g[:n_grid], t]) for g, t in zip(grid, thr)], (F(0), F(0), F(0), F(0), np.uint32(1)))
    n = len(th1)
    # the threshold: q == 1 does not terminate, its upper neighbour does
    q, done = acrobot_q(th1, th2, w1, w2, a)
    t = slice(n_grid, real)
    one = F(1)
    tie, below, over = (int((q[t] == v).sum()) for v in (one, np.nextafter(one, F(0)), np.nextafter(one, F(2))))
    assert tie >= 32 and below >= 16 and over >= 16, (tie, below, over)
    assert np.array_equal(done[t].astype(bool), q[t] > one) and not done[t][q[t] == one].any()
    n1, n2, nw1, nw2, rew, done, bad = R.step_words(th1, th2, w1, w2, a)
    assert not bad.any() and done.sum() >= 1000 and (~done.astype(bool)).sum() >= 1000
    for v, lim in ((nw1, V1), (nw2, V2)):   # each clamp on each side
        assert (v == lim).sum() >= 16 and (v == -lim).sum() >= 16 and ((np.abs(v) < lim) & (np.abs(v) > lim * F(0.9))).any()
    fin = np.isfinite(n1) & np.isfinite(n2) & np.isfinite(nw1) & np.isfinite(nw2)
    assert fin.sum() >= n // 2 and (~fin).sum() >= 1000   # 1e30 velocities overflow to NaN results: present, and not everything
    assert sum(int(is_denormal(v).sum()) for v in (n1, n2, nw1, nw2)) >= 16
    assert mixed_groups(np.abs(th1[:n_grid]) >= 120) == n_grid // 64
    blob = blob_of([th1, th2, w1, w2], n)
    for v in (blob, a):
        v.setflags(write=False)
    return blob, a


# ---- MountainCar and MountainCarContinuous ----------------------------------------------------------------------------------------------
MC_POS = uniq([x for v in (F(-1.2), F(-1.2) + F(0.07), F(0.45), F(0.5), F(0.6) - F(0.07), F(0.6), F(-0.5), F(0)) for x in nb(v)] + TINY)
MC_VEL = uniq(pm([0, 0.07, 0.03]) + TINY)
MCC_FORCE = uniq(pm([0, 1]) + [INF, -INF, F(1e30)] + TINY)
MC_GOAL_VELOCITIES = (0.0, 0.03)
MC_LANDING_STARTS = np.array(nb(F(0.4)) + nb(F(0.45) - F(0.05)), F)   # further starts of the landing cases: the goals reached at a speed above 0.03


def oracle_step(kind, blob, actions, **cfg):
    """one oracle step from the blob -> (obs, reward, done, truncated)"""
    from oracle import oracle as ora
    ref = ora.OracleVec(kind, blob.shape[1], **cfg)
    ref.set_state(np.ascontiguousarray(blob, np.uint32).view(F))
    return ref.step(actions)


def mc_solve(cont, pos, act, targets, col):
    """for every (position, action, target) the start velocity that makes the stepped position (col 0) or velocity (col 1) land exactly on the target:
    found with the oracle among the 33 floats around a first guess from the step's velocity increment; the oracle decides.  -> (p, v, a, target)"""
    from oracle import oracle as ora
    kind = ora.MOUNTAINCAR_CONT if cont else ora.MOUNTAINCAR
    targets = np.asarray(targets, F)
    P, A, T = np.meshgrid(np.arange(len(pos)), np.arange(len(act)), np.arange(len(targets)), indexing="ij")
    P, A, T = P.ravel(), A.ravel(), T.ravel()
    p, a, t = pos[P], act[A], targets[T]
    with np.errstate(all="ignore"):
        force = np.clip(a, F(-1), F(1)) * F(0.0015) if cont else (a.astype(F) - F(1)) * F(0.001)
        inc = force + _cosf(F(3) * p) * F(-0.0025)
        guess = (t.astype(np.float64) - (p.astype(np.float64) if col == 0 else 0.0) - inc.astype(np.float64)).astype(F)
    keep = np.abs(guess) <= 0.08
    p, a, t, guess = p[keep], a[keep], t[keep], guess[keep]
    found = np.zeros(len(p), bool)
    vel = np.zeros(len(p), F)
    for k in range(-16, 17):   # every candidate through the oracle; the first that lands on the target is kept
        w = words(guess).astype(np.int64)
        sign = np.where(w & 0x80000000, -1, 1)
        mag = (w & 0x7FFFFFFF) + sign * k
        cand = np.where(mag >= 0, mag | (w & 0x80000000), (-mag) | ((w & 0x80000000) ^ 0x80000000)).astype(np.uint32).view(F)
        blob = np.stack([words(p), words(cand), np.zeros(len(p), np.uint32)])
        hit = (oracle_step(kind, blob, a)[0][col] == t) & ~found
        vel[hit], found = cand[hit], found | hit
    return p[found], vel[found], a[found], t[found]


def mc_landing_cases(cont, pos, act):
    """the velocities that make the stepped position land exactly on -1.2, the goal position or 0.6, or on a float next to one of them; and, from the
    positions at or beyond the goal less one top speed, those that make the stepped velocity land on a goal velocity (0, 0.03) or next to one"""
    goal = F(0.45) if cont else F(0.5)
    on_p = mc_solve(cont, pos, act, [x for v in (F(-1.2), goal, F(0.6)) for x in nb(v)], 0)
    on_v = mc_solve(cont, pos[pos >= goal - F(0.07)], act, [F(0)] + nb(F(0.03)), 1)
    inside = mc_solve(cont, pos, act, [nb(F(0.07))[0], nb(F(-0.07))[2]], 1)   # the speed clamp missed by one float
    # a stepped velocity next to 0 is a denormal, which no sum with the step's increment gives: beside the tie, the start velocities next to its own
    z = on_v[3] == 0
    side = [tuple(np.concatenate([x[z], x[z]]) for x in (on_v[0], on_v[2])) + (np.concatenate([np.nextafter(on_v[1][z], F(-1)), np.nextafter(on_v[1][z], F(1))]),)]
    (sp, sa, sv), = side
    on_v = (np.concatenate([on_v[0], sp]), np.concatenate([on_v[1], sv]), np.concatenate([on_v[2], sa]), np.concatenate([on_v[3], np.full(len(sp), NAN, F)]))
    return tuple(np.concatenate([x, y, z]) for x, y, z in zip(on_p, on_v, inside)) + (len(on_p[0]),)


def _cosf(x):
    import pendulum_ref as R
    return R.cosf(x)


@functools.lru_cache(None)
def mountain_car_cases(cont):
    """-> (blob [3, n], actions [n]): uint32 actions 0..2 for MountainCar, float32 forces for MountainCarContinuous.  The product position x velocity x
    action (position fastest), then the landing cases.  The same cases serve both goal velocities."""
    from oracle import oracle as ora
    kind = ora.MOUNTAINCAR_CONT if cont else ora.MOUNTAINCAR
    act = MCC_FORCE if cont else np.arange(3, dtype=np.uint32)
    idx = product([MC_POS, MC_VEL, act])
    lp, lv, la, lt, n_on_p = mc_landing_cases(cont, np.concatenate([MC_POS, MC_LANDING_STARTS]), act)
    vt, lt = lt[n_on_p:], lt[:n_on_p]
    goal = F(0.45) if cont else F(0.5)
    for target in (F(-1.2), goal, F(0.6)):   # landings on each target and on its neighbours inside the track: from every position within reach
        for v in nb(target)[1:] if target == F(-1.2) else nb(target)[:2] if target == F(0.6) else nb(target):
            assert (lt == v).sum() >= 4 * len(act), (cont, float(v), int((lt == v).sum()))
    for gv in MC_GOAL_VELOCITIES:   # and on each goal velocity and its neighbours
        assert all((vt == v).sum() >= 4 * len(act) for v in ([F(0)] if gv == 0 else nb(gv))), (cont, gv)
    (p, v, a), real = pad([np.concatenate([MC_POS[idx[0]], lp]), np.concatenate([MC_VEL[idx[1]], lv]), np.concatenate([act[idx[2]], la])],
                          (F(-0.5), F(0), F(0) if cont else np.uint32(1)))
    n = len(p)
    blob = blob_of([p, v], n)
    for gv in MC_GOAL_VELOCITIES:
        obs, rew, done, trunc = oracle_step(kind, blob, a, goal_velocity=gv)
        p2, v2 = obs
        done = done.astype(bool)
        assert not trunc.any() and done.sum() >= 100 and (~done).sum() >= 100
        # the goal: position on the tie (done), just below (not done) and above, with a velocity that qualifies; the velocity on its own tie
        ok_v = v2 >= F(gv)
        assert (done & (p2 == goal)).any() and (~done & (p2 == nb(goal)[0]) & ok_v).any() and (done & (p2 == nb(goal)[2])).any()
        assert (done & (v2 == F(gv))).any() and (done & (v2 > F(gv)) & (v2 < F(gv) + F(1e-8))).any()
        assert (~done & (p2 >= goal) & (v2 < F(gv)) & (v2 > F(gv) - F(1e-8))).any()
        # the position clamps and the wall: on the boundary exactly, and beside it
        assert ((p2 == F(-1.2)) & (v2 == 0)).sum() >= 50 and (p2 == nb(F(-1.2))[2]).any() and (p2 == F(0.6)).sum() >= 50 and (p2 == nb(F(0.6))[0]).any()
        assert (v2 == F(0.07)).sum() >= 50 and (v2 == F(-0.07)).sum() >= 50 and (v2 == nb(F(0.07))[0]).any() and (v2 == nb(F(-0.07))[2]).any()
        # (no result of this step can be a denormal: every sum has a term of 1e-3 or more; the denormals are inputs, to cos(3 p) and to the sums)
        assert is_denormal(p).sum() >= 100 and is_denormal(v).sum() >= 100
        if cont:
            assert is_denormal(a).sum() >= 100 and (a > 1).any() and (a < -1).any() and (a == 1).any() and (a == -1).any()
            assert (rew == F(100)).any() and ((rew < 100) & (rew > 99)).any() and np.isinf(rew).any()   # 0.1 a^2 overflows for a = 1e30 and +-inf
    for x in (blob, a):
        x.setflags(write=False)
    return blob, a


# ---- CartPole -------------------------------------------------------------------------------------------------------------------------
CP_THETA_THR = F(F(F(12.0) * F(2.0)) * F(3.14159265358979323846) / F(360.0))
CP_X = uniq(pm([2.4]) + [F(0)] + TINY)
CP_THETA = uniq(pm([CP_THETA_THR]) + [F(0)] + TINY + [F(119.99), F(120), F(1e6)])
CP_VEL = uniq([F(0), F(1), F(-1)] + TINY + [F(1e30)])
CP_STEPS = np.array([498, 499, 500], np.uint32)
CP_SBT = np.array([0xFFFFFFFF, 0, 1], np.uint32)   # None, Some(0), Some(1)
CP_CONFIGS = [(sb, eu) for sb in (False, True) for eu in (True, False)]


@functools.lru_cache(None)
def cartpole_cases():
    """-> (blob [7, n], actions [n] uint32): a pairwise-complete seeded sample of the product (theta fastest).  The same cases serve the four
    (sutton_barto_reward, is_euler) configurations."""
    from oracle import oracle as ora
    order = [2, 0, 1, 3, 4, 5, 6]   # theta fastest
    cols = [CP_X, CP_VEL, CP_THETA, CP_VEL, CP_STEPS, CP_SBT, np.arange(2)]
    idx = pairwise_sample([cols[k] for k in order], NMAX // 2 - 256, 22)[np.argsort(order)]
    (x, xd, th, thd, steps, sbt, a), real = pad([CP_X[idx[0]], CP_VEL[idx[1]], CP_THETA[idx[2]], CP_VEL[idx[3]], CP_STEPS[idx[4]], CP_SBT[idx[5]],
                                                 idx[6].astype(np.uint32)], (F(0), F(0), F(0), F(0), np.uint32(0), np.uint32(0xFFFFFFFF), np.uint32(0)))
    n = len(x)
    blob = np.stack([words(x), words(xd), words(th), words(thd), steps, sbt, np.arange(n, dtype=np.uint32)])
    for sb, eu in CP_CONFIGS:
        obs, rew, done, trunc = oracle_step(ora.CARTPOLE, blob, a, sutton_barto_reward=sb, is_euler=eu)
        done, trunc = done.astype(bool), trunc.astype(bool)
        assert np.array_equal(trunc[:real], steps[:real] >= 499) and not (done & trunc).any() and done.sum() >= 1000
        live = ~trunc
        for col, thr in ((0, F(2.4)), (2, CP_THETA_THR)):   # each threshold: the tie does not terminate, its neighbour beyond does, on both sides
            others_in = (np.abs(obs[2 - col]) <= (CP_THETA_THR if col == 0 else F(2.4)))
            for s in (1, -1):
                v = obs[col] * F(s)
                if col == 2 and not eu:   # the semi-implicit form adds 0.5 tau^2 thetaacc, which is never 0 at the threshold: no tie, the two sides within 0.02
                    assert (live & others_in & (v <= thr) & (v > thr - F(2e-2)) & ~done).any() and (live & (v > thr) & (v < thr + F(2e-2)) & done).any()
                    continue
                assert (live & others_in & (v == thr) & ~done).any() and (live & (v == nb(thr)[2]) & done).any()
                assert (live & others_in & (v == nb(thr)[0]) & ~done).any()
        assert sorted(set(np.unique(rew).tolist())) == ([-1.0, 0.0, 1.0] if sb else [0.0, 1.0])
        assert sum(int(is_denormal(obs[k]).sum()) for k in range(4)) >= 16 and np.isnan(obs).any()
        assert mixed_groups(np.abs(th[:real - real % 64]) >= 120) >= real // 64 - 1
    for v in (blob, a):
        v.setflags(write=False)
    return blob, a


# ---- non-finite states ------------------------------------------------------------------------------------------------------------------
NON_FINITE = (INF, -INF, NAN)


@functools.lru_cache(None)
def non_finite_cases(kind):
    """kind in ("pendulum", "acrobot", "mountain_car_continuous") -> (blob, actions): +-inf and NaN in each f32 column in turn, over a small product of
    ordinary values in the other columns and the family's actions"""
    if kind == "pendulum":
        base, acts, rest = [F([0, 1e-40, 3.0, -200.0]), F([0, -1.0, 8.0])], F([0, -2.5, 1e-40, np.inf]), (F(0), F(0), F(0))
    elif kind == "acrobot":
        base = [F([0, 2.0, -130.0]), F([0, -1.0]), F([0, V1, -1.0]), F([0, -V2])]
        acts, rest = np.arange(3, dtype=np.uint32), (F(0), F(0), F(0), F(0), np.uint32(1))
    else:
        base, acts, rest = [F([-1.2, -0.5, 0.45, 0.6]), F([0, 0.07, -0.03, 1e-40])], F([0, 1.0, -1.5, 1e-40, np.inf]), (F(-0.5), F(0), F(0))
    out = [[] for _ in range(len(base) + 1)]
    for c in range(len(base)):
        cols = [np.array(NON_FINITE, F) if k == c else b for k, b in enumerate(base)] + [acts]
        idx = product(cols)
        for k, col in enumerate(cols):
            out[k].append(col[idx[k]])
    cols, real = pad([np.concatenate(o) for o in out], rest)
    n = len(cols[0])
    blob, a = blob_of(cols[:-1], n), cols[-1]
    with np.errstate(all="ignore"):
        if kind == "pendulum":
            import pendulum_ref as R
            res = R.step_words(cols[0], cols[1], a, F(15))[:3]
        elif kind == "acrobot":
            import acrobot_ref as R
            res = R.step_words(*cols[:4], a)[:4]
        else:
            from oracle import oracle as ora
            obs, rew, _, _ = oracle_step(ora.MOUNTAINCAR_CONT, blob, a)
            res = (obs[0], obs[1], rew)
    nan_results = int(np.isnan(np.stack(res)).any(axis=0).sum())
    assert nan_results >= real // 3, (kind, nan_results, real)   # every NaN import and most infinities give a NaN somewhere
    if kind != "acrobot":   # (there every non-finite word reaches every result)
        assert (~np.isnan(np.stack(res)).any(axis=0))[:real].any()    # some non-finite imports come back finite: a clamp took them
    for v in (blob, a):
        v.setflags(write=False)
    return blob, a
