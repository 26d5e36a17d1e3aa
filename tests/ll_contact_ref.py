"""Float64 rules for LunarLander's contact steps, from two sources alone: the reference's text (src/box_2d/lunar_lander.rs, cited
by line) and the float64 distance between the bodies' polygons and the terrain polyline (tests/ll_geom_ref.py).  Nothing of the
contact solver is restated and no momentum is balanced: the rules say which OUTCOMES a step may have (leg flags, crash, sleep,
rewards, endings, the wind gate, the terrain a reset builds), given where the polygons are before and after it.  Nothing here
imports the engine or the oracle.

Blob columns ([27, n] 32-bit words, include/mgym.h): 0-17 bodies (hull, leg 0, leg 1: origin x, y, angle, vx, vy, w), 18 / 19 leg
flags, 20 game_over, 21 awake, 22 prev_shaping (NaN = None), 23 / 24 wind and torque index (i32), 25 step, 26 episode (u32).

What the rules lean on, from Box2D v2.4.1 and the reference's ContactDetector (:154-205):

(a) The order inside b2World::Step.  b2ContactManager::Collide evaluates every existing contact at the PRE-step poses; then the
    island is solved and the bodies move; then b2World::SolveTOI takes a body that would pass through the terrain back to its
    time of impact, evaluates that contact THERE, and moves the body on for the rest of the step with the velocity the
    sub-step's solver leaves it.  That velocity is the one the blob shows after the step, so the pose of the last impact lies
    on the ray  post pose - s h v_post, s in [0, 1]  (centre of mass and angle, b2Sweep).  A flag after the step therefore
    describes the pre-step pose or a pose on that ray ("backward sweep"), never the post pose alone.  The issue offered the
    linear sweep from the pre to the post pose as the evidence of a touch within the step; on the oracle it explains 1 of the
    74 leg-flag rows and none of the 11 crash rows that are far at both ends, and the backward sweep explains all of them (it
    comes down to 0.0144 .. 0.0148 = RADIUS - b2_linearSlop, where SolveTOI's position correction leaves a body).  Both sweeps
    are accepted as evidence.
(b) The flags are EVENTS, not states.  Every (leg, terrain edge) pair is a contact of its own; begin_contact of any of them sets
    the leg's flag and end_contact of any of them clears it (:154-205), also while another edge still holds the leg.  So "leg
    inside the radius, flag clear" is a legitimate state: it follows an EndContact of a neighbouring edge, and lasts until the
    next BeginContact.  This resolves the issue's open question (a leg at 0.0098, 0.0062, 0.015 with its flag clear): the oracle
    and the kernels are right, and gymnasium's ContactDetector behaves the same.  Landings do end asleep with a flag clear (9 of
    42 on the oracle), so "+100 implies both flags" is NOT a rule.  What follows from (a) and (b) and can be tested:
      R5a  flag set after the step       =>  the leg was near the terrain at the pre pose or on the backward sweep;
      R5b  flag falls, leg inside before =>  a second edge is within reach (else nothing could have ended);
      R5c  leg arrives (far from every edge one step earlier, inside now) => the flag is set before or after this step, unless
           a second edge is within reach.
    By induction over the steps R5b and R5c leave no other way to "inside, flag clear".
(c) b2CollideEdgeAndPolygon has no vertex-vertex manifold: its axes are the edge's normal and the polygon's normals, and
    b2ClipSegmentToLine cuts at the reference edge's end planes without the radius.  A polygon within RADIUS of an edge's END
    only may touch neither edge that meets there.  "Inside" therefore means: within RADIUS - delta of an edge and farther than
    RADIUS + delta from both of its end points.

Three rules of the issue were false as stated and are kept in the form their own sources give them: R4's "the hull stays where
it hit" (after Collide has raised game_over at the pre pose, the leg joints and the position correction push the hull out again,
to 0.048 on the oracle: the pre pose and the backward sweep are evidence too), R6's "+100 implies both flags" (see (b)), and R7's
"if and only if" (an environment can leave the viewport on the step it crashes; both directions are kept as implications).

Numbers measured on the CPU oracle by `python tests/ll_contact_cases.py --measure`; the asserted bounds are 4 x the measured
values, as tests/ll_flight_ref.py does."""
import numpy as np

import ll_geom_ref as G

F = np.float32
SCALE, FPS = F(30.0), F(50.0)                                   # lunar_lander.rs:31-32
VIEWPORT_W, VIEWPORT_H = F(600.0), F(400.0)                     # :57-58
W, H = VIEWPORT_W / SCALE, VIEWPORT_H / SCALE                   # :748-749 (f32, as the reference computes them)
CHUNKS = 11                                                     # :751
N_EDGES = CHUNKS                                                # 10 of the polyline and the bottom edge
LEG_DOWN = F(18.0)                                              # :48
HELIPAD_Y = H / F(4.0)                                          # :765
SLOT_RESET0 = 0                                                 # csrc/philox.h
STEP_H = 1.0 / 50.0

RADIUS = G.RADIUS                # 2 * b2_polygonRadius
LINEAR_SLOP = 0.005              # b2_linearSlop
SLEEP_LIN, SLEEP_ANG = 0.01, 2.0 / 180.0 * np.pi                # b2_linearSleepTolerance, b2_angularSleepTolerance
SLEEP_STEPS = 25                 # b2_timeToSleep 0.5 at h = 1 / 50

# delta: half-width of the band around RADIUS in which a rule declines to judge; the issue allows at most half of b2_linearSlop.
# Measured: with the rules in the form above the oracle shows no exception at any delta from 0.0005 up (--measure prints the
# counts); 0.002, the issue's estimate, is used.
DELTA = 0.002
BAND_CAP = 0.05                  # share of the checked case-steps a rule may decline

# measured on the oracle (float64 on its f32 words), `python tests/ll_contact_cases.py --measure`:
MEASURED_REWARD = 7.744e-05      # worst |reward - float64 reward| (the shaping is a difference of two numbers of some hundreds)
MEASURED_SINK = 0.0              # deepest lowest vertex below the polyline before an ending, as a positive number: none sinks
BOUND_REWARD = 4.0 * MEASURED_REWARD
BOUND_SINK = min(4.0 * MEASURED_SINK, float(G.LEG_W / G.SCALE))   # never more than the leg's half-width

RULES = ("R1", "R2", "R3", "R4", "R5", "R7", "R8")


# ---------------------------------------------------------------------------------------------------------------- terrain
def terrain(heights):
    """heights [12, n] f32 (:753-756) -> (chunk_x [11], smooth_y [n, 11]) float64, computed in f32 as the reference does:
    chunk_x = W / (CHUNKS - 1) * i (:758-760), the five helipad chunks at H / 4 (:766-770),
    smooth_y[i] = 0.33 * (h[i - 1 saturating at 0] + h[i] + h[i + 1]) (:772-774).  The polyline's edges run between neighbours
    (:795-808); bottom_edge() is the extra one (:783-792)."""
    h = np.array(heights, F).reshape(CHUNKS + 1, -1).copy()
    chunk_x = np.array([W / F(CHUNKS - 1) * F(i) for i in range(CHUNKS)], F)
    h[CHUNKS // 2 - 2:CHUNKS // 2 + 3] = HELIPAD_Y
    smooth = np.stack([F(0.33) * ((h[max(i - 1, 0)] + h[i]) + h[i + 1]) for i in range(CHUNKS)], 1)
    return chunk_x.astype(np.float64), smooth.astype(np.float64)


def bottom_edge():
    return np.array([0.0, 0.0]), np.array([float(W), 0.0])


def deterministic_heights(n):
    """reset_deterministic: H / 8 everywhere (:1276-1280)"""
    return np.full((CHUNKS + 1, n), H / F(8.0), F)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) over arrays of counters -> four uint32 arrays"""
    M = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(v, np.uint64) & M for v in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & M, p1 >> np.uint64(32), p1 & M
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    return [v.astype(np.uint32) for v in (c0, c1, c2, c3)]


def seeded_heights(seed, gid, episode):
    """Heights of the seeded reset (include/mgym.h, csrc/philox.h): the 12 words of env_draw(seed, gid, episode, SLOT_RESET0..2),
    that is Philox4x32-10(key = seed; counter = (lo32(gid), hi32(gid), episode, slot)), each through the 23-bit uniform
    (w >> 9) * 2^-23 and times H / 2 (random_range(0.0..h / 2.0), :755).  episode is the counter BEFORE the reset raises it:
    blob column 26 minus one.  gid, episode: arrays [n] -> [12, n] f32."""
    gid = np.asarray(gid, np.uint64)
    ep = np.asarray(episode, np.uint64)
    words = []
    for slot in range(3):
        words += philox4x32_10(gid & np.uint64(0xFFFFFFFF), gid >> np.uint64(32), ep, np.uint64(SLOT_RESET0 + slot), int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    u = np.stack([(w >> np.uint32(9)).astype(F) * F(1.0 / 8388608.0) for w in words])
    return u * (H / F(2.0) - F(0.0)) + F(0.0)


# --------------------------------------------------------------------------------------------------------------- geometry
_SHAPES = [G.shape(0), G.shape(1), G.shape(1)]
_LC = [G.polygon_mass(V, 1.0)[1] for V in _SHAPES]
_RMAX = [np.sqrt(((V - lc) ** 2).sum(1)).max() for V, lc in zip(_SHAPES, _LC)]
SKIP = 0.5                       # geometry(): a body this far above every terrain vertex gets no distances


def poses64(blob):
    """[3, 3, m] float64: per body (origin x, y, angle) from blob words 6b .. 6b + 2"""
    b = np.asarray(blob)[:18].astype(np.float64)
    return np.stack([b[6 * k:6 * k + 3] for k in range(3)])


def polygon(body, pose):
    """world polygon [m, verts, 2] of `body` at pose [3, m] (float64 sin / cos of the angle)"""
    return G.world(_SHAPES[body], pose[:2].T, pose[2])


def polyline_y(x, chunk_x, smooth_y):
    """height of the polyline under x [m, ...] for smooth_y [m, 11]; NaN outside the viewport, where there is no terrain"""
    step = chunk_x[1] - chunk_x[0]
    k = np.clip(np.floor(x / step).astype(int), 0, CHUNKS - 2)
    rows = np.arange(len(smooth_y)).reshape((-1,) + (1,) * (x.ndim - 1))
    y0, y1 = smooth_y[rows, k], smooth_y[rows, k + 1]
    return np.where((x >= chunk_x[0]) & (x <= chunk_x[-1]), y0 + (y1 - y0) * (x - chunk_x[k]) / step, np.nan)


def edges(chunk_x, smooth_y):
    """the terrain's N_EDGES edges for smooth_y [m, 11] -> (a, b) [N_EDGES, m, 2]: the polyline's ten, then the bottom edge"""
    m = len(smooth_y)
    pts = np.stack([np.broadcast_to(chunk_x, (m, CHUNKS)), smooth_y], -1)          # [m, 11, 2]
    a0, b0 = bottom_edge()
    a = np.concatenate([pts[:, :-1].transpose(1, 0, 2), np.broadcast_to(a0, (1, m, 2))])
    b = np.concatenate([pts[:, 1:].transpose(1, 0, 2), np.broadcast_to(b0, (1, m, 2))])
    return a, b


def body_edge_distances(body, pose, Wp, terr, ends=False):
    """float64 distance of the solid polygons Wp [m, v, 2] of `body` at pose [3, m] to every terrain edge, by
    ll_geom_ref.seg_poly -> [N_EDGES, m]; ends: also the smaller distance to the edge's two end points [N_EDGES, m].
    Only what can matter is evaluated, the rest stays at infinity: nothing for a body that is SKIP above the highest terrain
    vertex (the rules compare with less than 0.1), and of the polyline the edge under the body's origin and its two neighbours
    (no vertex is as far as a chunk's width from the origin)."""
    chunk_x, smooth_y = terr
    m = pose.shape[1]
    a, b = edges(chunk_x, smooth_y)
    step = chunk_x[1] - chunk_x[0]
    d, e = np.full((N_EDGES, m), np.inf), np.full((N_EDGES, m), np.inf)
    assert np.sqrt((_SHAPES[body] ** 2).sum(1)).max() < step
    low = np.nonzero(pose[1] - np.sqrt((_SHAPES[body] ** 2).sum(1)).max() <= smooth_y.max(1) + SKIP)[0]
    k0 = np.clip(np.floor(pose[0, low] / step).astype(int), 0, CHUNKS - 2)
    for off in (-1, 0, 1, None):
        ek = np.full(len(low), N_EDGES - 1) if off is None else np.clip(k0 + off, 0, CHUNKS - 2)
        pa, pb, wp = a[ek, low], b[ek, low], Wp[low]
        d[ek, low] = G.seg_poly(pa, pb, wp)
        if ends:
            e[ek, low] = np.minimum(G.pt_poly(pa, wp), G.pt_poly(pb, wp))
    return (d, e) if ends else d


def geometry(blob, terr):
    """Everything the rules need of one pose per case: blob [>= 18, m], terr = (chunk_x, smooth_y [m, 11]) -> dict:
    edge [3, N_EDGES, m] distance of each body's solid polygon to each terrain edge, end [3, N_EDGES, m] to the nearer end point
    of each edge, dist [3, m] their minimum over the edges, low [3, m] the signed height of the lowest vertex above the polyline
    (vertices outside the viewport have no terrain under them), origin [3, m] the same of the body's origin."""
    chunk_x, smooth_y = terr
    pose = poses64(blob)
    out = dict(edge=[], end=[], low=[], origin=[])
    for k in range(3):
        Wp = polygon(k, pose[k])
        d, e = body_edge_distances(k, pose[k], Wp, terr, ends=True)
        out["edge"].append(d), out["end"].append(e)
        hgt = Wp[..., 1] - polyline_y(Wp[..., 0], chunk_x, smooth_y)
        out["low"].append(np.where(np.isnan(hgt), np.inf, hgt).min(-1))
        o = pose[k, 1] - polyline_y(pose[k, 0], chunk_x, smooth_y)
        out["origin"].append(np.where(np.isnan(o), np.inf, o))
    out = {k: np.array(v) for k, v in out.items()}
    out["dist"] = out["edge"].min(1)
    return out


def take(geo, idx):
    return {k: v[..., idx] for k, v in geo.items()}


def sweep_min_distance(pose0, pose1, body, terr):
    """minimum distance to the terrain along ll_geom_ref's linear sweep (b2Sweep: centre of mass and angle linear in t) from
    pose0 to pose1 [3, m] of `body`, sampled so that no vertex moves more than TOL / 4 between samples; [m]"""
    chunk_x, smooth_y = terr
    V, lc = _SHAPES[body], _LC[body]
    rot = lambda a: np.stack([np.cos(a) * lc[0] - np.sin(a) * lc[1], np.sin(a) * lc[0] + np.cos(a) * lc[1]], -1)
    c0, c1 = pose0[:2].T + rot(pose0[2]), pose1[:2].T + rot(pose1[2])
    travel = np.sqrt(((c1 - c0) ** 2).sum(1)) + np.abs(pose1[2] - pose0[2]) * _RMAX[body]
    out = np.zeros(len(travel))
    for i in range(len(travel)):
        ns = max(2, int(np.ceil(travel[i] / (G.TOL / 4.0))) + 1)
        t = np.linspace(0.0, 1.0, ns)
        p, ang = G.sweep_pose(lc, np.broadcast_to(c0[i], (ns, 2)), np.full(ns, pose0[2, i]), np.broadcast_to(c1[i], (ns, 2)), np.full(ns, pose1[2, i]), t)
        out[i] = body_edge_distances(body, np.concatenate([p.T, ang[None]]), G.world(V, p, ang), (chunk_x, np.broadcast_to(smooth_y[i], (ns, CHUNKS)))).min()
    return out


def impact_pose(post, body):
    """the far end of the backward sweep (module docstring, (a)): the post pose of `body` taken back by one whole step of its
    post-step velocity, centre of mass and angle -> pose [3, m]"""
    b = np.asarray(post)[:18].astype(np.float64)
    lc = _LC[body]
    x, y, a1, vx, vy, w = b[6 * body:6 * body + 6]
    a0 = a1 - STEP_H * w
    rot = lambda a: np.stack([np.cos(a) * lc[0] - np.sin(a) * lc[1], np.sin(a) * lc[0] + np.cos(a) * lc[1]])
    c0 = np.stack([x, y]) + rot(a1) - STEP_H * np.stack([vx, vy])
    return np.concatenate([c0 - rot(a0), a0[None]])


def touched_on_the_way(pre, post, body, terr, cand):
    """for the cases cand (indices): how near `body` came to the terrain on the linear sweep from the pre to the post pose (the
    issue's evidence) and on the backward sweep (Box2D's, see (a)) -> (min over both [len(cand)], linear, backward)"""
    if not len(cand):
        return np.zeros(0), np.zeros(0), np.zeros(0)
    t = (terr[0], terr[1][cand])
    p0, p1 = poses64(pre[:, cand])[body], poses64(post[:, cand])[body]
    lin = sweep_min_distance(p0, p1, body, t)
    back = sweep_min_distance(impact_pose(post[:, cand], body), p1, body, t)
    return np.minimum(lin, back), lin, back


# ------------------------------------------------------------------------------------------------------------------ rules
def observation(blob):
    """obs[0..5] as :1095-1121 computes them, in float64 from the f32 hull words and the reference's f32 constants, with each
    word's tolerance: 2 spacings of f32 at the larger operand -> (obs [6, m], tol [6, m])"""
    b = np.asarray(blob, F)
    x, y, ang, vx, vy, w = (b[k].astype(np.float64) for k in range(6))
    w2, h2 = float(W / F(2.0)), float(H / F(2.0))
    pad = float(HELIPAD_Y + LEG_DOWN / SCALE)
    o = np.stack([(x - w2) / w2, (y - pad) / h2, vx * w2 / float(FPS), vy * h2 / float(FPS), ang, 20.0 * w / float(FPS)])
    big = np.stack([np.maximum(np.abs(x), w2), np.maximum(np.abs(y), pad), np.abs(vx * w2), np.abs(vy * h2), np.abs(ang), np.abs(20.0 * w)])
    big = np.maximum(big, np.abs(o))
    return o, 2.0 * np.spacing(big.astype(F)).astype(np.float64)


def shaping64(obs):
    o = np.asarray(obs, F).astype(np.float64)
    return -100.0 * np.sqrt(o[0] ** 2 + o[1] ** 2) - 100.0 * np.sqrt(o[2] ** 2 + o[3] ** 2) - 100.0 * np.abs(o[4]) + 10.0 * o[6] + 10.0 * o[7]


def shaping32(obs):
    """:1127-1131 in f32, operation by operation (the reference never fuses a * b + c)"""
    o = np.asarray(obs, F)
    return (F(-100.0) * np.sqrt(o[0] * o[0] + o[1] * o[1]) - F(100.0) * np.sqrt(o[2] * o[2] + o[3] * o[3]) - F(100.0) * np.abs(o[4])
            + F(10.0) * o[6] + F(10.0) * o[7])


def reward64(pre, obs, action):
    """:1126-1139: shaping(post obs) - prev_shaping (0 if None) - 0.30 [a == 2] - 0.03 [a in (1, 3)]"""
    prev = np.asarray(pre, F)[22].astype(np.float64)
    a = np.asarray(action)
    r = np.where(np.isnan(prev), 0.0, shaping64(obs) - prev)
    return r - 0.30 * (a == 2) - 0.03 * ((a == 1) | (a == 3))


def inside(geo, body, delta):
    """[N_EDGES, m]: within RADIUS - delta of the edge and farther than RADIUS + delta from both of its end points ((c))"""
    return (geo["edge"][body] <= RADIUS - delta) & (geo["end"][body] > RADIUS + delta)


def check(pre, post, action, obs, reward, done, trunc, wind, terr, prev=None, has_prev=None, geo=None, delta=DELTA, bound_reward=None,
          bound_sink=None, contact_rules=True):
    """One step of m case-steps: pre / post blobs [27, m], action [m], obs [8, m], reward, done, trunc [m], wind (bool, the
    handle's enable_wind), terr = (chunk_x, smooth_y [m, 11]).  prev [27, m]: the blob one step before pre, where has_prev [m]
    (R5c needs it).  geo: (geometry(prev), geometry(pre), geometry(post)) if the caller has them already.  contact_rules=False:
    R1-R3 and R7 only.
    -> (violations {rule: [m] bool}, bands {rule: [m] bool}: where the rule declines, figures for --measure and the messages)"""
    bound_reward = BOUND_REWARD if bound_reward is None else bound_reward
    bound_sink = BOUND_SINK if bound_sink is None else bound_sink
    pre, post, obs = np.asarray(pre, F), np.asarray(post, F), np.asarray(obs, F)
    reward, done = np.asarray(reward, F), np.asarray(done).astype(bool)
    m = pre.shape[1]
    no = np.zeros(m, bool)
    viol, band = {}, {r: no.copy() for r in RULES}
    flag_pre, flag_post = pre[18:20] > 0.5, post[18:20] > 0.5
    game_over, awake = post[20] > 0.5, post[21] > 0.5

    # R1
    o, tol = observation(post)
    viol["R1"] = (np.abs(obs[:6].astype(np.float64) - o) > tol).any(0) | (obs[6] != post[18]) | (obs[7] != post[19])

    # R2 (:1126-1156): -100 before +100
    oob = np.abs(obs[0]) >= F(1.0)                                   # :1150, on the f32 word
    r64 = reward64(pre, obs, action)
    lost = game_over | oob
    ends = lost | ~awake
    rerr = np.abs(reward.astype(np.float64) - r64)
    bad_reward = np.where(lost, reward != F(-100.0), np.where(~awake, reward != F(100.0), ~(rerr <= bound_reward)))
    viol["R2"] = bad_reward | (done != ends) | (post[22].view(np.uint32) != shaping32(obs).view(np.uint32)) | (np.asarray(trunc) != 0)

    # R3 (:927-959)
    d_wind = post[23].view(np.int32).astype(np.int64) - pre[23].view(np.int32)
    d_torque = post[24].view(np.int32).astype(np.int64) - pre[24].view(np.int32)
    expect = (~flag_pre.any(0)).astype(np.int64) if wind else np.zeros(m, np.int64)
    viol["R3"] = (d_wind != expect) | (d_torque != expect)

    # R7 (:1150): leaving the viewport ends the episode with -100, and a -100 ending without game_over has left it
    lost_reward = done & (reward == F(-100.0))
    viol["R7"] = (oob & ~lost_reward) | (lost_reward & ~game_over & ~oob)

    figures = dict(reward_err=np.where(ends, 0.0, rerr))
    if not contact_rules:
        return viol, band, figures
    has_prev = no.copy() if prev is None else (np.ones(m, bool) if has_prev is None else np.asarray(has_prev, bool))
    gq, gp, gs = geo if geo is not None else (geometry(prev if prev is not None else pre, terr), geometry(pre, terr), geometry(post, terr))
    near = RADIUS + delta

    # R4: game_over needs the hull near the terrain (pre pose, post pose as the issue has it, or on the way); the hull inside
    # raises it
    hull_far = game_over & ~(gp["dist"][0] <= near) & ~(gs["dist"][0] <= RADIUS + 2.0 * delta + LINEAR_SLOP)
    cand = np.nonzero(hull_far)[0]
    way, hull_lin, hull_back = np.full(m, np.nan), np.full(m, np.nan), np.full(m, np.nan)
    way[cand], hull_lin[cand], hull_back[cand] = touched_on_the_way(pre, post, 0, terr, cand)
    viol["R4"] = (hull_far & ~(way <= near)) | (inside(gp, 0, delta).any(0) & ~game_over)
    band["R4"] = (gp["dist"][0] <= near) & ~inside(gp, 0, delta).any(0) & ~game_over

    # R5: leg j = body j + 1
    v5, b5 = no.copy(), no.copy()
    lin, back = np.full((2, m), np.nan), np.full((2, m), np.nan)
    judged = dict(falls=no.copy(), arrives=no.copy(), inside=no.copy(), inside_second=no.copy())
    for j in range(2):
        body = j + 1
        # a: a set flag needs the leg near the terrain at the pre pose or on the way
        far = flag_post[j] & ~(gp["dist"][body] <= near) & ~(gs["dist"][body] <= near)       # (the post pose is the sweep's near end)
        cand = np.nonzero(far)[0]
        w_, lin[j, cand], back[j, cand] = touched_on_the_way(pre, post, body, terr, cand)
        way = np.full(m, np.nan)
        way[cand] = w_
        v5 |= far & ~(way <= near)
        # reach of each edge over the step: nearest of the three poses, less what the leg travels in a step
        p0, p1 = poses64(pre)[body], poses64(post)[body]
        b = post.astype(np.float64)
        travel = np.sqrt(((p1[:2] - p0[:2]) ** 2).sum(0)) + np.abs(p1[2] - p0[2]) * (_RMAX[body] + np.sqrt((_LC[body] ** 2).sum()))
        travel = travel + STEP_H * (np.sqrt(b[6 * body + 3] ** 2 + b[6 * body + 4] ** 2) + np.abs(b[6 * body + 5]) * _RMAX[body])
        reach = np.minimum(np.where(has_prev, gq["edge"][body], np.inf), np.minimum(gp["edge"][body], gs["edge"][body])) - travel
        in_p = inside(gp, body, delta)
        second = ((reach <= near) & ~in_p).any(0) | (in_p.sum(0) >= 2)           # another edge could have begun or ended
        # b: the flag falls with the leg inside -> only a second edge can have ended
        falls = in_p.any(0) & flag_pre[j] & ~flag_post[j]
        v5 |= falls & ~second
        # c: the leg arrives -> the flag is set by the end of this step, unless a second edge could have ended meanwhile
        arrives = has_prev & in_p.any(0) & ~(gq["edge"][body] <= near).any(0)
        v5 |= arrives & ~flag_pre[j] & ~flag_post[j] & ~second
        judged["falls"] |= falls
        judged["arrives"] |= arrives & ~second
        judged["inside"] |= in_p.any(0)
        judged["inside_second"] |= in_p.any(0) & second
        b5 |= (in_p.any(0) & second) | (np.abs(gp["dist"][body] - RADIUS) < delta) | ((gp["dist"][body] <= RADIUS - delta) & ~in_p.any(0))
    viol["R5"], band["R5"] = v5, b5

    # R8: the pre-step state of every checked step is a state before the ending; the origins always
    viol["R8"] = ~(gp["low"].min(0) >= -bound_sink) | (gp["origin"].min(0) <= 0.0) | (gs["origin"].min(0) <= 0.0)

    figures.update(dpre=gp["dist"], dpost=gs["dist"], low_pre=gp["low"], lin=lin, back=back, hull_lin=hull_lin, hull_back=hull_back, judged=judged, inside=np.stack([inside(gp, k, delta).any(0) for k in range(3)]))
    return viol, band, figures


def still(blob):
    """[..., m]: all three bodies below Box2D's sleep tolerances (|v| <= 0.01, |w| <= 2 degrees per second), float64 on the f32 words"""
    b = np.asarray(blob, F).astype(np.float64)
    ok = True
    for k in range(3):
        ok = ok & (b[..., 6 * k + 3, :] ** 2 + b[..., 6 * k + 4, :] ** 2 <= SLEEP_LIN ** 2) & (b[..., 6 * k + 5, :] ** 2 <= SLEEP_ANG ** 2)
    return ok


def check_sleep(posts, reward, done, alive, leg_dist=None, delta=DELTA):
    """R6 over whole trajectories: posts [T, 27, n], reward, done, alive [T, n] (alive: the step is checked); leg_dist [T, 2, n]:
    the legs' distances to the terrain after each step, where known.
    A +100 ending at step t needs the 25 post-step states t - 24 .. t with all three bodies below the sleep tolerances, game_over
    clear and a leg on the ground; no run of 26 such states passes without an ending.
    -> (violations [T, n], run [T, n]: length of the run of still post-step states that ends at t)"""
    T, _, n = posts.shape
    st = still(posts)
    run = np.zeros((T, n), int)
    prev = np.zeros(n, int)
    for t in range(T):
        prev = np.where(st[t], prev + 1, 0)
        run[t] = prev
    done = np.asarray(done).astype(bool)
    plus = alive & done & (np.asarray(reward, F) == F(100.0))
    bad = (posts[:, 20] > 0.5) | (posts[:, 21] > 0.5)
    if leg_dist is not None:
        bad |= ~(leg_dist.min(1) <= RADIUS + delta)
    viol = plus & ((run < SLEEP_STEPS) | bad)
    viol |= alive & ~done & (run >= SLEEP_STEPS + 1)
    return viol, run
