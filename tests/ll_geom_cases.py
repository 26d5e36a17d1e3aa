"""Cases for the collision-geometry probes (mgym_ll_geom_probe and its oracle / host twins): seeded random sets in the regime of
a lander near the terrain, and hand-built edge cases.  Columns are f32, [cols][n]; pi travels as a bit pattern.
  static (DISTANCE, MANIFOLD): v1.x v1.y v2.x v2.y pi p.x p.y angle
  sweep (TOI):                 v1.x v1.y v2.x v2.y pi c0.x c0.y a0 c.x c.y a
The float64 references of the sets are computed once per process (reference())."""
import functools

import numpy as np

import ll_geom_ref as ref

N_RANDOM = 8192
HELIPAD_Y = (400.0 / 30.0) / 4.0      # lunar_lander.rs:763
HX, HY = 2.0 / 30.0, 8.0 / 30.0       # leg half extents


def _pack(cols, pi):
    out = np.array(cols, np.float64).astype(np.float32)
    out[4] = np.asarray(pi, np.uint32).view(np.float32)
    return np.ascontiguousarray(out)


def _edges(rng, n):
    x0, y0 = rng.uniform(0.0, 18.0, n), rng.uniform(0.5, 6.0, n)
    v1 = np.stack([x0, y0])
    v2 = np.stack([x0 + 2.0, y0 + rng.uniform(-2.0, 2.0, n)])
    anchor = v1 + rng.uniform(-0.2, 1.2, n) * (v2 - v1)
    return v1, v2, anchor, (np.arange(n) & 1).astype(np.uint32)


def random_static(seed, n=N_RANDOM):
    rng = np.random.default_rng(seed)
    v1, v2, anchor, pi = _edges(rng, n)
    h = np.where(np.arange(n) % 3 == 0, rng.uniform(-0.3, 0.6, n), rng.uniform(-0.05, 0.35, n))
    p = anchor + np.stack([rng.uniform(-0.3, 0.3, n), h])
    return _pack([v1[0], v1[1], v2[0], v2[1], np.zeros(n), p[0], p[1], rng.uniform(-1.0, 1.0, n)], pi)


def random_sweeps(seed, n=N_RANDOM):
    rng = np.random.default_rng(seed)
    v1, v2, anchor, pi = _edges(rng, n)
    c0 = anchor + np.stack([rng.uniform(-0.3, 0.3, n), rng.uniform(0.05, 0.9, n)])
    c = c0 + np.stack([rng.uniform(-0.2, 0.2, n), rng.uniform(-0.45, 0.05, n)])
    a0 = rng.uniform(-1.0, 1.0, n)
    a = a0 + rng.uniform(-0.1, 0.1, n)      # 5 rad/s at 50 Hz
    return _pack([v1[0], v1[1], v2[0], v2[1], np.zeros(n), c0[0], c0[1], a0, c[0], c[1], a], pi)


def _leg_lowest(angle):
    """offset of the leg box's lowest vertex from its origin at `angle`"""
    V = ref.shape(1)
    W = ref.world(V, np.zeros(2), np.float64(angle))
    return W[np.argmin(W[:, 1])]


def _place_legs(x, y, angle):
    """tests/test_gpu_lunar.py _place(): the legs hang from the lander at (x, y, angle) where the joints put them"""
    out = []
    for sgn in (-1.0, 1.0):
        la = angle + sgn * 0.3
        ax, ay = sgn * 20.0 / 30.0, 18.0 / 30.0
        out.append((x - (np.cos(la) * ax - np.sin(la) * ay), y - (np.sin(la) * ax + np.cos(la) * ay), la))
    return out


def hand_static():
    """name -> column; the names say what each case is"""
    rows, names = [], []

    def add(name, v1, v2, pi, p, angle):
        names.append(name)
        rows.append([v1[0], v1[1], v2[0], v2[1], pi, p[0], p[1], angle])
    for gap in (0.005, 0.015, -0.003):
        add(f"leg flat on a horizontal edge, gap {gap}", (4.0, 2.0), (6.0, 2.0), 1, (5.0, 2.0 + HY + gap), 0.0)
        for ang in (0.4, -0.4):
            low = _leg_lowest(np.float32(ang))
            add(f"leg at joint limit {ang} on a horizontal edge, gap {gap}", (4.0, 2.0), (6.0, 2.0), 1, (5.0 - low[0], 2.0 - low[1] + gap), ang)
    # resting pose of _place() on the helipad edges: the leg tips 0.01 above the pad (inside the contact skin)
    legs = _place_legs(10.0, 0.0, 0.0)
    y_l = HELIPAD_Y + 0.01 - min(l[1] + _leg_lowest(np.float32(l[2]))[1] for l in legs)
    legs = _place_legs(10.0, y_l, 0.0)
    for e, (v1, v2) in enumerate((((8.0, HELIPAD_Y), (10.0, HELIPAD_Y)), ((10.0, HELIPAD_Y), (12.0, HELIPAD_Y)))):
        add(f"resting lander over helipad edge {e}", v1, v2, 0, (10.0, y_l), 0.0)
        for j, l in enumerate(legs):
            add(f"resting leg {j} on helipad edge {e}", v1, v2, 1, (l[0], l[1]), l[2])
    # a polygon vertex exactly above an edge end: the box's vertex (-hx, -hy) over v2, and the hexagon's (17, -10) / 30 over v1
    hx, hy = np.float32(2.0) / np.float32(30.0), np.float32(8.0) / np.float32(30.0)
    add("leg vertex above the edge's second end", (8.0, 3.0), (10.0, 3.5), 1, (np.float32(10.0) + hx, np.float32(3.5) + hy + np.float32(0.0078125)), 0.0)
    lx, ly = np.float32(17.0) / np.float32(30.0), np.float32(10.0) / np.float32(30.0)
    add("lander vertex above the edge's first end", (8.0, 3.0), (10.0, 2.5), 0, (np.float32(8.0) - lx, np.float32(3.0) + ly + np.float32(0.0078125)), 0.0)
    add("leg centred on the edge (deep overlap)", (4.0, 2.0), (6.0, 2.5), 1, (5.0, 2.25), 0.3)
    add("lander centred on the edge (deep overlap)", (4.0, 2.0), (6.0, 2.5), 0, (5.0, 2.25), -0.2)
    add("lander 15 m away", (2.0, 1.0), (4.0, 1.5), 0, (12.0, 12.0), 0.5)
    add("leg 15 m away", (16.0, 1.0), (18.0, 0.5), 1, (5.0, 10.0), -0.7)
    add("leg on the edge from x = 0", (0.0, 1.0), (2.0, 1.2), 1, (0.03, 1.0 + HY + 0.012), 0.0)
    add("lander straddling x = 0", (0.0, 1.0), (2.0, 1.2), 0, (0.1, 1.35), 0.1)
    add("leg on the edge to x = 20", (18.0, 1.5), (20.0, 1.0), 1, (19.97, 1.0 + HY + 0.012), 0.05)
    add("lander straddling x = 20", (18.0, 1.5), (20.0, 1.0), 0, (19.9, 1.4), -0.1)
    cols = np.array(rows, np.float64).T
    return names, _pack(cols, cols[4].astype(np.uint32))


def hand_sweeps():
    rows, names = [], []
    lc = [ref.polygon_mass(ref.shape(pi), 1.0)[1] for pi in (0, 1)]

    def add(name, v1, v2, pi, p0, a0, p1, a1):
        """poses are given for the body ORIGIN; the sweep carries the centre c = p + R(a) localCenter"""
        c0 = np.asarray(p0, np.float64) + ref.world(lc[pi][None, :], np.zeros(2), np.float64(a0))[0]
        c1 = np.asarray(p1, np.float64) + ref.world(lc[pi][None, :], np.zeros(2), np.float64(a1))[0]
        names.append(name)
        rows.append([v1[0], v1[1], v2[0], v2[1], pi, c0[0], c0[1], a0, c1[0], c1[1], a1])
    e1, e2 = (4.0, 2.0), (6.0, 2.0)
    add("exact overlap at t = 0 (leg across the edge)", e1, e2, 1, (5.0, 2.1), 0.2, (5.0, 1.9), 0.25)
    add("exact overlap at t = 0 (lander across the edge)", e1, e2, 0, (5.0, 2.1), -0.3, (5.1, 2.0), -0.25)
    add("lander 15 m away", (2.0, 1.0), (4.0, 1.5), 0, (12.0, 12.0), 0.5, (12.1, 11.6), 0.55)
    add("leg 15 m away", (16.0, 1.0), (18.0, 0.5), 1, (5.0, 10.0), -0.7, (4.9, 9.7), -0.75)
    add("zero motion, separated", e1, e2, 1, (5.0, 2.0 + HY + 0.1), 0.0, (5.0, 2.0 + HY + 0.1), 0.0)
    add("zero motion, inside the target band", e1, e2, 1, (5.0, 2.0 + HY + 0.005), 0.0, (5.0, 2.0 + HY + 0.005), 0.0)
    add("zero motion, overlapping", e1, e2, 0, (5.0, 2.2), 0.4, (5.0, 2.2), 0.4)
    add("leg descends flat and ends exactly at the target distance", e1, e2, 1, (5.0, 2.0 + HY + 0.3), 0.0, (5.0, 2.0 + HY + ref.TARGET), 0.0)
    add("tilted leg ends exactly at the target distance", e1, e2, 1, (5.0, 2.0 - _leg_lowest(np.float32(0.4))[1] + 0.25), 0.4,
        (5.0, 2.0 - _leg_lowest(np.float32(0.4))[1] + ref.TARGET), 0.4)
    add("leg descends flat through the edge", e1, e2, 1, (5.0, 2.0 + HY + 0.3), 0.0, (5.0, 2.0 + HY - 0.1), 0.0)
    add("lander descends and turns through the edge", e1, e2, 0, (5.0, 2.8), 0.3, (5.1, 2.35), 0.4)
    add("leg descends next to x = 0", (0.0, 1.0), (2.0, 1.2), 1, (0.03, 1.0 + HY + 0.3), 0.0, (0.03, 1.0 + HY - 0.1), 0.05)
    add("lander descends across x = 0", (0.0, 1.0), (2.0, 1.2), 0, (0.1, 1.9), 0.1, (0.0, 1.45), 0.15)
    add("leg descends next to x = 20", (18.0, 1.5), (20.0, 1.0), 1, (19.97, 1.0 + HY + 0.3), 0.05, (19.97, 1.0 + HY - 0.1), 0.0)
    add("lander descends across x = 20", (18.0, 1.5), (20.0, 1.0), 0, (19.9, 1.9), -0.1, (20.0, 1.45), -0.15)
    cols = np.array(rows, np.float64).T
    return names, _pack(cols, cols[4].astype(np.uint32))


# the sets the tests run: name -> (probe kind, cases)
@functools.lru_cache(maxsize=None)
def cases(name):
    return {"distance": lambda: random_static(20260101), "manifold": lambda: random_static(20260102), "toi": lambda: random_sweeps(20260103),
            "hand_static": lambda: hand_static()[1], "hand_sweeps": lambda: hand_sweeps()[1]}[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 reference of a set, computed once per process and never modified."""
    c = cases(name)
    return ref.SweepRef(c) if c.shape[0] == 11 else ref.StaticRef(c)
