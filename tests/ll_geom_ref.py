"""Float64 reference for LunarLander's collision geometry, from the numbers alone: plain numpy, nothing from the engine, the
oracle or Box2D.  Distances between a segment and a convex polygon, their minimum along a linear sweep, and the polygons' area,
centroid and second moment by the shoelace formulas.  Inputs are the f32 values the probes receive (mgym_ll_geom_probe,
ora_b2_geom_probe, tests/native/ll_geom_check.cpp); rotations are float64 sin / cos of the f32 angle.

Shapes come from the reference's own constants (src/box_2d/lunar_lander.rs)."""
import numpy as np

SCALE = 30.0                                                                            # lunar_lander.rs:32
LANDER_POLY = ((-14.0, 17.0), (-17.0, 0.0), (-17.0, -10.0), (17.0, -10.0), (17.0, 0.0), (14.0, 17.0))   # :39-46
LEG_W, LEG_H = 2.0, 8.0                                                                 # :49-50, set_as_box(LEG_W / SCALE, LEG_H / SCALE) :875
DENSITY = (5.0, 1.0)                                                                    # lander :836, leg :879

# Box2D's constants (b2_common.h, b2_time_of_impact.cpp), as csrc/ll_b2.h has them
RADIUS = 0.02        # both polygon radii (2 * b2_polygonRadius): contact points exist up to this plane distance
TARGET = 0.005       # b2TimeOfImpact: max(linearSlop, totalRadius - 3 linearSlop)
TOL = 0.00125        # 0.25 * linearSlop


def shape_points_f32(pi):
    """The shape's defining points as the reference computes them: f32 constants divided by the f32 SCALE."""
    s = np.float32(SCALE)
    if pi == 0:
        return np.array(LANDER_POLY, np.float32) / s
    hx, hy = np.float32(LEG_W) / s, np.float32(LEG_H) / s
    return np.array([(-hx, -hy), (hx, -hy), (hx, hy), (-hx, hy)], np.float32)


def convex_hull_ccw(pts):
    """Andrew's monotone chain; counter-clockwise, collinear points dropped."""
    p = sorted(map(tuple, np.asarray(pts, np.float64)))

    def half(seq):
        h = []
        for q in seq:
            while len(h) >= 2 and (h[-1][0] - h[-2][0]) * (q[1] - h[-2][1]) - (h[-1][1] - h[-2][1]) * (q[0] - h[-2][0]) <= 0:
                h.pop()
            h.append(q)
        return h[:-1]
    return np.array(half(p) + half(p[::-1]), np.float64)


def shape(pi):
    """Counter-clockwise float64 hull of the shape's f32 points."""
    return convex_hull_ccw(shape_points_f32(pi))


def polygon_mass(V, density):
    """mass, centroid, second moment about the centroid: shoelace formulas over the counter-clockwise polygon V."""
    x, y = V[:, 0], V[:, 1]
    xn, yn = np.roll(x, -1), np.roll(y, -1)
    cr = x * yn - xn * y
    area = 0.5 * cr.sum()
    cx, cy = ((x + xn) * cr).sum() / (6.0 * area), ((y + yn) * cr).sum() / (6.0 * area)
    i_origin = density * (cr * (x * x + x * xn + xn * xn + y * y + y * yn + yn * yn)).sum() / 12.0
    mass = density * area
    return mass, np.array([cx, cy]), i_origin - mass * (cx * cx + cy * cy)


def cross(u, v):
    return u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]


def dot(u, v):
    return u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]


def pt_seg(p, a, b):
    """Distance from point p to segment a-b (a == b allowed)."""
    ab, ap = b - a, p - a
    den = dot(ab, ab)
    t = np.clip(dot(ap, ab) / np.where(den > 0.0, den, 1.0), 0.0, 1.0)
    d = ap - t[..., None] * ab
    return np.sqrt(dot(d, d))


def seg_seg(a, b, c, d):
    """Distance between segments a-b and c-d: 0 if they cross, otherwise an end point of one is closest to the other."""
    crossing = (cross(b - a, c - a) * cross(b - a, d - a) < 0.0) & (cross(d - c, a - c) * cross(d - c, b - c) < 0.0)
    m = np.minimum(np.minimum(pt_seg(a, c, d), pt_seg(b, c, d)), np.minimum(pt_seg(c, a, b), pt_seg(d, a, b)))
    return np.where(crossing, 0.0, m)


def in_poly(p, W):
    """p inside or on the counter-clockwise convex polygon W [..., m, 2]."""
    Wn = np.roll(W, -1, -2)
    return (cross(Wn - W, p[..., None, :] - W) >= 0.0).all(-1)


def pt_poly(p, W):
    """Distance from point p to the SOLID convex polygon W."""
    d = pt_seg(p[..., None, :], W, np.roll(W, -1, -2)).min(-1)
    return np.where(in_poly(p, W), 0.0, d)


def seg_poly_by_edges(a, b, W):
    """The definition: 0 if segment a-b and the solid polygon intersect, otherwise the minimum over the polygon's edges."""
    d = seg_seg(a[..., None, :], b[..., None, :], W, np.roll(W, -1, -2)).min(-1)
    return np.where(in_poly(a, W) | in_poly(b, W), 0.0, d)


def seg_poly(a, b, W):
    """The same distance with fewer point-segment evaluations (the sweeps call it ~10^7 times): when nothing intersects, the minimum
    is reached at a polygon vertex against the segment or at a segment end against the polygon."""
    Wn = np.roll(W, -1, -2)
    a1, b1 = a[..., None, :], b[..., None, :]
    sa, sb = cross(Wn - W, a1 - W), cross(Wn - W, b1 - W)
    s = cross(b1 - a1, W - a1)
    hit = ((sa * sb < 0.0) & (s * np.roll(s, -1, -1) < 0.0)).any(-1) | (sa >= 0.0).all(-1) | (sb >= 0.0).all(-1)
    d = np.minimum(pt_seg(W, a1, b1).min(-1), np.minimum(pt_seg(a1, W, Wn).min(-1), pt_seg(b1, W, Wn).min(-1)))
    return np.where(hit, 0.0, d)


def world(V, p, angle):
    """Polygon V [m, 2] at pose (p, angle): [..., m, 2]."""
    c, s = np.cos(angle)[..., None], np.sin(angle)[..., None]
    return np.stack([c * V[:, 0] - s * V[:, 1] + p[..., 0, None], s * V[:, 0] + c * V[:, 1] + p[..., 1, None]], -1)


def sweep_pose(lc, c0, a0, c, a, t):
    """b2Sweep as a formula: centre and angle linear in t, origin p(t) = c(t) - R(a(t)) lc."""
    ct = (1.0 - t)[..., None] * c0 + t[..., None] * c
    at = (1.0 - t) * a0 + t * a
    cs, sn = np.cos(at), np.sin(at)
    return ct - np.stack([cs * lc[0] - sn * lc[1], sn * lc[0] + cs * lc[1]], -1), at


def fp_slack(M):
    """16 spacings of float32 at the case's largest absolute coordinate: each world vertex carries a few ulp(M) from the
    transform, and the results are differences and convex combinations of those."""
    return 16.0 * np.spacing(np.asarray(M, np.float32)).astype(np.float64)


class StaticRef:
    """Distance and end-point clearances of static cases: columns v1.xy v2.xy pi p.xy angle (f32)."""

    def __init__(self, cases):
        c = cases.astype(np.float64)
        n = cases.shape[1]
        self.pi = (cases[4].view(np.uint32) & 1).astype(int)
        self.v1, self.v2 = c[0:2].T.copy(), c[2:4].T.copy()
        self.p, self.angle = c[5:7].T.copy(), c[7].copy()
        self.d = np.zeros(n)
        self.end_clear = np.zeros(n)          # min distance of the edge's end points from the polygon
        self.M = np.zeros(n)
        self.W = [None] * n
        for pi in (0, 1):
            k = np.nonzero(self.pi == pi)[0]
            if not len(k):
                continue
            W = world(shape(pi), self.p[k], self.angle[k])
            self.d[k] = seg_poly(self.v1[k], self.v2[k], W)
            self.end_clear[k] = np.minimum(pt_poly(self.v1[k], W), pt_poly(self.v2[k], W))
            self.M[k] = np.maximum(np.abs(W).max((-1, -2)), np.abs(c[0:4, k]).max(0))
            for j, w in zip(k, W):
                self.W[j] = w
        self.fp = fp_slack(self.M)
        self.interior = self.end_clear > 0.1


def seg_poly_clear(a, b, W):
    """(seg_poly(a, b, W), min(pt_poly(a, W), pt_poly(b, W))) sharing the point-segment evaluations."""
    Wn = np.roll(W, -1, -2)
    a1, b1 = a[..., None, :], b[..., None, :]
    sa, sb = cross(Wn - W, a1 - W), cross(Wn - W, b1 - W)
    s = cross(b1 - a1, W - a1)
    a_in, b_in = (sa >= 0.0).all(-1), (sb >= 0.0).all(-1)
    hit = ((sa * sb < 0.0) & (s * np.roll(s, -1, -1) < 0.0)).any(-1) | a_in | b_in
    da, db = pt_seg(a1, W, Wn).min(-1), pt_seg(b1, W, Wn).min(-1)
    d = np.minimum(pt_seg(W, a1, b1).min(-1), np.minimum(da, db))
    return np.where(hit, 0.0, d), np.minimum(np.where(a_in, 0.0, da), np.where(b_in, 0.0, db))


class SweepRef:
    """Sampled distance along sweeps: columns v1.xy v2.xy pi c0.xy a0 c.xy a (f32).  No vertex moves more than h <= TOL / 4
    between samples (it moves at most |c - c0| + |a - a0| r_max over the whole sweep), and the distance is 1-Lipschitz in
    vertex motion, so the continuous minimum is >= the sampled minimum - h.

    Two levels, for speed.  Every FINE-th sample is always evaluated (coarse spacing H = FINE h).  The samples inside a coarse
    interval are evaluated only where they can matter: where an end of the interval is within CUT + H / 2 of the edge and the
    running minimum has not reached 0 yet.  Elsewhere they are entered as min(ends) - H / 2 — a lower bound of their value by the
    same Lipschitz argument, and above CUT.  CUT lies above every threshold the tests compare with (the largest is
    TARGET + TOL + fp + h < 0.0066), so each comparison comes out as with all samples evaluated.  The end-point clearances
    (`interior`: > 0.1 at every sample) are decided the same way."""
    FINE = 16
    CUT = 0.012

    def __init__(self, cases, chunk_poses=1 << 17):
        c = cases.astype(np.float64)
        n = cases.shape[1]
        F = self.FINE
        self.n = n
        self.pi = (cases[4].view(np.uint32) & 1).astype(int)
        self.v1, self.v2 = c[0:2].T.copy(), c[2:4].T.copy()
        self.c0, self.a0, self.c1, self.a1 = c[5:7].T.copy(), c[7].copy(), c[8:10].T.copy(), c[10].copy()
        self.V = [shape(0), shape(1)]
        self.lc = [polygon_mass(V, 1.0)[1] for V in self.V]
        rmax = np.array([np.sqrt(((V - lc) ** 2).sum(1)).max() for V, lc in zip(self.V, self.lc)])
        travel = np.sqrt(((self.c1 - self.c0) ** 2).sum(1)) + np.abs(self.a1 - self.a0) * rmax[self.pi]
        nc = np.maximum(2, np.ceil(travel / (F * TOL / 4.0)).astype(int) + 1)   # coarse samples
        self.N = (nc - 1) * F + 1                                               # samples
        self.h = travel / (self.N - 1)
        assert (self.h <= TOL / 4.0).all()
        self.runmin = [None] * n               # running minimum over the samples
        self.min_all = np.zeros(n)
        self.interior = np.zeros(n, bool)      # both edge end points > 0.1 from the polygon at every sample
        self.M = np.zeros(n)
        self.evaluated = 0
        for pi in (0, 1):
            idx = np.nonzero(self.pi == pi)[0]
            idx = idx[np.argsort(nc[idx], kind="stable")]
            at = 0
            while at < len(idx):
                stop = at + 1
                while stop < len(idx) and (stop - at + 1) * nc[idx[stop]] * F <= chunk_poses:
                    stop += 1
                k = idx[at:stop]
                at = stop
                ncm = nc[k].max()
                # every case of the chunk on its own coarse grid, padded by repeating t = 1
                j = np.minimum(np.arange(ncm)[None, :], (nc[k] - 1)[:, None])
                d, clear, M = self._eval(pi, k[:, None], j / (nc[k] - 1)[:, None])
                self.M[k] = M.max(1)
                H = (travel[k] / (nc[k] - 1))[:, None]
                valid = np.arange(ncm - 1)[None, :] < (nc[k] - 1)[:, None]
                lo = np.minimum(d[:, :-1], d[:, 1:])
                live = np.minimum.accumulate(d, 1)[:, :-1] > 0.0
                clo = np.minimum(clear[:, :-1], clear[:, 1:])
                maybe_interior = clear.min(1) > 0.1
                refine = valid & ((live & (lo <= self.CUT + H / 2)) | (maybe_interior[:, None] & (clo <= 0.1 + H / 2)))
                lb = np.repeat(np.maximum(lo - H / 2, 0.0), F, 1)
                lb[:, ::F] = d[:, :-1]
                lb = np.concatenate([lb, d[:, -1:]], 1)
                rr, jj = np.nonzero(refine)
                clear_min = clear.min(1)
                if len(rr):
                    q = np.arange(1, F)[None, :]
                    dd, cc, _ = self._eval(pi, k[rr][:, None], (jj[:, None] + q / F) / (nc[k[rr]] - 1)[:, None])
                    lb[rr[:, None], jj[:, None] * F + q] = dd
                    np.minimum.at(clear_min, rr, cc.min(1))
                rm = np.minimum.accumulate(lb, 1)
                for row, kk in enumerate(k):
                    self.runmin[kk] = rm[row, :self.N[kk]].copy()
                self.min_all[k] = rm[:, -1]
                self.interior[k] = clear_min > 0.1
        self.d0 = np.array([r[0] for r in self.runmin])
        self.fp = fp_slack(self.M)

    def _eval(self, pi, k, t):
        k, t = np.broadcast_arrays(k, t)
        self.evaluated += k.size
        p, ang = sweep_pose(self.lc[pi], self.c0[k], self.a0[k], self.c1[k], self.a1[k], t)
        W = world(self.V[pi], p, ang)
        d, clear = seg_poly_clear(self.v1[k], self.v2[k], W)
        M = np.maximum(np.abs(W).max((-1, -2)), np.maximum(np.abs(self.v1[k]).max(-1), np.abs(self.v2[k]).max(-1)))
        return d, clear, M

    def at(self, t):
        """d_ref at each case's own time t [n]."""
        out = np.zeros(self.n)
        for pi in (0, 1):
            k = np.nonzero(self.pi == pi)[0]
            if len(k):
                out[k] = self._eval(pi, k, np.asarray(t, np.float64)[k])[0]
        return out

    def min_until(self, t):
        """min over the samples s <= t and s = t itself."""
        t = np.asarray(t, np.float64)
        j = np.floor(np.clip(t, 0.0, 1.0) * (self.N - 1)).astype(int)
        return np.minimum(np.array([r[q] for r, q in zip(self.runmin, j)]), self.at(t))
