"""What the collision-geometry probes must satisfy, against the float64 reference of tests/ll_geom_ref.py.  The same checks run on
the oracle's output (ora_b2_geom_probe), on the kernel source compiled for the host (tests/native/ll_geom_check.cpp) and on the
device (mgym_ll_geom_probe).  Every check prints its figures before it asserts.

Slack: fp = 16 spacings of float32 at the case's largest absolute coordinate (ll_geom_ref.fp_slack) — derived, not tuned.  The
other constants are Box2D's (ll_geom_ref.RADIUS / TARGET / TOL); margins that are not are explained where they are used."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import ll_geom_cases as gc
import ll_geom_ref as ref
import native_build
from words import same  # noqa: F401  (exact words: what the probes' outputs are compared by)

SHAPES, DISTANCE, MANIFOLD, TOI = range(4)
IN_COLS = {SHAPES: 0, DISTANCE: 8, MANIFOLD: 8, TOI: 11}
OUT_COLS = {SHAPES: 60, DISTANCE: 3, MANIFOLD: 12, TOI: 2}
SLOTS = 6
U = 2.0 ** -23
TOI_UNKNOWN, TOI_FAILED, TOI_OVERLAPPED, TOI_TOUCHING, TOI_SEPARATED = range(5)
FACE_A, FACE_B = 1, 2
CF_VERTEX, CF_FACE = 0, 1


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def unpack_shapes(out):
    """per polygon: (count, vertices [6, 2], normals [6, 2], mass, invMass, invI, localCenter [2]) of a SHAPES result [60, 1]"""
    res = []
    for p in range(2):
        c = out[p * 30:(p + 1) * 30, 0]
        res.append((int(words(c[0:1])[0]), c[1:13].reshape(SLOTS, 2).copy(), c[13:25].reshape(SLOTS, 2).copy(), c[25], c[26], c[27], c[28:30].copy()))
    return res


def impl_polygons(out):
    """the implementation's vertex lists in ITS order (what contact-feature ids index), float64; valid once check_shapes passed"""
    return [v[:cnt].astype(np.float64) for cnt, v, *_ in unpack_shapes(out)]


def check_shapes(out, who):
    for pi, (cnt, v, nrm, mass, inv_mass, inv_i, lc) in enumerate(unpack_shapes(out)):
        pts, hull = ref.shape_points_f32(pi), ref.shape(pi)
        assert cnt == len(hull) == len(pts), (who, pi, cnt)       # every defining point is a hull vertex
        # the vertex set is the reference's constants / 30, exactly in f32 (compared by value: +0 and -0 are one coordinate)
        assert sorted(map(tuple, v[:cnt].tolist())) == sorted(map(tuple, pts.tolist())), (who, pi, v)
        assert not v[cnt:].any() and not nrm[cnt:].any(), (who, pi)
        V = v[:cnt].astype(np.float64)
        E = np.roll(V, -1, 0) - V
        assert (ref.cross(E, np.roll(E, -1, 0)) > 0.0).all(), (who, pi, "not counter-clockwise and convex")
        n_ref = np.stack([E[:, 1], -E[:, 0]], 1) / np.sqrt(ref.dot(E, E))[:, None]
        N = nrm[:cnt].astype(np.float64)
        err_len, err_dir = np.abs(np.sqrt(ref.dot(N, N)) - 1.0).max(), np.abs(N - n_ref).max()
        m_ref, c_ref, i_ref = ref.polygon_mass(hull, ref.DENSITY[pi])
        rel = {"mass": abs(mass - m_ref) / m_ref, "invMass": abs(inv_mass * m_ref - 1.0), "invI": abs(inv_i * i_ref - 1.0),
               "centroid": np.sqrt(((lc - c_ref) ** 2).sum()) / max(np.sqrt((c_ref ** 2).sum()), 1e-300)}
        print(f"[{who}] shape {pi}: mass {mass!r} invI {inv_i!r} centre {lc.tolist()}; normals: length error {err_len:.2e}, direction error "
              f"{err_dir:.2e} (bound {4 * U:.2e}); relative errors {({k: float(f'{x:.2e}') for k, x in rel.items()})} (bound {16 * U:.2e})")
        assert err_len <= 4 * U and err_dir <= 4 * U, (who, pi)
        assert all(x <= 16 * U for x in rel.values()), (who, pi, rel)


def check_static_regime(r_dist, r_man):
    """conditions decided by the reference alone: a test cannot pass by leaving the hard cases out"""
    d = r_dist.d
    f = {"0 < d < 0.05": np.mean((d > 0.0) & (d < 0.05)), "overlapping": np.mean(d == 0.0), "beyond 0.05": np.mean(d > 0.05),
         "manifold interior": np.mean(r_man.interior)}
    print("static regime:", {k: round(float(x), 4) for k, x in f.items()})
    assert f["0 < d < 0.05"] >= 0.05 and f["overlapping"] >= 0.20 and f["beyond 0.05"] >= 0.20 and f["manifold interior"] >= 0.50, f


def check_sweep_regime(r):
    free = r.d0 > 0.0
    f = {"interior throughout, of non-overlapped": np.mean(r.interior[free]), "min < target - tol": np.mean(r.min_all < ref.TARGET - ref.TOL),
         "min > target + tol": np.mean(r.min_all > ref.TARGET + ref.TOL)}
    print("sweep regime:", {k: round(float(x), 4) for k, x in f.items()}, f"samples {int(r.N.sum())}, evaluated {r.evaluated}, h max {r.h.max():.3e}")
    assert f["interior throughout, of non-overlapped"] >= 0.60 and f["min < target - tol"] >= 0.15 and f["min > target + tol"] >= 0.25, f


def check_distance(r, out, who):
    cold, warm = out[0].astype(np.float64), out[1].astype(np.float64)
    cached = words(out[2])
    e0, e1 = np.abs(cold - r.d), np.abs(warm - r.d)
    print(f"[{who}] distance, {len(cold)} cases: max error cold {e0.max():.3e} warm {e1.max():.3e}; largest error / fp {max((e0 / r.fp).max(), (e1 / r.fp).max()):.3f};"
          f" cold != warm in {int((words(out[0]) != words(out[1])).sum())}; cache sizes {np.bincount(cached, minlength=4).tolist()}")
    assert ((cached >= 1) & (cached <= 3)).all(), who
    for d, e in ((cold, e0), (warm, e1)):
        bad = np.nonzero(e > r.fp)[0]
        assert not len(bad), (who, bad[:8], d[bad[:8]], r.d[bad[:8]])
        # d == 0 <=> d_ref <= fp (cases with 0 < d_ref < fp may go either way)
        assert (r.d[d == 0.0] <= r.fp[d == 0.0]).all() and (d[r.d == 0.0] == 0.0).all(), (who, np.nonzero((r.d == 0.0) & (d != 0.0))[0][:8])


def _unit(v):
    return v / np.sqrt(ref.dot(v, v))[..., None]


def check_manifold(r, out, polys, who, require_parallel=0):
    """polys: impl_polygons() of the same implementation — contact-feature ids index ITS vertex order (check_shapes has shown the
    list to be the reference's point set, counter-clockwise).

    The normal's direction.  The issue words it as "n points from the edge towards the polygon's centroid".  Box2D's rule
    (b2ComputeEdgeSeparation) is to take, of the edge's two normals, the one along which the polygon's overlap is SMALLER; that is
    the centroid's side unless the centroid is within half the shape's asymmetry along the normal of the edge's line (53 of the 4 422
    random FACE_A manifolds, every one of them sunk deeper than 0.47 — the lander hexagon with its centroid nearly on the line).  Asserted here: the exact rule for every FACE_A manifold, the
    centroid's side wherever the reference says the rule implies it, and for FACE_B that n is the inward normal of the polygon
    face the ids name (so it points at the centroid from that face)."""
    n_cases = out.shape[1]
    pc, typ = words(out[0]).astype(int), words(out[1]).astype(int)
    n = out[2:4].T.astype(np.float64)
    P = np.stack([out[4:6].T, out[8:10].T], 1).astype(np.float64)            # [n, 2 points, 2]
    sep = np.stack([out[6], out[10]], 1).astype(np.float64)
    ids = np.stack([words(out[7]), words(out[11])], 1)
    iA, iB, tA, tB = (ids & 255).astype(int), ((ids >> 8) & 255).astype(int), ((ids >> 16) & 255).astype(int), ((ids >> 24) & 255).astype(int)
    has = pc > 0
    assert ((pc >= 0) & (pc <= 2)).all() and np.isin(typ[has], (FACE_A, FACE_B)).all() and (typ[~has] == 0).all(), who
    assert not out[2:, ~has].any() and not out[8:, pc < 2].any(), who      # unused words are 0
    fp = r.fp
    e = _unit(r.v2 - r.v1)
    perp = np.stack([e[:, 1], -e[:, 0]], 1)
    stats = {}

    # points only within the radius.  Margin 1e-4: 0.5 % of the radius and >= 3 fp, fixed beforehand.
    stats["points beyond radius + 1e-4"] = int((has & (r.d > ref.RADIUS + 1e-4)).sum())
    stats["| |n| - 1 | max"] = float(np.abs(np.sqrt(ref.dot(n[has], n[has])) - 1.0).max(initial=0.0))
    bad = {k: [] for k in ("normal", "rule", "centroid", "separation", "separation > 0", "point off the segment", "point off the polygon", "ids", "adjacent")}
    worst_sep = worst_at = 0.0
    twins = 0
    centroid_implied = 0
    for pi in (0, 1):
        V = polys[pi]
        cnt = len(V)
        k = np.nonzero(has & (r.pi == pi))[0]
        if not len(k):
            continue
        W = ref.world(V, r.p[k], r.angle[k])                                    # [m, cnt, 2], implementation's order
        C = ref.world(ref.polygon_mass(ref.shape(pi), 1.0)[1][None, :], r.p[k], r.angle[k])[:, 0]
        v1, v2, ek, nk, fpk = r.v1[k], r.v2[k], e[k], n[k], fp[k]
        face_a = typ[k] == FACE_A
        rows = np.arange(len(k))
        # reference plane normal (pointing out of the reference face) and a point of it
        fidx = np.where(face_a, 0, iA[k, 0]) % cnt
        Wf, Wf2 = W[rows, fidx], W[rows, (fidx + 1) % cnt]
        tf = _unit(Wf2 - Wf)
        nf = np.stack([tf[:, 1], -tf[:, 0]], 1)                                 # outward normal of polygon face fidx (counter-clockwise)
        side = np.where(ref.dot(nk, perp[k]) >= 0.0, 1.0, -1.0)
        n_ref = np.where(face_a[:, None], side[:, None] * perp[k], -nf)        # the world normal: from the edge to the polygon
        # rounding of a unit vector: normalisation (FACE_A), table normal rotated by f32 sin / cos (FACE_B): a few 2^-23 per component
        bad["normal"] += k[np.abs(nk - n_ref).max(1) > 8 * U].tolist()
        h_plus, h_minus = ref.dot(n_ref[:, None, :], W - v1[:, None, :]).min(1), ref.dot(-n_ref[:, None, :], W - v1[:, None, :]).min(1)
        bad["rule"] += k[face_a & (h_plus < h_minus - 2 * fpk)].tolist()
        c_n = ref.dot(n_ref, C - v1)
        ext = ref.dot(n_ref[:, None, :], W - C[:, None, :])
        implied = face_a & (np.abs(ref.dot(perp[k], C - v1)) > np.abs(ext.max(1) + ext.min(1)) / 2 + fpk)
        centroid_implied += int(implied.sum())
        bad["centroid"] += k[(implied & (c_n <= 0.0)) | (~face_a & (ref.dot(nk, C - Wf) <= 0.0))].tolist()
        plane_n, plane_p = np.where(face_a[:, None], n_ref, nf), np.where(face_a[:, None], v1, Wf)
        named = []                                                             # which of the four kinds of pair each id was found to name
        for q in range(2):
            on = pc[k] > q
            a, b, ta, tb = iA[k, q], iB[k, q], tA[k, q], tB[k, q]
            # the point of the feature pair the id names, float64 (nan where the id names no such pair)
            with np.errstate(all="ignore"):
                # FACE_A, (edge face, polygon vertex b): the vertex
                x_a1 = W[rows, b % cnt]
                # FACE_A, (edge vertex a, polygon face b): where the polygon's edge b crosses the perpendicular at the edge's end a
                va = np.where((a == 0)[:, None], v1, v2)
                w1, w2 = W[rows, b % cnt], W[rows, (b + 1) % cnt]
                x_a2 = w1 + (ref.dot(ek, va - w1) / ref.dot(ek, w2 - w1))[:, None] * (w2 - w1)
                # FACE_B, (polygon face a, edge vertex b)
                x_b1 = np.where((b == 0)[:, None], v1, v2)
                # FACE_B, (polygon face a, polygon vertex b of that face): where the edge crosses the face's side plane at vertex b
                wb = W[rows, b % cnt]
                x_b2 = v1 + (ref.dot(tf, wb - v1) / ref.dot(tf, v2 - v1))[:, None] * (v2 - v1)
            cands = []
            for ok, x in ((face_a & (ta == CF_FACE) & (tb == CF_VERTEX) & (a == 0) & (b < cnt), x_a1),
                          (face_a & (ta == CF_VERTEX) & (tb == CF_FACE) & (a <= 1) & (b < cnt), x_a2),
                          (~face_a & (ta == CF_FACE) & (tb == CF_VERTEX) & (b <= 1), x_b1),
                          (~face_a & (ta == CF_FACE) & (tb == CF_VERTEX) & ((b == fidx) | (b == (fidx + 1) % cnt)), x_b2)):
                cands.append(np.where(ok, np.abs(ref.dot(plane_n, x - plane_p) - (sep[k, q] + ref.RADIUS)), np.inf))
            err = np.minimum.reduce(cands)          # (a FACE_B id with indexB <= 1 can name an edge end or a polygon vertex: Box2D's ids do not tell)
            named.append(np.argmin(cands, 0))
            bad["separation"] += k[on & ~(err <= fpk)].tolist()
            if on.any():
                j = np.argmax(np.where(on & np.isfinite(err), err / fpk, -1.0))
                worst_sep = max(worst_sep, float(err[j] / fpk[j]) if np.isfinite(err[j]) else np.inf)
            bad["separation > 0"] += k[on & (sep[k, q] > 0.0)].tolist()
            # the point is the midpoint between the two skins: within |s| / 2 of the segment and of the solid polygon
            s_half = np.abs(sep[k, q] + ref.RADIUS) / 2
            off_seg, off_poly = ref.pt_seg(P[k, q], v1, v2) - s_half, ref.pt_poly(P[k, q], W) - s_half
            bad["point off the segment"] += k[on & (off_seg > fpk)].tolist()
            bad["point off the polygon"] += k[on & (off_poly > fpk)].tolist()
            if on.any():
                worst_at = max(worst_at, float((np.maximum(off_seg, off_poly) / fpk)[on].max()))
        two = pc[k] == 2
        # Two points have different ids — except where Box2D's own ids collide: a FACE_B point is (polygon face, VERTEX b) whether b
        # is an end of the edge or, after clipping, a vertex of that face (b2CollideEdgeAndPolygon swaps the clip point's A and B
        # fields), so the edge's end 0 / 1 and the clip at polygon vertex 0 / 1 carry one id (143 of 3 672 random two-point
        # manifolds).  Then the two ids must have been found to name different pairs.
        twin = two & (ids[k, 0] == ids[k, 1])
        twins += int(twin.sum())
        bad["ids"] += k[twin & (face_a | (named[0] == named[1]))].tolist()
        # FACE_A: both points come from ONE polygon edge — two adjacent vertices, or a vertex and the clip point of the edge that
        # starts at it or at its neighbour
        step = (iB[k, 1] - iB[k, 0]) % cnt
        both_v = (tB[k, 0] == CF_VERTEX) & (tB[k, 1] == CF_VERTEX)
        bad["adjacent"] += k[two & face_a & ~np.where(both_v, (step == 1) | (step == cnt - 1), (step <= 1) | (step == cnt - 1))].tolist()
    # interior cases: both edge ends > 0.1 from the polygon
    inner = r.interior
    stats["interior"] = int(inner.sum())
    missed = np.nonzero(inner & (r.d < ref.RADIUS - 1e-4) & (pc == 0))[0]
    stats["interior within radius - 1e-4 without a point"] = len(missed)
    stats["end-vertex cases within radius - 1e-4 without a point (not asserted: Box2D's clipping)"] = int((~inner & (r.d < ref.RADIUS - 1e-4) & (pc == 0)).sum())
    # a polygon face parallel to the edge (1e-3 rad), wholly over it and within the radius, must give two points
    parallel = np.zeros(n_cases, bool)
    for pi in (0, 1):
        k = np.nonzero(inner & (r.pi == pi))[0]
        if not len(k):
            continue
        W = ref.world(polys[pi], r.p[k], r.angle[k])
        Wn = np.roll(W, -1, 1)
        L = np.sqrt(ref.dot(r.v2[k] - r.v1[k], r.v2[k] - r.v1[k]))[:, None]
        para = np.abs(ref.cross(_unit(Wn - W), e[k][:, None, :])) < np.sin(1e-3)
        h = ref.dot(perp[k][:, None, :], W - r.v1[k][:, None, :])                  # signed heights of the vertices over the edge's line
        u = ref.dot(e[k][:, None, :], W - r.v1[k][:, None, :]) / L                 # their positions along the edge
        hn, un = np.roll(h, -1, 1), np.roll(u, -1, 1)
        sgn = np.sign(h.sum(1))[:, None]
        over = (np.minimum(u, un) > 0.0) & (np.maximum(u, un) < 1.0)
        near = (sgn * h > 0.0) & (sgn * hn > 0.0) & (sgn * h < ref.RADIUS - 1e-4) & (sgn * hn < ref.RADIUS - 1e-4)
        parallel[k] = (para & over & near).any(1) & (sgn * h > 0.0).all(1)      # (the whole polygon on that side: the face is its nearest)
    stats["parallel face within the radius"] = int(parallel.sum())
    stats["... of which without two points"] = int((parallel & (pc != 2)).sum())
    print(f"[{who}] manifold, {n_cases} cases, {int(has.sum())} with points ({int((typ == FACE_A).sum())} face A, {int((typ == FACE_B).sum())} face B), centroid side implied in "
          f"{centroid_implied}, two points with Box2D's ambiguous id {twins}: {stats}; worst separation error / fp {worst_sep:.3f}, worst point offset / fp {worst_at:.3f}; failures { {k: v[:6] for k, v in bad.items() if v} }")
    assert stats["points beyond radius + 1e-4"] == 0 and stats["| |n| - 1 | max"] <= 4 * U, (who, stats)
    assert not any(bad.values()), (who, {k: v[:8] for k, v in bad.items() if v})
    assert len(missed) == 0, (who, missed[:8])
    assert stats["... of which without two points"] == 0 and stats["parallel face within the radius"] >= require_parallel, (who, stats)


def check_toi(r, out, who):
    state, t = words(out[0]).astype(int), out[1].astype(np.float64)
    fp, h = r.fp, r.h
    lo, hi = ref.TARGET - ref.TOL, ref.TARGET + ref.TOL
    counts = np.bincount(state, minlength=5)
    assert counts[TOI_UNKNOWN] == 0 and counts[TOI_FAILED] == 0 and len(counts) == 5, (who, counts)
    assert ((t >= 0.0) & (t <= 1.0)).all() and (t[state == TOI_SEPARATED] == 1.0).all() and (t[state == TOI_OVERLAPPED] == 0.0).all(), who
    d_t = r.at(t)
    min_t = r.min_until(t)
    ov, to, se = state == TOI_OVERLAPPED, state == TOI_TOUCHING, state == TOI_SEPARATED
    bad = {
        "OVERLAPPED but d_ref(0) > fp": ov & (r.d0 > fp),
        "TOUCHING at 0 outside (0, target + tol + fp)": to & (t == 0.0) & ~((r.d0 > 0.0) & (r.d0 < hi + fp)),
        "TOUCHING at t > 0 outside the band": to & (t > 0.0) & ~((d_t >= lo - fp) & (d_t <= hi + fp)),
        "interior TOUCHING at t > 0 that passed below the band before t": r.interior & to & (t > 0.0) & (min_t < lo - fp - h),
        "interior SEPARATED that went below the band": r.interior & se & (r.min_all < lo - fp - h),
        "interior and always above the band, not SEPARATED": r.interior & (r.min_all > hi + fp + h) & ~se,
    }
    outside = ~r.interior & ((to & (t > 0.0) & (min_t < lo - fp - h)) | (se & (r.min_all < lo - fp - h)) | ((r.min_all > hi + fp + h) & ~se))
    print(f"[{who}] time of impact, {len(t)} sweeps: overlapped / touching / separated {counts[2:].tolist()}, touching at t > 0: {int((to & (t > 0)).sum())}, "
          f"interior throughout {int(r.interior.sum())}; non-interior sweeps where conservative advancement is off (printed, not asserted): "
          f"{int(outside.sum())} of {int((~r.interior).sum())}; failures { {k: np.nonzero(v)[0][:6].tolist() for k, v in bad.items() if v.any()} }")
    assert not any(v.any() for v in bad.values()), (who, {k: np.nonzero(v)[0][:8].tolist() for k, v in bad.items() if v.any()})


# ---- running the probes: each returns the output columns [OUT_COLS[fn], n] as float32 words ------------------------------------
def oracle_probe(fn, cases=None):
    from oracle import oracle as ora
    lib = ora.lib()
    lib.ora_b2_geom_probe.argtypes = [C.c_int, C.c_uint64, C.c_void_p, C.c_void_p]
    n = 1 if fn == SHAPES else cases.shape[1]
    out = np.zeros((OUT_COLS[fn], n), np.float32)
    st = lib.ora_b2_geom_probe(fn, n, None if cases is None else cases.ctypes.data, out.ctypes.data)
    assert st == ora.OK, st
    return out


def host_exe():
    return native_build.program("ll_geom_check.cpp")


def host_probe(fn, cases=None):
    n = 1 if fn == SHAPES else cases.shape[1]
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        (cases if cases is not None else np.zeros(0, np.float32)).tofile(fin)
        subprocess.run([host_exe(), str(fn), str(n), fin, fout], check=True)
        return np.fromfile(fout, np.float32).reshape(OUT_COLS[fn], n)


def device_probe(fn, cases=None):
    from modurl_gym_amd import _lib
    lib = _lib.load()
    n = 1 if fn == SHAPES else cases.shape[1]
    out = np.zeros((OUT_COLS[fn], n), np.float32)
    d_in, d_out = C.c_void_p(), C.c_void_p()
    assert lib.mgym_malloc(0, max(4, 0 if cases is None else cases.nbytes), C.byref(d_in)) == _lib.OK, lib.mgym_last_error()
    try:
        assert lib.mgym_malloc(0, out.nbytes, C.byref(d_out)) == _lib.OK, lib.mgym_last_error()
        try:
            if cases is not None:
                assert lib.mgym_memcpy_h2d(0, d_in, cases.ctypes.data, cases.nbytes) == _lib.OK, lib.mgym_last_error()
            assert lib.mgym_ll_geom_probe(0, fn, n, d_in, d_out) == _lib.OK, lib.mgym_last_error()
            assert lib.mgym_memcpy_d2h(0, out.ctypes.data, d_out, out.nbytes) == _lib.OK, lib.mgym_last_error()
        finally:
            lib.mgym_free(0, d_out)
    finally:
        lib.mgym_free(0, d_in)
    return out


SET_FN = {"distance": DISTANCE, "manifold": MANIFOLD, "toi": TOI}
HAND_PARALLEL = 2      # hand_static(): the leg lying flat over the edge at the two gaps inside the radius


def run_set(probe, name, fn, count=None):
    c = gc.cases(name)
    return probe(fn, c if count is None else np.ascontiguousarray(c[:, :count]))
