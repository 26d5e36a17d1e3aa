// ll_geom_probe.h — one case of mgym_ll_geom_probe (test seam): the collision-geometry primitives of ll_b2.h called as pure
// functions, one case per lane.  Shared by selftest.hip (gfx950) and tests/native/ll_geom_check.cpp (the same source on the host).
// Columns are SoA, [cols][count]; integer fields travel as bit patterns.  include/mgym.h documents the layout.
#pragma once
#include "ll_env.h"

namespace mgym {

enum { GEOM_SHAPES = 0, GEOM_DISTANCE = 1, GEOM_MANIFOLD = 2, GEOM_TOI = 3, GEOM_FN_COUNT = 4 };
constexpr int kGeomShapeCols = 1 + 4 * kMaxPoly + 5;  // count, vertices, normals, mass, invMass, invI, localCenter
constexpr int geom_in_cols(int fn) { return fn == GEOM_TOI ? 11 : fn == GEOM_SHAPES ? 0 : 8; }
constexpr int geom_out_cols(int fn) { return fn == GEOM_SHAPES ? 2 * kGeomShapeCols : fn == GEOM_DISTANCE ? 3 : fn == GEOM_MANIFOLD ? 12 : 2; }

// `tab`: the staged polygon table, `tmp`: 2 * kMaxPoly vectors of this lane — both LDS on the device (collide_edge_polygon)
template <int FN>
__device__ __forceinline__ void ll_geom_probe_case(const LLConst& k, const PolyTab& tab, V2* tmp, uint64_t count, uint64_t i,
                                                   const float* in, float* out) {
#define GEOM_IN(c) in[(uint64_t)(c) * count + i]
#define GEOM_OUT(c) out[(uint64_t)(c) * count + i]
    if constexpr (FN == GEOM_SHAPES) {
        for (int p = 0; p < 2; ++p) {
            const int c0 = p * kGeomShapeCols;
            GEOM_OUT(c0) = as_f32((uint32_t)tab.count[p]);
            for (int q = 0; q < kMaxPoly; ++q) {
                GEOM_OUT(c0 + 1 + 2 * q) = tab.v[p][q].x; GEOM_OUT(c0 + 2 + 2 * q) = tab.v[p][q].y;
                GEOM_OUT(c0 + 1 + 2 * kMaxPoly + 2 * q) = tab.n[p][q].x; GEOM_OUT(c0 + 2 + 2 * kMaxPoly + 2 * q) = tab.n[p][q].y;
            }
            const int m0 = c0 + 1 + 4 * kMaxPoly;
            GEOM_OUT(m0) = k.mass[p]; GEOM_OUT(m0 + 1) = k.invMass[p]; GEOM_OUT(m0 + 2) = k.invI[p];
            GEOM_OUT(m0 + 3) = k.localCenter[p].x; GEOM_OUT(m0 + 4) = k.localCenter[p].y;
        }
    } else {
        V2 ev[2];
        ev[0] = mk(GEOM_IN(0), GEOM_IN(1)); ev[1] = mk(GEOM_IN(2), GEOM_IN(3));
        const int pi = (int)(as_u32(GEOM_IN(4)) & 1u);
        if constexpr (FN == GEOM_TOI) {
            Sweep sw;
            sw.localCenter = k.localCenter[pi];
            sw.c0 = mk(GEOM_IN(5), GEOM_IN(6)); sw.a0 = GEOM_IN(7);
            sw.c = mk(GEOM_IN(8), GEOM_IN(9)); sw.a = GEOM_IN(10);
            sw.alpha0 = 0.0f;
            float t;
            const int state = time_of_impact(ev, tab, pi, sw, t);
            GEOM_OUT(0) = as_f32((uint32_t)state); GEOM_OUT(1) = t;
        } else {
            Xf xf;
            xf.p = mk(GEOM_IN(5), GEOM_IN(6));
            xf.q = rot_set(GEOM_IN(7));
            if constexpr (FN == GEOM_DISTANCE) {
                SCache cache;
                cache.count = 0; cache.metric = 0.0f;
                const float cold = gjk_distance(cache, ev, tab, pi, xf);
                const int cached = cache.count;
                const float warm = gjk_distance(cache, ev, tab, pi, xf);
                GEOM_OUT(0) = cold; GEOM_OUT(1) = warm; GEOM_OUT(2) = as_f32((uint32_t)cached);
            } else {
                Manifold m;
                m.type = 0; m.pointCount = 0;
                collide_edge_polygon(m, ev[0], ev[1], tab, pi, xf, tmp);
                V2 normal = mk(0.0f, 0.0f), pts[2];
                world_manifold(m, xf, normal, pts);
                GEOM_OUT(0) = as_f32((uint32_t)m.pointCount);
                GEOM_OUT(1) = as_f32(m.pointCount ? (uint32_t)m.type : 0u);
                GEOM_OUT(2) = normal.x; GEOM_OUT(3) = normal.y;
                // separation as b2WorldManifold has it: the clip point's distance from the reference plane minus both radii
                V2 pn = mk(0.0f, 0.0f), pp = pn;  // the reference plane in the ground frame, normal pointing out of the reference face
                if (m.pointCount > 0) {
                    if (m.type == FACE_A) { pn = m.localNormal; pp = m.localPoint; }
                    else { pn = rmul(xf.q, m.localNormal); pp = xmul(xf, m.localPoint); }
                }
                for (int q = 0; q < 2; ++q) {
                    const bool on = q < m.pointCount;
                    float sep = 0.0f;
                    if (on) {
                        const V2 clip = m.type == FACE_A ? xmul(xf, m.points[q].localPoint) : m.points[q].localPoint;
                        sep = (dot(clip - pp, pn) - b2_polygonRadius) - b2_polygonRadius;
                    }
                    GEOM_OUT(4 + 4 * q) = on ? pts[q].x : 0.0f; GEOM_OUT(5 + 4 * q) = on ? pts[q].y : 0.0f;
                    GEOM_OUT(6 + 4 * q) = sep;
                    GEOM_OUT(7 + 4 * q) = as_f32(on ? cf_pack(m.points[q].id) : 0u);
                }
            }
        }
    }
#undef GEOM_IN
#undef GEOM_OUT
}

}  // namespace mgym
