"""Device half of the collision-geometry pin (see tests/test_ll_geom_host.py): mgym_ll_geom_probe runs LunarLander's b2Distance,
b2TimeOfImpact, b2CollideEdgeAndPolygon + b2WorldManifold and the staged polygon tables of csrc/ll_b2.h on gfx950, one case per lane.
Its output meets the float64 reference of tests/ll_geom_ref.py under the same assertions as the oracle and the host build, at
count = 1, 65 (a ragged tail after one full block) and 8 192 (full blocks), and equals the oracle's probe word for word."""
import ctypes as C

import numpy as np
import pytest

import ll_geom_cases as gc
import ll_geom_checks as ck
from modurl_gym_amd import _lib

pytestmark = pytest.mark.gpu

COUNTS = (1, 65, gc.N_RANDOM)


@pytest.fixture(scope="module")
def polys():
    out = ck.device_probe(ck.SHAPES)
    ck.check_shapes(out, "device")
    assert ck.same(out, ck.oracle_probe(ck.SHAPES))
    return ck.impl_polygons(out)


def _prefix(r, count):
    """the reference of the first `count` cases of a set (the sets' references are computed once and shared)"""
    if count == len(r.fp):
        return r
    import copy
    s = copy.copy(r)
    for k, v in vars(r).items():
        if isinstance(v, np.ndarray) and v.shape[:1] == (len(r.fp),):
            setattr(s, k, v[:count])
        elif isinstance(v, list) and len(v) == len(r.fp):
            setattr(s, k, v[:count])
    s.n = count
    return s


def test_shapes(polys):
    assert [len(p) for p in polys] == [6, 4]


@pytest.mark.parametrize("count", COUNTS)
def test_distance(count):
    out = ck.run_set(ck.device_probe, "distance", ck.DISTANCE, count)
    ck.check_distance(_prefix(gc.reference("distance"), count), out, f"device distance[:{count}]")
    assert ck.same(out, ck.run_set(ck.oracle_probe, "distance", ck.DISTANCE, count))


@pytest.mark.parametrize("count", COUNTS)
def test_manifold(polys, count):
    out = ck.run_set(ck.device_probe, "manifold", ck.MANIFOLD, count)
    ck.check_manifold(_prefix(gc.reference("manifold"), count), out, polys, f"device manifold[:{count}]")
    assert ck.same(out, ck.run_set(ck.oracle_probe, "manifold", ck.MANIFOLD, count))


@pytest.mark.parametrize("count", COUNTS)
def test_time_of_impact(count):
    out = ck.run_set(ck.device_probe, "toi", ck.TOI, count)
    ck.check_toi(_prefix(gc.reference("toi"), count), out, f"device toi[:{count}]")
    assert ck.same(out, ck.run_set(ck.oracle_probe, "toi", ck.TOI, count))


def test_hand_built_cases(polys):
    d = ck.run_set(ck.device_probe, "hand_static", ck.DISTANCE)
    m = ck.run_set(ck.device_probe, "hand_static", ck.MANIFOLD)
    t = ck.run_set(ck.device_probe, "hand_sweeps", ck.TOI)
    ck.check_distance(gc.reference("hand_static"), d, "device hand_static")
    ck.check_manifold(gc.reference("hand_static"), m, polys, "device hand_static", require_parallel=ck.HAND_PARALLEL)
    ck.check_toi(gc.reference("hand_sweeps"), t, "device hand_sweeps")
    # every case and column as bit patterns (no column needs comparing by value: not even the sign of a zero differs)
    assert ck.same(d, ck.run_set(ck.oracle_probe, "hand_static", ck.DISTANCE))
    assert ck.same(m, ck.run_set(ck.oracle_probe, "hand_static", ck.MANIFOLD))
    assert ck.same(t, ck.run_set(ck.oracle_probe, "hand_sweeps", ck.TOI))


def test_probe_rejects_bad_arguments():
    lib = _lib.load()
    dev = C.c_void_p()
    assert lib.mgym_malloc(0, 64 * 60 * 4, C.byref(dev)) == _lib.OK, lib.mgym_last_error()
    try:
        for fn, n, pin, pout in ((_lib.LL_GEOM_TOI + 1, 1, dev, dev), (-1, 1, dev, dev), (_lib.LL_GEOM_DISTANCE, 0, dev, dev),
                                 (_lib.LL_GEOM_DISTANCE, 1, None, dev), (_lib.LL_GEOM_TOI, 1, dev, None), (_lib.LL_GEOM_SHAPES, 1, None, None),
                                 (_lib.LL_GEOM_SHAPES, 2, None, dev), (_lib.LL_GEOM_MANIFOLD, (1 << 31) + 1, dev, dev)):
            assert lib.mgym_ll_geom_probe(0, fn, n, pin, pout) == _lib.ERR_BAD_ARG, (fn, n)
        assert lib.mgym_ll_geom_probe(0, _lib.LL_GEOM_SHAPES, 1, None, dev) == _lib.OK    # SHAPES ignores `in`
    finally:
        lib.mgym_free(0, dev)
