"""No-GPU half of the collision-geometry pin: LunarLander's b2Distance, b2TimeOfImpact, b2CollideEdgeAndPolygon + b2WorldManifold and
the polygon tables / mass data, as the oracle has them (ora_b2_geom_probe) and as the kernel source has them compiled for the host
(tests/native/ll_geom_check.cpp), against a plain float64 reference computed from the numbers alone (tests/ll_geom_ref.py), and word
for word against each other.  Every other LunarLander test compares the kernels with the oracle — a restatement of Box2D from the
same understanding — so an error the two share passes them; this reference shares nothing with either.
tests/test_gpu_ll_geom.py runs the same checks on the device."""
import subprocess

import numpy as np
import pytest

import ll_geom_cases as gc
import ll_geom_checks as ck
import ll_geom_ref as ref

IMPLS = {"oracle": ck.oracle_probe, "host": ck.host_probe}


@pytest.fixture(scope="module", params=sorted(IMPLS))
def impl(request):
    return request.param, IMPLS[request.param]


def test_reference_agrees_with_itself():
    """The fast segment-polygon distance equals its definition (minimum over the polygon's edges, 0 on intersection), and the
    shoelace mass data are the figures the issue gives for orientation."""
    for name in ("distance", "manifold", "hand_static"):
        r = gc.reference(name)
        by_edges = np.array([ref.seg_poly_by_edges(r.v1[i], r.v2[i], r.W[i]) for i in range(len(r.d))])
        assert np.array_equal(by_edges == 0.0, r.d == 0.0) and np.abs(by_edges - r.d).max() <= 1e-15
    for pi, (mass, inv_i) in enumerate(((4.8166666, 1.2757046), (0.07111112, 558.3637))):
        m, _, i_c = ref.polygon_mass(ref.shape(pi), ref.DENSITY[pi])
        assert abs(m / mass - 1.0) < 1e-6 and abs(1.0 / i_c / inv_i - 1.0) < 1e-6


def test_case_sets_cover_the_hard_regimes():
    ck.check_static_regime(gc.reference("distance"), gc.reference("manifold"))
    ck.check_sweep_regime(gc.reference("toi"))


def test_shapes(impl):
    who, probe = impl
    ck.check_shapes(probe(ck.SHAPES), who)


@pytest.mark.parametrize("name", ["distance", "hand_static"])
def test_distance(impl, name):
    who, probe = impl
    ck.check_distance(gc.reference(name), ck.run_set(probe, name, ck.DISTANCE), f"{who} {name}")


@pytest.mark.parametrize("name", ["manifold", "hand_static"])
def test_manifold(impl, name):
    who, probe = impl
    ck.check_manifold(gc.reference(name), ck.run_set(probe, name, ck.MANIFOLD), ck.impl_polygons(probe(ck.SHAPES)), f"{who} {name}",
                      require_parallel=ck.HAND_PARALLEL if name == "hand_static" else 0)


@pytest.mark.parametrize("name", ["toi", "hand_sweeps"])
def test_time_of_impact(impl, name):
    who, probe = impl
    ck.check_toi(gc.reference(name), ck.run_set(probe, name, ck.TOI), f"{who} {name}")


def test_hand_built_sweeps_end_as_constructed():
    """the hand-built sweeps whose answer is known by construction"""
    names, _ = gc.hand_sweeps()
    out = ck.run_set(ck.oracle_probe, "hand_sweeps", ck.TOI)
    state, t = ck.words(out[0]), out[1]
    for i, nm in enumerate(names):
        if "overlap" in nm:
            assert state[i] == ck.TOI_OVERLAPPED, nm
        if "15 m away" in nm or nm == "zero motion, separated":
            assert state[i] == ck.TOI_SEPARATED and t[i] == 1.0, nm
        if nm == "zero motion, inside the target band":
            assert state[i] == ck.TOI_TOUCHING and t[i] == 0.0, nm
        if "exactly at the target distance" in nm:
            assert state[i] == ck.TOI_TOUCHING and t[i] > 0.9, (nm, t[i])
        if "through the edge" in nm:
            assert state[i] == ck.TOI_TOUCHING and 0.0 < t[i] < 1.0, (nm, t[i])


@pytest.mark.parametrize("name,fn", [("distance", ck.DISTANCE), ("manifold", ck.MANIFOLD), ("toi", ck.TOI), ("hand_static", ck.DISTANCE),
                                     ("hand_static", ck.MANIFOLD), ("hand_sweeps", ck.TOI)])
def test_oracle_and_host_build_agree_word_for_word(name, fn):
    """every case and column as bit patterns (no column needs comparing by value: not even the sign of a zero differs)"""
    a, b = ck.run_set(ck.oracle_probe, name, fn), ck.run_set(ck.host_probe, name, fn)
    diff = np.nonzero(ck.words(a) != ck.words(b))
    assert ck.same(a, b), (name, fn, len(diff[0]), diff[0][:8], diff[1][:8])
    assert ck.same(ck.oracle_probe(ck.SHAPES), ck.host_probe(ck.SHAPES))


def test_probes_reject_bad_arguments():
    from oracle import oracle as ora
    import ctypes as C
    lib = ora.lib()
    lib.ora_b2_geom_probe.argtypes = [C.c_int, C.c_uint64, C.c_void_p, C.c_void_p]
    c = gc.cases("hand_static")
    out = np.zeros((60, c.shape[1]), np.float32)
    for fn, n, pin, pout in ((4, 1, c.ctypes.data, out.ctypes.data), (-1, 1, c.ctypes.data, out.ctypes.data), (ck.DISTANCE, 0, c.ctypes.data, out.ctypes.data),
                             (ck.DISTANCE, 1, None, out.ctypes.data), (ck.TOI, 1, c.ctypes.data, None), (ck.SHAPES, 2, None, out.ctypes.data)):
        assert lib.ora_b2_geom_probe(fn, n, pin, pout) == ora.BAD_CONFIG
    assert subprocess.run([ck.host_exe(), "7", "1", "/dev/null", "/dev/null"], capture_output=True).returncode == 2
