"""Every f32 bit pattern through the device's sin / cos / tanh (mgym_math_probe: csrc/mgym_math.h compiled for gfx950) against
the host's glibc, the libm the oracle and the Rust reference call.  tests/test_ll_host.py runs the same enumeration on the header
compiled for the host; this one sees what only the device build can get wrong (f32 denormal flushing, contraction or instruction
selection by the device compiler).  Compare rule (tests/native/math_glibc_exhaustive.cpp): NaN meets NaN, everything else bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

import native_build
from modurl_gym_amd import _lib

pytestmark = pytest.mark.gpu

CHUNK = 1 << 26   # patterns per probe launch: 8 result rows of 256 MiB
ROWS = ("sinf", "cosf", "sincosf.sin", "sincosf.cos", "sincosf_u.sin", "sincosf_u.cos", "cosf_u", "tanhf")
# entry point -> first result row (the sincos forms fill two: sin, then cos)
PROBES = ((_lib.MATH_SINF, 0), (_lib.MATH_COSF, 1), (_lib.MATH_SINCOSF, 2), (_lib.MATH_SINCOSF_U, 4), (_lib.MATH_COSF_U, 6), (_lib.MATH_TANHF, 7))
CLASSES = ("|x|<=16", "16<|x|<120", "|x|>=120", "inf/nan")


def _threads():
    return max(1, min(16, len(os.sched_getaffinity(0))))


@pytest.fixture(scope="module")
def glibc_helper():
    if not native_build.host_has_fma():
        pytest.skip("host CPU has no FMA: glibc runs its non-FMA sinf/cosf build, which mgym_math.h does not restate")
    h = C.CDLL(native_build.shared("math_glibc_exhaustive.cpp", "mg_glibc", extra=("-mfma", "-fopenmp", "-DMG_GLIBC_LIB")))
    h.mg_glibc_compare.restype = C.c_uint64
    h.mg_glibc_compare.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_int,
                                   C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    h.mg_glibc_ref_bits.restype = C.c_uint32
    h.mg_glibc_ref_bits.argtypes = [C.c_uint32, C.c_int]
    return h


def test_device_sin_cos_tanh_equal_glibc_on_every_pattern(glibc_helper):
    lib = _lib.load()
    dev = C.c_void_p()
    host = np.empty((len(ROWS), CHUNK), np.uint32)
    assert lib.mgym_malloc(0, host.nbytes, C.byref(dev)) == _lib.OK, lib.mgym_last_error()
    bad_total = np.zeros((len(ROWS), len(CLASSES)), np.uint64)
    first_bad = {}   # row -> [(pattern, device bits, glibc bits)], smallest patterns first
    bad = (C.c_uint64 * (len(ROWS) * 4))()
    fb = (C.c_uint32 * (len(ROWS) * 4))()
    try:
        for first in range(0, 1 << 32, CHUNK):
            for fn, row in PROBES:
                rc = lib.mgym_math_probe(0, fn, first, CHUNK, dev.value + row * CHUNK * 4)
                assert rc == _lib.OK, lib.mgym_last_error()
            assert lib.mgym_memcpy_d2h(0, host.ctypes.data, dev, host.nbytes) == _lib.OK, lib.mgym_last_error()
            if glibc_helper.mg_glibc_compare(first, CHUNK, 1, host.ctypes.data, CHUNK, _threads(), bad, fb) == 0:
                continue
            bad_total += np.frombuffer(bad, np.uint64).reshape(len(ROWS), 4)
            for r in range(len(ROWS)):
                for k in range(4):
                    u = fb[r * 4 + k]
                    if u != 0xFFFFFFFF and len(first_bad.setdefault(r, [])) < 4:
                        first_bad[r].append((u, int(host[r, u - first]), int(glibc_helper.mg_glibc_ref_bits(u, r))))
        # the probe's argument checks
        assert lib.mgym_math_probe(0, _lib.MATH_SINF, 1, 1 << 32, dev) == _lib.ERR_BAD_ARG
        assert lib.mgym_math_probe(0, _lib.MATH_TANHF + 1, 0, 16, dev) == _lib.ERR_BAD_ARG
        assert lib.mgym_math_probe(0, _lib.MATH_SINF, 0, 0, dev) == _lib.ERR_BAD_ARG
    finally:
        lib.mgym_free(0, dev)

    def f32(u):
        return float(np.uint32(u).view(np.float32))
    report = []
    for r, name in enumerate(ROWS):
        if bad_total[r].sum():
            cls = ", ".join(f"{c}: {int(n)}" for c, n in zip(CLASSES, bad_total[r]) if n)
            firsts = "; ".join(f"x={f32(u).hex()} ({u:08x}) device {f32(d).hex()} ({d:08x}) glibc {f32(g).hex()} ({g:08x})"
                               for u, d, g in first_bad.get(r, []))
            report.append(f"{name}: {int(bad_total[r].sum())} mismatches ({cls}); first: {firsts}")
    assert not report, "device math differs from glibc:\n" + "\n".join(report)
