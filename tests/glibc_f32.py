"""glibc's float functions for the restatements of include/mgym.h: over float32 arrays through tests/native/glibc_f32.cpp (numpy's own float32 sin / cos /
tanh are not glibc's), and on single floats.  fmaf is ONE correctly rounded operation per element: Python 3.10 has no math.fma, and a float64 product and
sum rounded once more to float32 rounds twice.  No test here."""
import ctypes as C
import ctypes.util

import numpy as np

import native_build

F = np.float32
_lib = None


def _glibc():
    global _lib
    if _lib is None:
        lib = C.CDLL(native_build.shared("glibc_f32.cpp"))
        for name in ("glibc_sinf", "glibc_cosf", "glibc_tanhf", "glibc_expm1f"):
            getattr(lib, name).restype, getattr(lib, name).argtypes = None, [C.c_uint64, C.c_void_p, C.c_void_p]
        lib.glibc_fmodf.restype, lib.glibc_fmodf.argtypes = None, [C.c_uint64, C.c_void_p, C.c_float, C.c_void_p]
        lib.glibc_fmaf.restype, lib.glibc_fmaf.argtypes = None, [C.c_uint64] + [C.c_void_p] * 4
        _lib = lib
    return _lib


def _unary(name, x):
    x = np.ascontiguousarray(x, F)
    y = np.empty_like(x)
    getattr(_glibc(), name)(x.size, x.ctypes.data, y.ctypes.data)
    return y


def sinf(x):
    return _unary("glibc_sinf", x)


def cosf(x):
    return _unary("glibc_cosf", x)


def tanhf(x):
    return _unary("glibc_tanhf", x)


def expm1f(x):
    return _unary("glibc_expm1f", x)


def fmodf(x, m):
    """fmodf(x[i], m) with a scalar m"""
    x = np.ascontiguousarray(x, F)
    y = np.empty_like(x)
    _glibc().glibc_fmodf(x.size, x.ctypes.data, float(F(m)), y.ctypes.data)
    return y


def fmaf(a, b, c):
    """fmaf(a[i], b[i], c[i]) over float32 arrays (scalars broadcast): one glibc call per element"""
    a, b, c = (np.ascontiguousarray(v, F) for v in np.broadcast_arrays(*(F(v) if np.isscalar(v) else v for v in (a, b, c))))
    y = np.empty(a.shape, F)
    _glibc().glibc_fmaf(a.size, a.ctypes.data, b.ctypes.data, c.ctypes.data, y.ctypes.data)
    return y


# ---- on single floats, straight from libm through ctypes: what the array forms are checked against ----
_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expm1f.restype, _libm.expm1f.argtypes = C.c_float, [C.c_float]
_libm.fmaf.restype, _libm.fmaf.argtypes = C.c_float, [C.c_float] * 3


def expm1f_scalar(x):
    return F(_libm.expm1f(float(F(x))))


def fmaf_scalar(a, b, c):
    return F(_libm.fmaf(float(F(a)), float(F(b)), float(F(c))))


def glibc_has_fdlibm_expm1f():
    """glibc replaced the fdlibm expm1f (which mg_expm1f restates) by a correctly rounded one in 2.41: the words of the draw are glibc's only before that"""
    libc = C.CDLL(None)
    libc.gnu_get_libc_version.restype = C.c_char_p
    major, minor = (int(v) for v in libc.gnu_get_libc_version().decode().split(".")[:2])
    return (major, minor) < (2, 41)
