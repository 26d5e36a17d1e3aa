"""MGYM_ACT_TANH_FAST restated from the text of include/mgym.h (not from csrc/mgym_math.h), shared by test_tanh_fast_host.py, test_mlp_tanh_fast_host.py,
test_gpu_tanh_fast_probe.py and test_gpu_mlp_tanh_fast.py.  No test here.

 * tanh_fast — the definition on numpy float32 arrays, one rounded operation per line.  Every fmaf is ONE correctly rounded operation: glibc's fmaf over
   arrays (tests/glibc_f32.py).
 * policy_actions — the action words of the three entry points from the scores of tests/mlp_ref.py with this activation: the argmax (or the score's bits), the categorical draw of
   tests/mlp_sample_ref.py, the Gaussian draw of tests/mlp_gauss_ref.py.
 * the build of tests/native/tanh_fast_check.cpp — csrc/mgym_math.h compiled for the host — as a shared object: header_tanh_fast, enumerate_all.
"""
import ctypes as C
import functools

import numpy as np

import mlp_gauss_ref as G
import mlp_ref as M
import mlp_sample_ref as S
import native_build
from glibc_f32 import fmaf
from mlp_ref import TANH_FAST, n_floats
from words import words_of

SRC = "tanh_fast_check.cpp"
F = np.float32
ARGMAX, SAMPLE, GAUSS = range(3)   # the three entry points: mgym_rollout_mlp, _mlp_sample, _mlp_gauss; a continuous family's drawn form is GAUSS, the others' SAMPLE
CLAMP_END = 0x41200100   # just past the clamp: 10.0f is 0x41200000


def fhex(text):
    """the f32 constant a C hexadecimal literal names (each one of the text is exactly an f32)"""
    v = float.fromhex(text)
    assert float(F(v)) == v
    return F(v)


class Stats(C.Structure):
    _fields_ = [("max_ulp", C.c_double), ("max_abs", C.c_double), ("max_ulp_at", C.c_uint32), ("max_abs_at", C.c_uint32), ("max_result", C.c_uint32),
                ("first_one", C.c_uint32), ("inf_result", C.c_uint32), ("n_min", C.c_int32), ("n_max", C.c_int32), ("decreases", C.c_uint64),
                ("nan_not_nan", C.c_uint64), ("not_odd", C.c_uint64), ("negative", C.c_uint64)]


@functools.lru_cache(maxsize=None)
def check_lib(fma=False):
    """tests/native/tanh_fast_check.cpp as a shared object; fma: built with the CPU's own FMA instruction (-mfma) in place of the call of glibc's fmaf"""
    name, extra = ("tanh_fast_check_fma", ("-mfma", "-fopenmp")) if fma else (None, ("-fopenmp",))
    lib = C.CDLL(native_build.shared(SRC, name, extra))
    lib.tanh_fast_enumerate.restype, lib.tanh_fast_enumerate.argtypes = C.c_int, [C.POINTER(Stats)]
    lib.tanh_fast_compare.restype, lib.tanh_fast_compare.argtypes = C.c_uint64, [C.c_uint32, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint32)]
    lib.tanh_fast_bulk.restype, lib.tanh_fast_bulk.argtypes = None, [C.c_uint64, C.c_void_p, C.c_void_p]
    return lib


def n_of(x):
    """n of the text for float32 x"""
    with np.errstate(all="ignore"):
        a = np.abs(np.ascontiguousarray(x, F))
        a = np.where(a < F(10.0), a, F(10.0)).astype(F)
        u = F(-2.0) * a
        return np.rint(u * fhex("0x1.715476p+0")).astype(F)


def tanh_fast(x):
    """the text of include/mgym.h, line by line, on a float32 array"""
    x = np.ascontiguousarray(x, F)
    with np.errstate(all="ignore"):
        a = np.abs(x)
        a = np.where(a < F(10.0), a, F(10.0)).astype(F)           # (an infinity gives 10; so does a NaN, whose result is replaced below)
        u = F(-2.0) * a
        n = np.rint(u * fhex("0x1.715476p+0")).astype(F)     # one f32 multiply, then round to nearest, ties to even
        r = fmaf(n, fhex("-0x1.62e4p-1"), u)
        r = fmaf(n, fhex("-0x1.7f7d1cp-20"), r)
        q = np.full(x.shape, fhex("0x1.a01a02p-13"), F)
        q = fmaf(q, r, fhex("0x1.6c16c2p-10"))
        q = fmaf(q, r, fhex("0x1.111112p-7"))
        q = fmaf(q, r, fhex("0x1.555556p-5"))
        q = fmaf(q, r, fhex("0x1.555556p-3"))
        q = fmaf(q, r, F(0.5))
        p = fmaf(q, r * r, r)
        s = ((np.int32(127) + n.astype(np.int32)).astype(np.uint32) << np.uint32(23)).view(F)
        em = fmaf(s, p, s - F(1.0))
        z = (-em) / (em + F(2.0))
        res = np.copysign(z, x).astype(F)
    return np.where(np.isnan(x), F(np.nan), res).astype(F)


def header_tanh_fast(x):
    """mg_tanhf_fast of the host-compiled header over a float32 array (or an array of uint32 words) -> float32"""
    w = np.ascontiguousarray(x).view(np.uint32).ravel()
    out = np.empty(w.size, np.uint32)
    check_lib().tanh_fast_bulk(w.size, w.ctypes.data, out.ctypes.data)
    return out.view(F)


@functools.lru_cache(maxsize=None)
def enumerate_all():
    """the host-compiled header over all 2^31 non-negative patterns (and their negatives) against float64 tanh: computed once per process"""
    st = Stats()
    assert check_lib().tanh_fast_enumerate(C.byref(st)) == 0
    return st


def policy_actions(form, policy, D, A, H, obs, sigma=0.0, seed=0, call=0, g=None, t=0, activation=None):
    """-> (action words [n] uint32, scores [A, n]) of env ids g at step t of a call: the restatement"""
    s = M.scores(policy, D, A, H, obs, activation or TANH_FAST)
    if form == ARGMAX:
        return (words_of(s[0]).copy() if A == 1 else M.argmax_words(s)), s
    if form == SAMPLE:
        assert A > 1
        return S.draw(s, S.words(seed, call, g, t))[0], s
    assert A == 1
    return words_of(G.gauss_actions(s[0], sigma, seed, call, g, t)).copy(), s
