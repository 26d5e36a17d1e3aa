"""MGYM_ACT_TANH_FAST restated from the text of include/mgym.h (not from csrc/mgym_math.h), shared by test_tanh_fast_host.py, test_mlp_tanh_fast_host.py,
test_gpu_tanh_fast_probe.py and test_gpu_mlp_tanh_fast.py.  No test here.

 * tanh_fast — the definition on numpy float32 arrays, one rounded operation per line.  Every fmaf is ONE correctly rounded operation: glibc's fmaf over
   arrays through ctypes (glibc_fmaf_arrays of tests/native/tanh_fast_check.cpp).  Python 3.10 has no math.fma, and an f64 product and sum rounded once
   more to f32 rounds twice (tests/mlp_policy_ref.py says the same of the policy's chains).
 * mlp_scores — the hidden-layer policy's fmaf chains of mgym_rollout_mlp with this activation, over an observation [D, n].
 * policy_actions — the action words of the three entry points from those scores: the argmax (or the score's bits), the categorical draw of
   tests/mlp_sample_ref.py, the Gaussian draw of tests/mlp_gauss_ref.py.
 * the build of tests/native/tanh_fast_check.cpp — csrc/mgym_math.h compiled for the host — as a shared object: header_tanh_fast, enumerate_all.
 * the build of tests/native/mlp_tanh_fast_check.cpp — csrc/mlp_policy.h with ACT = MLP_ACT_TANH_FAST compiled for the host: header_policy_actions.
"""
import ctypes as C
import os
import subprocess

import numpy as np

import mlp_gauss_ref as G
import mlp_sample_ref as S
from mlp_policy_ref import n_floats, split  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "native", "_build")
SRC = os.path.join(ROOT, "tests", "native", "tanh_fast_check.cpp")
MLP_SRC = os.path.join(ROOT, "tests", "native", "mlp_tanh_fast_check.cpp")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"]
F = np.float32
TANH_FAST = 3   # MGYM_ACT_TANH_FAST
ARGMAX, SAMPLE, GAUSS = range(3)   # the three entry points: mgym_rollout_mlp, _mlp_sample, _mlp_gauss
# (D, A) of the families: A = 1 are the continuous ones, whose drawn form is GAUSS; the others draw with SAMPLE
FAMILIES = {"cartpole": (4, 2), "mountain_car": (2, 3), "mountain_car_continuous": (2, 1), "pendulum": (3, 1), "acrobot": (6, 3), "lunar_lander": (8, 4)}
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


_shared = None


def build_shared():
    global _shared
    if _shared is None:
        os.makedirs(BUILD, exist_ok=True)
        so = os.path.join(BUILD, "libtanh_fast_check.so")
        subprocess.run(["g++", *FLAGS, "-fopenmp", "-shared", "-fPIC", "-o", so, SRC, "-lm"], check=True)
        lib = C.CDLL(so)
        lib.tanh_fast_enumerate.restype, lib.tanh_fast_enumerate.argtypes = C.c_int, [C.POINTER(Stats)]
        lib.tanh_fast_compare.restype, lib.tanh_fast_compare.argtypes = C.c_uint64, [C.c_uint32, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint32)]
        lib.tanh_fast_bulk.restype, lib.tanh_fast_bulk.argtypes = None, [C.c_uint64, C.c_void_p, C.c_void_p]
        lib.glibc_fmaf_arrays.restype, lib.glibc_fmaf_arrays.argtypes = None, [C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _shared = lib
    return _shared


def fmaf(a, b, c):
    """fmaf(a[i], b[i], c[i]) over float32 arrays (scalars broadcast): one glibc call per element"""
    a, b, c = (np.ascontiguousarray(v, F) for v in np.broadcast_arrays(F(a) if np.isscalar(a) else a, F(b) if np.isscalar(b) else b, F(c) if np.isscalar(c) else c))
    y = np.empty(a.shape, F)
    build_shared().glibc_fmaf_arrays(a.size, a.ctypes.data, b.ctypes.data, c.ctypes.data, y.ctypes.data)
    return y


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


def words_of(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_words(got, exp):
    """equal bit patterns; NaNs are equal as a class"""
    g, e = np.ascontiguousarray(got).view(F), np.ascontiguousarray(exp).view(F)
    return bool(np.all((g.view(np.uint32) == e.view(np.uint32)) | (np.isnan(g) & np.isnan(e))))


def header_tanh_fast(x):
    """mg_tanhf_fast of the host-compiled header over a float32 array (or an array of uint32 words) -> float32"""
    w = np.ascontiguousarray(x).view(np.uint32).ravel()
    out = np.empty(w.size, np.uint32)
    build_shared().tanh_fast_bulk(w.size, w.ctypes.data, out.ctypes.data)
    return out.view(F)


_stats = None


def enumerate_all():
    """the host-compiled header over all 2^31 non-negative patterns (and their negatives) against float64 tanh: computed once per process"""
    global _stats
    if _stats is None:
        st = Stats()
        assert build_shared().tanh_fast_enumerate(C.byref(st)) == 0
        _stats = st
    return _stats


def mlp_scores(policy, D, A, H, obs, activation=None):
    """scores [A, n] of mgym_rollout_mlp with MGYM_ACT_TANH_FAST over an observation [D, n]: the fmaf chains of include/mgym.h in ascending index
    order from the bias, the hidden activation tanh_fast (or `activation`, a function of a float32 array: glibc's tanhf for MGYM_ACT_TANH)"""
    activation = activation or tanh_fast
    w1, b1, w2, b2 = split(policy, D, A, H)
    obs = np.ascontiguousarray(obs, F)
    n = obs.shape[1]
    s = [np.full(n, b2[a], F) for a in range(A)]
    for j in range(H):
        pre = np.full(n, b1[j], F)
        for q in range(D):
            pre = fmaf(w1[j, q], obs[q], pre)
        h = activation(pre)
        for a in range(A):
            s[a] = fmaf(w2[a, j], h, s[a])
    return np.stack(s)


def argmax_words(s):
    """the sequential strict argmax of the text: the first of equal scores wins, a NaN never replaces an earlier score"""
    best, act = s[0].copy(), np.zeros(s.shape[1], np.uint32)
    with np.errstate(all="ignore"):
        for a in range(1, s.shape[0]):
            m = s[a] > best
            best, act = np.where(m, s[a], best).astype(F), np.where(m, np.uint32(a), act).astype(np.uint32)
    return act


def policy_actions(form, policy, D, A, H, obs, sigma=0.0, seed=0, call=0, g=None, t=0, activation=None):
    """-> (action words [n] uint32, scores [A, n]) of env ids g at step t of a call: the restatement"""
    s = mlp_scores(policy, D, A, H, obs, activation)
    if form == ARGMAX:
        return (words_of(s[0]).copy() if A == 1 else argmax_words(s)), s
    if form == SAMPLE:
        assert A > 1
        return S.draw(s, S.words(seed, call, g, t))[0], s
    assert A == 1
    return words_of(G.gauss_actions(s[0], sigma, seed, call, g, t)).copy(), s


_mlp_shared = None


def build_mlp_shared():
    global _mlp_shared
    if _mlp_shared is None:
        os.makedirs(BUILD, exist_ok=True)
        so = os.path.join(BUILD, "libmlp_tanh_fast_check.so")
        subprocess.run(["g++", *FLAGS, "-shared", "-fPIC", "-o", so, MLP_SRC, "-lm"], check=True)
        fn = C.CDLL(so).mlp_tanh_fast_eval
        fn.restype = C.c_int
        fn.argtypes = [C.c_int] * 4 + [C.c_void_p, C.c_float, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _mlp_shared = fn
    return _mlp_shared


def header_policy_actions(form, policy, D, A, H, obs, sigma=0.0, seed=0, call=0, g0=0, t=0):
    """the same from the host-compiled header for the ids g0 .. g0 + n - 1 (SAMPLE, GAUSS: g0 a multiple of 4; GAUSS: n too) -> (action words, scores [A, n])"""
    obs = np.ascontiguousarray(obs, F)
    pol = np.ascontiguousarray(policy, F)
    n = obs.shape[1]
    assert obs.shape[0] == D and pol.size == n_floats(D, A, H)
    words = np.zeros(1, np.uint32)
    if form == SAMPLE:
        words = np.ascontiguousarray(S.words(seed, call, np.uint64(g0) + np.arange(n, dtype=np.uint64), t), np.uint32)
    elif form == GAUSS:
        assert n % 4 == 0 and g0 % 4 == 0
        g4 = np.uint64(g0) + np.uint64(4) * np.arange(n // 4, dtype=np.uint64)
        words = np.ascontiguousarray(np.stack(S.philox4x32_10(g4 & S.M32, g4 >> np.uint64(32), np.uint64(call), np.uint64(G.SLOT_GAUSS + int(t)), int(seed) & 0xFFFFFFFF,
                                                              (int(seed) >> 32) & 0xFFFFFFFF)), np.uint32)
    out, sc = np.zeros(n, np.uint32), np.zeros((n, A), F)
    assert build_mlp_shared()(D, A, form, H, pol.ctypes.data, float(F(sigma)), n, obs.ctypes.data, words.ctypes.data, out.ctypes.data, sc.ctypes.data) == 0
    return out, np.ascontiguousarray(sc.T)
