"""Shared by test_mlp_gauss_host.py, test_gpu_gauss_probe.py and test_gpu_mlp_gauss.py: a numpy restatement of the draw of mgym_rollout_mlp_gauss, written
from the text of include/mgym.h ("The draw of z") — numpy float64 for mg_log_u25 (numpy has no fused multiply-add), numpy float32 for the rest, glibc's sinf /
cosf (tests/glibc_f32.py), the block keying of tests/philox_ref.py; mu is tests/mlp_ref.py's one score — the cases the tests share, and the build of
tests/native/mlp_gauss_check.cpp (modurl_gym_amd/csrc/mlp_policy.h compiled for the host) as a shared object.  No test here."""
import ctypes as C
import functools
import math

import numpy as np

import native_build
from glibc_f32 import cosf, sinf
from philox_ref import M32, SLOT_POLICY_GAUSS, block_words

SRC = "mlp_gauss_check.cpp"
F = np.float32
SQRT2 = float.fromhex("0x1.6a09e667f3bcdp+0")
LN2 = float.fromhex("0x1.62e42fefa39efp-1")
R_MAX = 5.8871   # above the largest r = sqrt(-2 ln 2^-25) = sqrt(50 ln 2) = 5.88705...


# ---- the text of include/mgym.h ----
def log_u25(n):
    """mg_log_u25 over an array of odd n in 1 .. 2^25 - 1 -> float64, every operation one numpy float64 operation"""
    x = np.asarray(n, np.uint64).astype(np.float64)
    b = x.view(np.uint64)
    e = ((b >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64) - 1023
    m = ((b & np.uint64((1 << 52) - 1)) | np.uint64(1023 << 52)).view(np.float64)
    big = m > SQRT2
    m = np.where(big, m * 0.5, m)
    e = np.where(big, e + 1, e)
    s = (m - 1.0) / (m + 1.0)
    s2 = s * s
    p = np.full_like(s, 2.0 / 15.0)
    for c in (2.0 / 13.0, 2.0 / 11.0, 2.0 / 9.0, 2.0 / 7.0, 2.0 / 5.0, 2.0 / 3.0, 2.0):
        p = p * s2
        p = p + c
    p = p * s
    t = (e - 25).astype(np.float64) * LN2
    return t + p


def log_reference(n):
    """ln(n 2^-25) in float64 from numpy's log / log1p (each within an ulp): log1p of the exact u1 - 1 near 1, log below 1/2"""
    u = np.asarray(n, np.uint64).astype(np.float64) * 2.0 ** -25
    return np.where(u < 0.5, np.log(u), np.log1p(u - 1.0))


def gauss_pair(wa, wb):
    """-> (z_even, z_odd, q) float32 for arrays of word pairs"""
    wa, wb = np.asarray(wa, np.uint32), np.asarray(wb, np.uint32)
    k1, k2 = wa >> np.uint32(8), wb >> np.uint32(8)
    n = k1.astype(np.uint64) * np.uint64(2) + np.uint64(1)
    L = log_u25(n)
    q = (-2.0 * L).astype(F)
    r = np.sqrt(q)
    assert r.dtype == F
    phi = (k2.astype(F) * F(2.0 ** -24)) * F(6.28318548)
    s, c = sinf(phi), cosf(phi)
    return r * c, r * s, q


def pair_words(seed, call, g, t):
    """(wa, wb, odd) of env g at step t: the pair (w0, w1) for g % 4 in {0, 1}, (w2, w3) for {2, 3}, of
    Philox4x32-10(key = seed; counter = (lo32(g & ~3), hi32(g & ~3), call, 0x60000000 + t)); odd = g % 2"""
    g = np.asarray(g, np.uint64)
    w = block_words(seed, call, g, SLOT_POLICY_GAUSS + int(t))
    second = ((g >> np.uint64(1)) & np.uint64(1)).astype(bool)
    return np.where(second, w[2], w[0]), np.where(second, w[3], w[1]), (g & np.uint64(1)).astype(bool)


def normals(seed, call, g, t):
    """z of env g at step t"""
    wa, wb, odd = pair_words(seed, call, g, t)
    ze, zo, _ = gauss_pair(wa, wb)
    return np.where(odd, zo, ze).astype(F)


def gauss_actions(mu, sigma, seed, call, g, t):
    """a = mu + sigma * z: an f32 multiply, then an f32 add"""
    with np.errstate(all="ignore"):
        sz = F(sigma) * normals(seed, call, g, t)
        return (np.asarray(mu, F) + sz).astype(F)


# ---- the host-compiled header ----
@functools.lru_cache(maxsize=None)
def check_lib():
    lib = C.CDLL(native_build.shared(SRC))
    lib.mlp_gauss_eval.restype, lib.mlp_gauss_eval.argtypes = None, [C.c_uint64] + [C.c_void_p] * 6
    return lib


def header_pair(wa, wb, want_log=False):
    """-> (z_even, z_odd, q[, L]) of the host-compiled header"""
    wa, wb = np.ascontiguousarray(wa, np.uint32), np.ascontiguousarray(wb, np.uint32)
    n = wa.size
    ze, zo, q, L = np.zeros(n, F), np.zeros(n, F), np.zeros(n, F), np.zeros(n, np.float64)
    check_lib().mlp_gauss_eval(n, wa.ctypes.data, wb.ctypes.data, ze.ctypes.data, zo.ctypes.data, q.ctypes.data, L.ctypes.data if want_log else None)
    return (ze, zo, q, L) if want_log else (ze, zo, q)


def lane_words(seed, call, g0, n, t):
    """the words [4, n / 4] of the blocks g0, g0 + 4, .. at step t: what the lane form of the header takes (g0 and n multiples of 4)"""
    assert n % 4 == 0 and g0 % 4 == 0
    g4 = np.uint64(g0) + np.uint64(4) * np.arange(n // 4, dtype=np.uint64)
    return np.ascontiguousarray(np.stack(block_words(seed, call, g4, SLOT_POLICY_GAUSS + int(t))), np.uint32)


# ---- the cases the host test and the probe test share: every k1, k2 a fixed integer hash of k1, and the hand cases ----
K1_HAND = sorted({0, 1, (1 << 23) - 1, 1 << 23, (1 << 24) - 1} | {v for p in range(1, 24) for v in ((1 << p) - 1, (1 << p) + 1) if 0 <= v < (1 << 24)})
K2_HAND = (0, 1 << 22, 1 << 23, 3 << 22, (1 << 24) - 1)   # the axis angles 0, pi/2, pi, 3 pi/2 and the last one below 2 pi: one of s, c is 0 or tiny


def hash_k2(k1):
    """a fixed integer hash (the murmur3 finaliser) of k1, its top 24 bits"""
    h = np.asarray(k1, np.uint64) & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & M32
    h ^= h >> np.uint64(16)
    return (h >> np.uint64(8)).astype(np.uint32)


def all_cases():
    """(wa, wb): every k1 in 0 .. 2^24 - 1 with the hashed k2, then every hand k1 with every hand k2; the low 8 bits of each word vary too (they must not matter)"""
    k1 = np.arange(1 << 24, dtype=np.uint32)
    k2 = hash_k2(k1)
    hk1 = np.repeat(np.array(K1_HAND, np.uint32), len(K2_HAND))
    hk2 = np.tile(np.array(K2_HAND, np.uint32), len(K1_HAND))
    k1, k2 = np.concatenate([k1, hk1]), np.concatenate([k2, hk2])
    return (k1 << np.uint32(8)) | (k1 & np.uint32(0xFF)), (k2 << np.uint32(8)) | ((k2 >> np.uint32(3)) & np.uint32(0xFF))


# ---- the constant policy of the distribution check: W1 = 0, W2 = 0, b2 = 0, so mu = 0 at every observation, and sigma = 1: the action is z ----
DIST_SEED, DIST_CALL, DIST_N, DIST_K = 0x1234567811, 3, 4096, 64


def constant_policy(D, H=1):
    return np.zeros((H, D), F), np.zeros(H, F), np.zeros((1, H), F), np.zeros(1, F)


def dist_actions(seed=DIST_SEED, call=DIST_CALL, n=DIST_N, K=DIST_K, base=0):
    """the restatement's actions [K, n] under the constant policy with sigma = 1"""
    g = np.uint64(base) + np.arange(n, dtype=np.uint64)
    return np.stack([gauss_actions(np.zeros(n, F), 1.0, seed, call, g, t) for t in range(K)])


def dist_deviations(z):
    """z [K, n] with the env id along the last axis -> (mean, variance, pair correlation, Kolmogorov-Smirnov distance), the first three in units of their
    standard errors 1 / sqrt(N), sqrt(2 / N), 1 / sqrt(N / 2), the last multiplied by sqrt(N) (its 5 % critical value is 1.36, 1.95 is the 0.1 % one)"""
    x = np.asarray(z, np.float64)
    N = x.size
    mean = x.mean() * math.sqrt(N)
    var = (x.var() - 1.0) / math.sqrt(2.0 / N)
    ev, od = x[..., 0::2].ravel(), x[..., 1::2].ravel()
    corr = float(np.corrcoef(ev, od)[0, 1]) * math.sqrt(N / 2)
    xs = np.sort(x.ravel())
    cdf = 0.5 * (1.0 + np.vectorize(math.erf)(xs / math.sqrt(2.0)))
    i = np.arange(1, N + 1, dtype=np.float64)
    ks = max(float(np.max(i / N - cdf)), float(np.max(cdf - (i - 1) / N))) * math.sqrt(N)
    return float(mean), float(var), corr, ks
