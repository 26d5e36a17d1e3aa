"""Shared by test_mlp_sample_host.py, test_gpu_sample_probe.py and test_gpu_mlp_sample.py: a Python restatement of the draw of mgym_rollout_mlp_sample,
written from the text of include/mgym.h ("The draw") — glibc's expm1f (tests/glibc_f32.py), numpy float32 for the subtraction, the adds and the one multiply,
and the Philox4x32-10 of tests/philox_ref.py, which test_mlp_sample_host.py checks against oracle.oracle.philox — the cases the tests share, and the build of
tests/native/mlp_sample_check.cpp (modurl_gym_amd/csrc/mlp_policy.h compiled for the host) as a shared object and as a program."""
import ctypes as C
import functools
import itertools

import numpy as np

import native_build
from glibc_f32 import expm1f
from philox_ref import SLOT_POLICY_SAMPLE, own_word

SRC = "mlp_sample_check.cpp"


@functools.lru_cache(maxsize=None)
def check_lib():
    """the host-compiled header: lib.mlp_sample_eval(A, n, scores [A][n], words [n], actions [n], cum [A][n] or None) -> 0"""
    lib = C.CDLL(native_build.shared(SRC))
    lib.mlp_sample_eval.restype = C.c_int
    lib.mlp_sample_eval.argtypes = [C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def check_program():
    return native_build.program(SRC, extra=("-fopenmp",))


def words(seed, call, g, t):
    """w of env g at step t: word (g % 4) of Philox4x32-10(key = seed; counter = (lo32(g & ~3), hi32(g & ~3), call, 0x50000000 + t))"""
    return own_word(seed, call, g, SLOT_POLICY_SAMPLE + int(t))


def draw(scores, w):
    """the text of include/mgym.h on scores [A, n] (float32) and words [n] -> (actions [n] uint32, c [A, n] float32)"""
    s = np.ascontiguousarray(scores, np.float32)
    w = np.asarray(w, np.uint32)
    A = s.shape[0]
    with np.errstate(all="ignore"):
        m = s[0].copy()
        for a in range(1, A):
            m = np.where(s[a] > m, s[a], m)
        c = np.empty_like(s)
        for a in range(A):
            e = expm1f(s[a] - m) + np.float32(1.0)
            c[a] = e if a == 0 else c[a - 1] + e
        u = (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
        thr = u * c[A - 1]
        action = np.full(s.shape[1], A - 1, np.uint32)
        for a in range(A - 2, -1, -1):
            action = np.where(thr < c[a], np.uint32(a), action)
    return action, c


def header_draw(scores, w, want_cum=True):
    """the same from the host-compiled header"""
    s = np.ascontiguousarray(scores, np.float32)
    w = np.ascontiguousarray(w, np.uint32)
    A, n = s.shape
    act, cum = np.zeros(n, np.uint32), np.zeros((A, n), np.float32)
    assert check_lib().mlp_sample_eval(A, n, s.ctypes.data, w.ctypes.data, act.ctypes.data, cum.ctypes.data if want_cum else None) == 0
    return act, cum


# ---- the cases the host test and the probe test share ----
SPECIAL_WORDS = (0x00000000, 0xFFFFFFFF, 0xFFFFFF00, 0x000000FF, 0x80000000, 0x7FFFFFFF, 0x00000100, 0x12345678)
GAPS = (16.5, 17.0, 18.0, 104.0)


def seeded_cases(A, count=1 << 16, seed=7):
    """scores uniform in +-20, uniform words"""
    rng = np.random.default_rng(seed + A)
    return rng.uniform(-20.0, 20.0, (A, count)).astype(np.float32), rng.integers(0, 1 << 32, count, dtype=np.uint64).astype(np.uint32)


def hand_score_vectors(A):
    f = np.float32
    vecs = []
    for v in (0.0, -0.0, 1.5, -3.0, 1e30, -1e30):                                  # all scores equal
        vecs.append([v] * A)
    for k in range(2, A + 1):                                                     # ties at the top, in every set of positions
        for pos in itertools.combinations(range(A), k):
            vecs.append([2.0 if a in pos else -1.0 - a for a in range(A)])
    for gap in GAPS:                                                              # exact gaps below the best, the best in every position
        for b in range(A):
            for x in (0.0, 3.25):
                vecs.append([x if a == b else x - gap for a in range(A)])
                vecs.append([x if a == b else (x - gap if a == (b + 1) % A else x - 0.5) for a in range(A)])
    tiny = [0.0, 1e-40, 2e-40, 1e-45, -1e-45, -1e-40, 1.1754944e-38]             # denormal differences
    for combo in itertools.permutations(tiny, A) if A == 2 else itertools.islice(itertools.permutations(tiny, A), 0, None, 7):
        vecs.append(list(combo))
    ulp = float(np.nextafter(f(1.0), f(2.0)))
    vecs += [[1.0 if a != b else ulp for a in range(A)] for b in range(A)]
    rng = np.random.default_rng(99 + A)
    for p in range(A):                                                            # +-inf and NaN in every position
        for v in (np.inf, -np.inf, np.nan):
            for _ in range(3):
                s = list(rng.uniform(-3, 3, A))
                s[p] = v
                vecs.append(s)
    for v, u in itertools.product((np.inf, -np.inf, np.nan), repeat=2):           # two of them, all of them
        for pos in itertools.combinations(range(A), 2):
            s = list(rng.uniform(-3, 3, A))
            s[pos[0]], s[pos[1]] = v, u
            vecs.append(s)
        vecs.append([v] * A)
    with np.errstate(over="ignore"):
        return np.array(vecs, np.float64).astype(np.float32)


def hand_cases(A):
    """every hand-built score vector with every special word -> (scores [A, n], words [n])"""
    v = hand_score_vectors(A)
    w = np.array(SPECIAL_WORDS, np.uint32)
    return np.repeat(v, len(w), axis=0).T.copy(), np.tile(w, len(v))


def gap_sweep_cases(A, count=1 << 20):
    """gaps below the best sweeping (-104, 0] densely: one half linearly under a best in +-8, the other half through every binade from 104 down to the
    denormals under a best of 0 (so the tiny gaps are exact); the best in a random position, every other score one of those gaps below it"""
    rng = np.random.default_rng(1234 + A)
    half = count // 2
    gaps = np.concatenate([-np.linspace(0.0, 104.0, half, endpoint=False), -np.exp2(rng.uniform(-150.0, np.log2(104.0), count - half))])
    best = np.concatenate([rng.uniform(-8.0, 8.0, half), np.zeros(count - half)]).astype(np.float32)
    s = np.empty((A, count), np.float32)
    for a in range(A):
        s[a] = best + np.concatenate([rng.permutation(gaps[:half]), rng.permutation(gaps[half:])]).astype(np.float32)
    s[rng.integers(0, A, count), np.arange(count)] = best
    return s, rng.integers(0, 1 << 32, count, dtype=np.uint64).astype(np.uint32)


# ---- the constant policy of the distribution check: W1 = 0, so the scores are b2 at every observation ----
DIST_B2 = {2: (0.3, -0.9), 3: (0.0, -0.7, 0.4), 4: (0.0, -0.7, 0.4, -2.5)}
DIST_SEED, DIST_CALL, DIST_N, DIST_K = 0x1234567811, 3, 4096, 64


def constant_policy(D, A, H=1):
    """nn.Linear-layout weights whose scores are DIST_B2[A] whatever the observation"""
    return np.zeros((H, D), np.float32), np.zeros(H, np.float32), np.zeros((A, H), np.float32), np.array(DIST_B2[A], np.float32)


def dist_actions(A, seed=DIST_SEED, call=DIST_CALL, n=DIST_N, K=DIST_K, base=0):
    """the restatement's actions [K, n] under the constant policy"""
    s = np.repeat(np.array(DIST_B2[A], np.float32)[:, None], n, axis=1)
    g = base + np.arange(n, dtype=np.uint64)
    return np.stack([draw(s, words(seed, call, g, t))[0] for t in range(K)])


def dist_deviation(actions, A):
    """largest |frequency - softmax| over the actions, in binomial standard deviations sqrt(p (1 - p) / N)"""
    b2 = np.array(DIST_B2[A], np.float64)
    p = np.exp(b2 - b2.max())
    p /= p.sum()
    N = actions.size
    freq = np.bincount(np.asarray(actions).ravel().astype(np.int64), minlength=A)[:A] / N
    return float(np.max(np.abs(freq - p) / np.sqrt(p * (1.0 - p) / N)))
