"""The one binding of tests/native/policy_check.cpp — modurl_gym_amd/csrc/mlp_policy.h and mlp2_policy.h compiled for the host: the action call
mlp_actions<D, A, ACT, HEAD, N> of both depths, every activation and every head, as a shared object (header_actions) and as a program (check_program).  The
independent side of every comparison is the numpy restatements (mlp_ref, mlp2_ref, mlp_sample_ref, mlp_gauss_ref, tanh_fast_ref).  No test here."""
import ctypes as C
import functools

import numpy as np

import mlp2_ref
import mlp_gauss_ref
import mlp_ref
import mlp_sample_ref
import native_build

SRC = "policy_check.cpp"
F = np.float32
GREEDY, SAMPLE, GAUSS = range(3)   # MGYM_HEAD_* (= MLP_HEAD_*)


@functools.lru_cache(maxsize=None)
def check_lib():
    lib = C.CDLL(native_build.shared(SRC))
    lib.policy_eval.restype = C.c_int
    lib.policy_eval.argtypes = [C.c_int] * 7 + [C.c_void_p, C.c_float, C.c_uint64, C.c_uint64] + [C.c_void_p] * 4
    return lib


def check_program():
    return native_build.program(SRC)


def header_actions(D, A, depth, act, head, widths, policy, obs, sigma=0.0, seed=0, call=0, g0=0, t=0):
    """the host-compiled header on an SoA observation [D, n] for the ids g0 .. g0 + n - 1 (SAMPLE, GAUSS: g0 a multiple of 4; GAUSS: n too); widths: (H,) or
    (H1, H2) -> (action words [n] uint32, scores [A, n])"""
    obs = np.ascontiguousarray(obs, F)
    pol = np.ascontiguousarray(policy, F)
    n = obs.shape[1]
    H1, H2 = (*widths, 0)[:2]
    assert len(widths) == depth and obs.shape[0] == D
    assert pol.size == (mlp_ref.n_floats(D, A, H1) if depth == 1 else mlp2_ref.n_floats(D, A, H1, H2))
    words = np.zeros(1, np.uint32)
    if head == SAMPLE:
        words = np.ascontiguousarray(mlp_sample_ref.words(seed, call, np.uint64(g0) + np.arange(n, dtype=np.uint64), t), np.uint32)
    elif head == GAUSS:
        words = mlp_gauss_ref.lane_words(seed, call, g0, n, t)
    out, sc = np.zeros(n, np.uint32), np.zeros((n, A), F)
    st = check_lib().policy_eval(D, A, depth, act, head, H1, H2, pol.ctypes.data, float(F(sigma)), n, n, obs.ctypes.data, words.ctypes.data, out.ctypes.data,
                                 sc.ctypes.data)
    assert st == 0, f"policy_eval: status {st} (2: the one-per-lane and the four-per-lane forms of the header differ)"
    return out, np.ascontiguousarray(sc.T)
