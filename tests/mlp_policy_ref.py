"""Shared by test_mlp_policy_host.py and the GPU suites of mgym_rollout_mlp: the restatement of tests/mlp_ref.py on one observation, and the build of
tests/native/mlp_policy_check.cpp — modurl_gym_amd/csrc/mlp_policy.h compiled for the host — as a program and as a shared object.  No test here."""
import ctypes as C

import numpy as np

import mlp_ref as M
import native_build
from mlp_ref import FAMILIES, RELU, TANH, n_floats, split  # noqa: F401
from words import words_of

SRC = "mlp_policy_check.cpp"


def mlp_refs(D, A, cont, act, H, policies, obs):
    """m cases of one shape at once: policies [m, n_floats], obs [m, D] -> (action words [m], scores [m, A], hidden pre-activations [m, H])"""
    s, pres = M.scores(np.asarray(policies, np.float32).T, D, A, H, np.asarray(obs, np.float32).T, act, want_pre=True)
    return (words_of(s[0]) if cont else M.argmax_words(s)), s.T, pres.T


def mlp_ref(D, A, cont, act, H, policy, o):
    """-> (action word, scores as Python floats, hidden pre-activations) for one observation o [D]"""
    a, s, pres = mlp_refs(D, A, cont, act, H, [policy], [o])
    return int(a[0]), [float(v) for v in s[0]], [float(v) for v in pres[0]]


def check_program():
    return native_build.program(SRC)


def header_eval():
    """the header's bulk form: fn(D, A, cont, act, H, policy, obs [D][stride], n, stride, actions [n], scores [n][A] or None) -> 0"""
    fn = C.CDLL(native_build.shared(SRC)).mlp_policy_eval
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * 5 + [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    return fn


def header_actions(fn, D, A, cont, act, H, policy, obs):
    """actions of the host-compiled header for an SoA observation [D, n]"""
    obs = np.ascontiguousarray(obs, np.float32)
    pol = np.ascontiguousarray(policy, np.float32)
    n = obs.shape[1]
    out = np.zeros(n, np.uint32)
    assert obs.shape[0] == D and pol.size == n_floats(D, A, H)
    assert fn(D, A, cont, act, H, pol.ctypes.data, obs.ctypes.data, n, n, out.ctypes.data, None) == 0
    return out
