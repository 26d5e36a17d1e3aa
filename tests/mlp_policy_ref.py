"""Shared by test_mlp_policy_host.py and test_gpu_mlp_policy.py: a Python restatement of the mgym_rollout_mlp policy written from the text of
include/mgym.h (glibc's fmaf and tanhf through ctypes: Python 3.10 has no math.fma, and f64 arithmetic would round twice), and the build of
tests/native/mlp_policy_check.cpp — modurl_gym_amd/csrc/mlp_policy.h compiled for the host — as a program and as a shared object."""
import ctypes as C
import ctypes.util
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "native", "_build")
SRC = os.path.join(ROOT, "tests", "native", "mlp_policy_check.cpp")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"]
RELU, TANH = 0, 1
# (D, A, cont): CartPole, MountainCar, MountainCarContinuous, LunarLander
FAMILIES = {"cartpole": (4, 2, 0), "mountain_car": (2, 3, 0), "mountain_car_continuous": (2, 1, 1), "lunar_lander": (8, 4, 0)}

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_fmaf, _tanhf = _libm.fmaf, _libm.tanhf
_fmaf.restype, _fmaf.argtypes = C.c_float, [C.c_float, C.c_float, C.c_float]
_tanhf.restype, _tanhf.argtypes = C.c_float, [C.c_float]


def n_floats(D, A, H):
    return H * (D + 1) + A * (H + 1)


def split(policy, D, A, H):
    p = np.asarray(policy, np.float32).ravel()
    assert p.size == n_floats(D, A, H)
    return p[: H * D].reshape(H, D), p[H * D: H * D + H], p[H * D + H: H * D + H + A * H].reshape(A, H), p[H * D + H + A * H:]


def bits(x):
    return int(np.float32(x).view(np.uint32))


def mlp_ref(D, A, cont, act, H, policy, o):
    """-> (action word, scores as Python floats, hidden pre-activations): every fmaf one glibc call, in ascending index order from the bias"""
    w1, b1, w2, b2 = split(policy, D, A, H)
    o = [float(v) for v in np.asarray(o, np.float32)]
    s = [float(v) for v in b2]
    pres = []
    for j in range(H):
        pre = float(b1[j])
        for q in range(D):
            pre = _fmaf(float(w1[j, q]), o[q], pre)
        pres.append(pre)
        h = _tanhf(pre) if act == TANH else (pre if pre > 0.0 else 0.0)
        for a in range(A):
            s[a] = _fmaf(float(w2[a, j]), h, s[a])
    if cont:
        return bits(s[0]), s, pres
    best, action = s[0], 0
    for a in range(1, A):
        if s[a] > best:
            best, action = s[a], a
    return action, s, pres


def build_program():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "mlp_policy_check")
    subprocess.run(["g++", *FLAGS, "-o", exe, SRC, "-lm"], check=True)
    return exe


def build_shared():
    """the header's bulk form: fn(D, A, cont, act, H, policy, obs [D][stride], n, stride, actions [n], scores [n][A] or None) -> 0"""
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "libmlp_policy_check.so")
    subprocess.run(["g++", *FLAGS, "-shared", "-fPIC", "-o", so, SRC, "-lm"], check=True)
    fn = C.CDLL(so).mlp_policy_eval
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
