"""The texts of mgym_gae and mgym_episode_returns (include/mgym.h) restated in numpy, vectorised over environments: every operation a float32 one, fmaf through
glibc (glibc_f32.fmaf), every ?: a np.where on the operand BEFORE the arithmetic.  gae64: the same recurrence with the same selections in float64 and no
rounding to float32 inside (ordinary float64 multiply and add: the reference the float32 words are measured against).  header_*: modurl_gym_amd/csrc/gae.h
compiled by g++ (tests/native/gae_check.cpp).  Input generators shared by the host and the GPU tests.  No test here."""
import ctypes as C

import numpy as np

import glibc_f32
import native_build

F = np.float32
NAN_WORD = 0x7FC0DEAD   # the fill of guards and of words nothing may read or write


def _flags(x, shape):
    return np.zeros(shape, bool) if x is None else (np.asarray(x) != 0)


def gae(reward, done, trunc, value, last_value, final_value, gamma, lam):
    """-> (adv, ret) float32 [K, n]"""
    reward, value = np.asarray(reward, F), np.asarray(value, F)
    K, n = reward.shape
    d, u = _flags(done, (K, n)), _flags(trunc, (K, n))
    gamma, lam = F(gamma), F(lam)
    gl = F(gamma * lam)
    zero = np.zeros(n, F)
    carry, nxt = zero.copy(), np.asarray(last_value, F).copy()
    adv_out, ret_out = np.empty((K, n), F), np.empty((K, n), F)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(K - 1, -1, -1):
            fin = d[t] | u[t]
            fv = zero if final_value is None else np.asarray(final_value[t], F)
            nv = np.where(fin, np.where(d[t], zero, fv), nxt).astype(F)
            c = np.where(fin, zero, carry).astype(F)
            delta = (glibc_f32.fmaf(np.full(n, gamma, F), nv, reward[t]) - value[t]).astype(F)
            adv = glibc_f32.fmaf(np.full(n, gl, F), c, delta)
            adv_out[t], ret_out[t] = adv, (adv + value[t]).astype(F)
            carry, nxt = adv, value[t]
    return adv_out, ret_out


def gae64(reward, done, trunc, value, last_value, final_value, gamma, lam):
    """the float64 form: inputs converted exactly, gamma and lambda the float32 values the call receives, gl their float64 product -> (adv, ret) float64"""
    reward, value = np.asarray(reward, F).astype(np.float64), np.asarray(value, F).astype(np.float64)
    K, n = reward.shape
    d, u = _flags(done, (K, n)), _flags(trunc, (K, n))
    gamma, lam = float(F(gamma)), float(F(lam))
    gl = gamma * lam
    carry, nxt = np.zeros(n), np.asarray(last_value, F).astype(np.float64)
    adv_out, ret_out = np.empty((K, n)), np.empty((K, n))
    for t in range(K - 1, -1, -1):
        fin = d[t] | u[t]
        fv = np.zeros(n) if final_value is None else np.asarray(final_value[t], F).astype(np.float64)
        nv = np.where(fin, np.where(d[t], 0.0, fv), nxt)
        c = np.where(fin, 0.0, carry)
        adv = gl * c + ((gamma * nv + reward[t]) - value[t])
        adv_out[t], ret_out[t] = adv, adv + value[t]
        carry, nxt = adv, value[t]
    return adv_out, ret_out


def episode_returns(reward, done, trunc, ep_return, ep_length, fill=NAN_WORD):
    """-> (ep_return, ep_length, return_out words uint32 [K, n], length_out uint32 [K, n]); the outputs hold `fill` wherever the text writes nothing"""
    reward = np.asarray(reward, F)
    K, n = reward.shape
    fin = _flags(done, (K, n)) | _flags(trunc, (K, n))
    acc, length = np.asarray(ep_return, F).copy(), np.asarray(ep_length, np.uint32).copy()
    ret_out, len_out = np.full((K, n), fill, np.uint32), np.full((K, n), fill, np.uint32)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(K):
            acc = (acc + reward[t]).astype(F)
            length = length + np.uint32(1)
            ret_out[t][fin[t]] = acc.view(np.uint32)[fin[t]]
            len_out[t][fin[t]] = length[fin[t]]
            acc, length = np.where(fin[t], F(0), acc).astype(F), np.where(fin[t], np.uint32(0), length).astype(np.uint32)
    return acc, length, ret_out, len_out


# ---- csrc/gae.h on the host -------------------------------------------------------------------------------------------------------------
_lib = None


def check_lib():
    global _lib
    if _lib is None:
        lib = C.CDLL(native_build.shared("gae_check.cpp"))
        vp = C.c_void_p
        lib.gae_eval.restype, lib.gae_eval.argtypes = C.c_int, [C.c_int32, C.c_uint64, vp, vp, vp, vp, vp, vp, C.c_float, C.c_float, vp, vp]
        lib.ep_eval.restype, lib.ep_eval.argtypes = C.c_int, [C.c_int32, C.c_uint64, vp, vp, vp, vp, vp, vp, vp]
        lib.gae_batch.restype, lib.gae_batch.argtypes = C.c_int, []
        _lib = lib
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data


def _u8(x):
    return None if x is None else np.ascontiguousarray(np.asarray(x) != 0, np.uint8)


def header_gae(reward, done, trunc, value, last_value, final_value, gamma, lam):
    reward, value, last_value = (np.ascontiguousarray(x, F) for x in (reward, value, last_value))
    K, n = reward.shape
    d, u = _u8(done), _u8(trunc)
    fv = None if final_value is None else np.ascontiguousarray(final_value, F)
    adv, ret = np.empty((K, n), F), np.empty((K, n), F)
    assert check_lib().gae_eval(K, n, _p(reward), _p(d), _p(u), _p(value), _p(last_value), _p(fv), float(F(gamma)), float(F(lam)), _p(adv), _p(ret)) == 0
    return adv, ret


def header_episode_returns(reward, done, trunc, ep_return, ep_length, fill=NAN_WORD):
    reward = np.ascontiguousarray(reward, F)
    K, n = reward.shape
    d, u = _u8(done), _u8(trunc)
    acc, length = np.array(ep_return, F), np.array(ep_length, np.uint32)
    ret_out, len_out = np.full((K, n), fill, np.uint32), np.full((K, n), fill, np.uint32)
    assert check_lib().ep_eval(K, n, _p(reward), _p(d), _p(u), _p(acc), _p(length), _p(ret_out), _p(len_out)) == 0
    return acc, length, ret_out, len_out


def batch():
    """kGaeBatch of csrc/gae.h: the steps the four-per-lane kernels load ahead"""
    return check_lib().gae_batch()


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def flags(rng, K, n, p_done=0.08, p_trunc=0.08):
    """done, trunc uint8 [K, n] at the given rates, then the first lanes patched by hand so that every class of check_coverage is present whatever the draw:
    lane 0 (envs 0 .. 3) never ends; lane 1 all four end on step 0 (done only) and on step K - 1 (trunc only); lane 2 mixed: env 8 done only at t = 0, env 9
    trunc only at t = 0, env 10 both at t = 0, env 11 none; lane 3 the same at t = K - 1; lane 4: env 16 done only on every step, env 17 trunc only on every
    step, env 18 both on every step, env 19 alternating done / trunc"""
    assert n >= 20
    d = (rng.random((K, n)) < p_done).astype(np.uint8)
    u = (rng.random((K, n)) < p_trunc).astype(np.uint8)
    d[:, :20], u[:, :20] = 0, 0
    d[0, 4:8] = 1
    u[K - 1, 4:8] = 1
    for base, t in ((8, 0), (12, K - 1)):
        d[t, base], u[t, base + 1] = 1, 1
        d[t, base + 2], u[t, base + 2] = 1, 1
    d[:, 16], u[:, 17] = 1, 1
    d[:, 18], u[:, 18] = 1, 1
    d[0::2, 19], u[1::2, 19] = 1, 1
    return d, u


def check_coverage(d, u):
    """the classes of endings a case claims, asserted on its own flags"""
    d, u = np.asarray(d) != 0, np.asarray(u) != 0
    K, n = d.shape
    classes = {"done only": d & ~u, "trunc only": ~d & u, "both": d & u}
    for name, m in classes.items():
        assert m[0].any() and m[K - 1].any(), f"{name} at t = 0 and at t = K - 1"
        if K > 1:
            assert (m[1:] & m[:-1]).any(), f"{name} on consecutive steps"
    fin = d | u
    per_lane = fin[:, : n // 4 * 4].reshape(K, -1, 4).sum(axis=2)
    assert (per_lane == 4).any(), "all four environments of a lane ending on one step"
    assert ((per_lane > 0) & (per_lane < 4)).any(), "endings mixed within a lane"
    assert (~fin.any(axis=0)).any(), "an environment with no ending at all"


def poisoned_final_value(rng, d, u, lo=-100.0, hi=100.0):
    """final_value: finite where trunc && !done (the only words the text reads), the NaN word everywhere else"""
    d, u = np.asarray(d) != 0, np.asarray(u) != 0
    fv = np.full(d.shape, NAN_WORD, np.uint32).view(F).copy()
    sel = u & ~d
    fv[sel] = rng.uniform(lo, hi, int(sel.sum())).astype(F)
    return fv
