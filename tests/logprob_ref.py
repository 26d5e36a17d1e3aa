"""The text of mgym_logprob_mlp (include/mgym.h) restated in numpy: the scores of mlp_ref.scores / mlp2_ref.scores (glibc fmaf chains in ascending order from the
bias) on the row value_ref.dense_rows gives step t (obs_first, then obs[t - 1]); mg_log_pos operation by operation in float64 (numpy has no fused multiply-add);
the categorical head through mlp_sample_ref.draw's own m and c (glibc expm1f); the Gaussian head in float32 with k from float64.  logp64_*: the same
log-probabilities in float64 from the restatement's f32 scores with numpy's log / exp, what a learner computes up to rounding.  header_logprob_mlp:
modurl_gym_amd/csrc/logprob.h compiled by g++ (tests/native/logprob_check.cpp).  Case generators shared by the host and the GPU tests.  No test here."""
import ctypes as C
import functools

import numpy as np

import families
import mlp2_ref
import mlp_ref
import mlp_sample_ref as S
import native_build
import value_ref

F = np.float32
NAN_WORD = 0x7FC00000   # what the call writes where the action has no log-probability
POISON = value_ref.POISON
RELU, TANH, TANH_FAST = mlp_ref.RELU, mlp_ref.TANH, mlp_ref.TANH_FAST
SAMPLE, GAUSS = mlp2_ref.SAMPLE, mlp2_ref.GAUSS
ACTS, ACT_NAMES, WIDTHS = value_ref.ACTS, value_ref.ACT_NAMES, value_ref.WIDTHS
SQRT2 = float.fromhex("0x1.6a09e667f3bcdp+0")
LN2 = float.fromhex("0x1.62e42fefa39efp-1")
HALF_LOG_2PI = 0.91893853320467274
SIGMA_MIN, SIGMA_MAX = float(2.0 ** -126), float(np.finfo(F).max)
ALL = tuple(families.FAMILIES)   # the six (D, A)
# the restatement's largest distance from the whole network in float64, per head, as test_logprob_host.py measures and records it; the bound is 4 x that
NET64_MEASURED = {SAMPLE: 5.14e-06, GAUSS: 8.95e-06}
NET64_BOUND = {h: 4 * v for h, v in NET64_MEASURED.items()}


def dims(family):
    f = families.FAMILIES[family]
    return f.D, f.A


def head_of(family):
    return GAUSS if families.FAMILIES[family].box is not None else SAMPLE


# ---- the text of include/mgym.h ------------------------------------------------------------------------------------------------------------------
def log_pos(x):
    """mg_log_pos over a float32 array of positive normal values -> float64, every operation one numpy float64 operation; m and e from the bits of (double)x"""
    d = np.ascontiguousarray(x, F).astype(np.float64)
    b = d.view(np.uint64)
    e = ((b >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64) - 1023
    m = ((b & np.uint64((1 << 52) - 1)) | np.uint64(1023 << 52)).view(np.float64)
    with np.errstate(all="ignore"):
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
        t = e.astype(np.float64) * LN2
        return t + p


def logp_discrete(s, act):
    """scores [A, n] float32, action words [n] uint32 -> the words [n] uint32 of logp"""
    s = np.ascontiguousarray(s, F)
    act = np.asarray(act, np.uint32)
    A, n = s.shape
    _, c = S.draw(s, np.zeros(n, np.uint32))   # c_0 .. c_{A-1} of "The draw"
    with np.errstate(all="ignore"):
        m, b = s[0].copy(), np.zeros(n, np.uint32)
        for a in range(1, A):
            up = s[a] > m
            m, b = np.where(up, s[a], m).astype(F), np.where(up, np.uint32(a), b).astype(np.uint32)
        sa = s[np.minimum(act, A - 1).astype(np.int64), np.arange(n)]
        d = np.where(act == b, m - m, sa - m).astype(F)
        lse = log_pos(c[A - 1]).astype(F)
        logp = (d - lse).astype(F)
        ok = (c[A - 1] >= F(1.0)) & (c[A - 1] <= F(A)) & (act < A)
    return np.where(ok, logp.view(np.uint32), np.uint32(NAN_WORD)).astype(np.uint32)


def gauss_k(sigma):
    """k = (float)(-(mg_log_pos(sigma) + 0.91893853320467274))"""
    return F(-(log_pos(np.array([sigma], F))[0] + HALF_LOG_2PI))


def logp_gauss(mu, a, sigma):
    """mu, a [n] float32 -> the words [n] uint32 of logp = k - 0.5f * ((a - mu) / sigma)^2"""
    mu, a = np.ascontiguousarray(mu, F), np.ascontiguousarray(a, F)
    with np.errstate(all="ignore"):
        z = ((a - mu) / F(sigma)).astype(F)
        q = (z * z).astype(F)
        return (gauss_k(sigma) - (F(0.5) * q).astype(F)).astype(F).view(np.uint32)


def n_floats(D, A, widths):
    return mlp_ref.n_floats(D, A, widths[0]) if len(widths) == 1 else mlp2_ref.n_floats(D, A, *widths)


def packed(weights):
    return mlp_ref.packed(weights) if len(weights) == 4 else mlp2_ref.packed(weights)


def row_scores(policy, D, A, widths, act, rows):
    """the scores over observation rows [R, D, n] -> float32 [A, R, n]"""
    rows = np.asarray(rows, F)
    R, n = rows.shape[0], rows.shape[-1]
    flat = np.ascontiguousarray(np.moveaxis(rows, 1, 0).reshape(D, -1))   # [D, R * n]
    s = mlp_ref.scores(policy, D, A, widths[0], flat, act) if len(widths) == 1 else mlp2_ref.scores(policy, D, A, widths[0], widths[1], flat, act)
    return s.reshape(A, R, n)


def acted_rows(obs_first, obs):
    """the K observation rows the policy acted on: row 0 = obs_first, row t = obs[t - 1] (value_ref.dense_rows without its last)"""
    return value_ref.dense_rows(obs_first, obs)[:-1]


def logprob_mlp(policy, D, A, widths, act, obs_first, obs, actions, sigma=0.0):
    """-> the words uint32 [K, n] of logp_out; actions [K, n] uint32 (A > 1) or float32 (A == 1: the Gaussian head)"""
    K, n = np.shape(obs)[0], np.shape(obs)[-1]
    s = row_scores(policy, D, A, widths, act, acted_rows(obs_first, obs)).reshape(A, K * n)
    if A == 1:
        return logp_gauss(s[0], np.ascontiguousarray(actions, F).reshape(-1), sigma).reshape(K, n)
    return logp_discrete(s, np.ascontiguousarray(actions, np.uint32).reshape(-1)).reshape(K, n)


# ---- float64, never the header ---------------------------------------------------------------------------------------------------------------------
def logp64_all(s):
    """log_softmax of f32 scores [A, n] in float64 -> [A, n]"""
    s = np.asarray(s, F).astype(np.float64)
    d = s - s.max(axis=0)
    return d - np.log(np.exp(d).sum(axis=0))


def logp64_discrete(s, act):
    return logp64_all(s)[np.asarray(act, np.int64), np.arange(np.shape(s)[1])]


def logp64_gauss(mu, a, sigma):
    """the Gaussian log-density of f32 mu, a, sigma in float64"""
    mu, a, sg = np.asarray(mu, F).astype(np.float64), np.asarray(a, F).astype(np.float64), float(F(sigma))
    z = (a - mu) / sg
    return -0.5 * z * z - np.log(sg) - 0.5 * np.log(2.0 * np.pi)


def scores64(policy, D, A, widths, act, rows):
    """the whole network in float64 (value_ref.value64 with A outputs): weights and observations converted exactly, numpy dot products, np.tanh for both tanh
    activations; rows [.., D, n] -> float64 [A, .., n].  What a learner's float64 forward pass computes from the same weights"""
    f = (lambda x: np.maximum(x, 0.0)) if act == RELU else np.tanh
    ws = mlp_ref.split(policy, D, A, widths[0]) if len(widths) == 1 else mlp2_ref.split(policy, D, A, *widths)
    ws = [np.asarray(w, np.float64) for w in ws]
    x = np.moveaxis(np.asarray(rows, F).astype(np.float64), -2, -1)   # [.., n, D]
    for k in range(0, len(ws) - 2, 2):
        x = f(x @ ws[k].T + ws[k + 1])
    return np.moveaxis(x @ ws[-2].T + ws[-1], -1, 0)


def logprob64(policy, D, A, widths, act, obs_first, obs, actions, sigma=0.0):
    """logp_out [K, n] in float64 throughout: scores64, then log_softmax + gather or the Gaussian log-density"""
    K, n = np.shape(obs)[0], np.shape(obs)[-1]
    s = scores64(policy, D, A, widths, act, acted_rows(obs_first, obs)).reshape(A, K * n)
    if A == 1:
        z = (np.asarray(actions, F).astype(np.float64).reshape(-1) - s[0]) / float(F(sigma))
        return (-0.5 * z * z - np.log(float(F(sigma))) - 0.5 * np.log(2.0 * np.pi)).reshape(K, n)
    d = s - s.max(axis=0)
    l = d - np.log(np.exp(d).sum(axis=0))
    return l[np.asarray(actions, np.int64).reshape(-1), np.arange(K * n)].reshape(K, n)


# ---- csrc/logprob.h on the host ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def check_lib():
    lib = C.CDLL(native_build.shared("logprob_check.cpp"))
    vp = C.c_void_p
    lib.logprob_eval.restype, lib.logprob_eval.argtypes = C.c_int, [C.c_int] * 6 + [vp, C.c_float, C.c_int32, C.c_uint64] + [vp] * 4
    lib.logprob_k.restype, lib.logprob_k.argtypes = C.c_float, [C.c_float]
    lib.logprob_sigma_ok.restype, lib.logprob_sigma_ok.argtypes = C.c_int, [C.c_float]
    lib.log_pos_eval.restype, lib.log_pos_eval.argtypes = None, [C.c_uint64, vp, vp]
    out = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    lib.log_pos_sweep.restype, lib.log_pos_sweep.argtypes = None, [C.c_uint32, C.c_uint32] + out
    lib.log_pos_stats.restype, lib.log_pos_stats.argtypes = None, [C.c_uint64, vp] + out
    return lib


def header_logprob_mlp(policy, D, A, widths, act, obs_first, obs, actions, sigma=0.0, fill=POISON):
    """logprob.h's logprob_env over every environment, the output pre-filled with `fill` -> words uint32 [K, n]"""
    policy, obs_first, obs = (np.ascontiguousarray(x, F) for x in (policy, obs_first, obs))
    K, n = obs.shape[0], obs.shape[-1]
    assert policy.size == n_floats(D, A, widths) and obs.shape == (K, D, n) and obs_first.shape == (D, n)
    a = np.ascontiguousarray(actions, F if A == 1 else np.uint32)
    assert a.shape == (K, n)
    out = np.full((K, n), fill, np.uint32)
    st = check_lib().logprob_eval(D, A, len(widths), act, widths[0], (*widths, 0)[1], policy.ctypes.data, float(sigma), K, n, obs_first.ctypes.data, obs.ctypes.data,
                                  a.ctypes.data, out.ctypes.data)
    assert st == 0, f"logprob_eval: status {st} (2: the four-per-lane form differs from the one-per-lane form)"
    return out


def header_log_pos(x):
    x = np.ascontiguousarray(x, F)
    out = np.zeros(x.size, np.float64)
    check_lib().log_pos_eval(x.size, x.ctypes.data, out.ctypes.data)
    return out.reshape(x.shape)


def _stats(call):
    a, r, d = C.c_double(), C.c_double(), C.c_uint64()
    call(C.byref(a), C.byref(r), C.byref(d))
    return a.value, r.value, int(d.value)


def log_pos_sweep(first_word, last_word):
    """the header over every f32 pattern first .. last against libm's float64 log -> (largest |error|, largest relative error, roundings to f32 that differ)"""
    return _stats(lambda *o: check_lib().log_pos_sweep(first_word, last_word, *o))


def log_pos_stats(x):
    x = np.ascontiguousarray(x, F)
    return _stats(lambda *o: check_lib().log_pos_stats(x.size, x.ctypes.data, *o))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
def actor_weights(rng, family, widths, spread=3.0):
    """mlp_ref / mlp2_ref.normal_weights with the family's A and inputs scaled to its bounds; the scores of order `spread`"""
    lo, hi = value_ref.obs_bounds(family)
    scale = 1.0 / np.maximum(np.abs(lo), np.abs(hi))
    D, A = dims(family)
    if len(widths) == 1:
        return mlp_ref.normal_weights(rng, D, A, widths[0], scale, w2_scale=spread, b2_scale=0.5)
    return mlp2_ref.normal_weights(rng, D, A, widths[0], widths[1], scale, w3_scale=spread, b3_scale=0.5)


@functools.lru_cache(maxsize=None)
def actor(family, widths, seed=0):
    """(packed policy, weights tuple) for a family and widths, drawn once"""
    w = actor_weights(np.random.default_rng(1900 + 7 * sum(widths) + len(widths) + seed), family, widths)
    p = packed(w)
    p.setflags(write=False)
    return p, w


def constant_actor(family, widths, b):
    """the weights whose scores are `b` at every observation under every activation: every layer's weights and hidden biases +0, the last bias b"""
    D, A = dims(family)
    b = np.asarray(b, F)
    assert b.shape == (A,)
    H1 = widths[0]
    if len(widths) == 1:
        return np.zeros((H1, D), F), np.zeros(H1, F), np.zeros((A, H1), F), b
    H2 = widths[1]
    return np.zeros((H1, D), F), np.zeros(H1, F), np.zeros((H2, H1), F), np.zeros(H2, F), np.zeros((A, H2), F), b


def actions_for(rng, family, policy, widths, act, obs_first, obs, sigma):
    """a rollout's kind of action words [K, n]: uniform over the A actions, or mu + sigma z with z standard normal (float32), as the heads draw them"""
    D, A = dims(family)
    K, n = obs.shape[0], obs.shape[-1]
    if A > 1:
        return rng.integers(0, A, (K, n)).astype(np.uint32)
    mu = row_scores(policy, D, 1, widths, act, acted_rows(obs_first, obs))[0]
    return (mu + F(sigma) * rng.standard_normal((K, n)).astype(F)).astype(F)


@functools.lru_cache(maxsize=None)
def case(family, K, n, seed=0):
    """the observation buffers of one shape, computed once and never modified"""
    rng = np.random.default_rng(8000 + 100 * K + n + seed)
    c = dict(obs_first=value_ref.observations(rng, family, (), n), obs=value_ref.observations(rng, family, (K,), n))
    for a in c.values():
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def full_case(family, K, n, widths, act, sigma=0.5, seed=0):
    """(policy, obs_first, obs, actions, expected words) of one call, computed once and never modified"""
    D, A = dims(family)
    c = case(family, K, n, seed)
    pol, _ = actor(family, widths, seed)
    acts = actions_for(np.random.default_rng(31 + K + n + seed), family, pol, widths, act, c["obs_first"], c["obs"], sigma)
    exp = logprob_mlp(pol, D, A, widths, act, c["obs_first"], c["obs"], acts, sigma)
    acts.setflags(write=False)
    exp.setflags(write=False)
    return pol, c["obs_first"], c["obs"], acts, exp
