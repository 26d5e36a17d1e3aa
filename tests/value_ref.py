"""The text of mgym_value_mlp (include/mgym.h) restated in numpy: V is the one score of mlp_ref.scores / mlp2_ref.scores with A = 1 (glibc fmaf chains in
ascending order from the bias); the row mapping (value_out[0] from obs_first, value_out[t] from obs[t - 1], last_value_out from obs[K - 1]); the selection
trunc != 0 && (done is None or done == 0); and a poison word everywhere the text does not write.  value64: the same network in float64 with ordinary dot
products, what a learner's critic computes up to summation order.  header_value_mlp: modurl_gym_amd/csrc/value.h compiled by g++ (tests/native/value_check.cpp).
Case generators shared by the host and the GPU tests.  No test here."""
import ctypes as C
import functools

import numpy as np

import families
import mlp2_ref
import mlp_ref
import modurl_gym_amd as mg
import native_build

F = np.float32
POISON = 0x7FC0DEAD   # the fill of guards, of outputs before the call, and of final_obs where nothing may read it
RELU, TANH, TANH_FAST = mlp_ref.RELU, mlp_ref.TANH, mlp_ref.TANH_FAST
ACTS = {1: (RELU, TANH, TANH_FAST), 2: (RELU, TANH_FAST)}   # the activations each depth accepts
ACT_NAMES = {RELU: "relu", TANH: "tanh", TANH_FAST: "tanh_fast"}
WIDTHS = ((1,), (17,), (64,), (1, 1), (3, 5), (17, 33), (64, 64))


def n_floats(D, widths):
    return mlp_ref.n_floats(D, 1, widths[0]) if len(widths) == 1 else mlp2_ref.n_floats(D, 1, *widths)


def packed(weights):
    return mlp_ref.packed(weights) if len(weights) == 4 else mlp2_ref.packed(weights)


def values(critic, D, widths, act, rows):
    """V over observation rows [.., D, n] -> float32 [.., n]"""
    rows = np.asarray(rows, F)
    lead, n = rows.shape[:-2], rows.shape[-1]
    flat = np.ascontiguousarray(np.moveaxis(rows.reshape(-1, D, n), 1, 0).reshape(D, -1))   # [D, R * n]
    s = mlp_ref.scores(critic, D, 1, widths[0], flat, act) if len(widths) == 1 else mlp2_ref.scores(critic, D, 1, widths[0], widths[1], flat, act)
    return s[0].reshape(*lead, n)


def selection(done, trunc):
    """where final_value_out is written: bool [K, n]"""
    u = np.asarray(trunc) != 0
    return u if done is None else u & ~(np.asarray(done) != 0)


def dense_rows(obs_first, obs):
    """the K + 1 observation rows of the dense outputs: row 0 = obs_first, row r = obs[r - 1]"""
    return np.concatenate([np.asarray(obs_first, F)[None], np.asarray(obs, F)])


def value_mlp(critic, D, widths, act, obs_first, obs, final_obs=None, done=None, trunc=None, fill=POISON):
    """-> (value [K, n] float32, last_value [n] float32, final words uint32 [K, n] or None): the final words hold `fill` wherever the text writes nothing, and
    final_obs is read only where it is selected"""
    v = values(critic, D, widths, act, dense_rows(obs_first, obs))
    if final_obs is None:
        return v[:-1], v[-1], None
    K, n = np.shape(obs)[0], np.shape(obs)[-1]
    sel = selection(done, trunc)
    t, i = np.nonzero(sel)
    out = np.full((K, n), fill, np.uint32)
    if t.size:
        cols = np.asarray(final_obs, F)[t, :, i].T   # [D, selected]
        out[t, i] = values(critic, D, widths, act, cols).view(np.uint32)
    return v[:-1], v[-1], out


def split(critic, D, widths):
    return mlp_ref.split(critic, D, 1, widths[0]) if len(widths) == 1 else mlp2_ref.split(critic, D, 1, *widths)


def value64(critic, D, widths, act, rows):
    """the same network in float64: weights and observations converted exactly, numpy dot products, np.tanh for both tanh activations -> float64 [.., n]"""
    f = (lambda x: np.maximum(x, 0.0)) if act == RELU else np.tanh
    ws = [np.asarray(w, np.float64) for w in split(critic, D, widths)]
    x = np.moveaxis(np.asarray(rows, F).astype(np.float64), -2, -1)   # [.., n, D]
    for k in range(0, len(ws) - 2, 2):
        x = f(x @ ws[k].T + ws[k + 1])
    return (x @ ws[-2].T + ws[-1])[..., 0]


# ---- csrc/value.h on the host ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def check_lib():
    lib = C.CDLL(native_build.shared("value_check.cpp"))
    vp = C.c_void_p
    lib.value_eval.restype, lib.value_eval.argtypes = C.c_int, [C.c_int] * 5 + [vp, C.c_int32, C.c_uint64] + [vp] * 8
    lib.value_chunk.restype, lib.value_wave_envs.restype = C.c_int, C.c_int
    return lib


def chunk():
    """kValueChunk of csrc/value.h: the steps one block of the final pass lists"""
    return check_lib().value_chunk()


def wave_envs():
    """kValueWaveEnvs: the consecutive environments one wave of the final pass owns"""
    return check_lib().value_wave_envs()


def _p(a):
    return None if a is None else a.ctypes.data


def header_value_mlp(critic, D, widths, act, obs_first, obs, final_obs=None, done=None, trunc=None, fill=POISON):
    """value.h's value_env over every environment, outputs pre-filled with `fill` -> the triple of value_mlp"""
    critic, obs_first, obs = (np.ascontiguousarray(x, F) for x in (critic, obs_first, obs))
    K, n = obs.shape[0], obs.shape[-1]
    assert critic.size == n_floats(D, widths) and obs.shape == (K, D, n) and obs_first.shape == (D, n)
    fo = None if final_obs is None else np.ascontiguousarray(final_obs, F)
    d, u = (None if x is None else np.ascontiguousarray(x, np.uint8) for x in (done, trunc))
    val, last = np.full((K, n), fill, np.uint32), np.full(n, fill, np.uint32)
    fin = None if fo is None else np.full((K, n), fill, np.uint32)
    st = check_lib().value_eval(D, len(widths), act, widths[0], (*widths, 0)[1], _p(critic), K, n, _p(obs_first), _p(obs), _p(fo), _p(d), _p(u), _p(val), _p(last), _p(fin))
    assert st == 0, f"value_eval: status {st} (2: the four-per-lane form of the dense rows differs from the one-per-lane form)"
    return val.view(F), last.view(F), fin


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
def obs_bounds(family):
    """(low [D], high [D]) of the family's observation space, an infinite bound taken as +-5"""
    s = mg.get_spec(families.FAMILIES[family].kind)
    lo, hi = np.array(s.obs_low[: s.obs_dim], np.float64), np.array(s.obs_high[: s.obs_dim], np.float64)
    return np.where(np.isfinite(lo), lo, -5.0), np.where(np.isfinite(hi), hi, 5.0)


def observations(rng, family, shape_lead, n):
    """float32 [*shape_lead, D, n] uniform inside the family's observation space"""
    lo, hi = obs_bounds(family)
    return rng.uniform(lo[:, None], hi[:, None], (*shape_lead, lo.size, n)).astype(F)


def critic_weights(rng, family, widths):
    """mlp_ref.normal_weights / mlp2_ref.normal_weights with A = 1 and inputs scaled to the family's bounds, the value head of order 10"""
    lo, hi = obs_bounds(family)
    scale = 1.0 / np.maximum(np.abs(lo), np.abs(hi))
    D = lo.size
    if len(widths) == 1:
        return mlp_ref.normal_weights(rng, D, 1, widths[0], scale, w2_scale=10.0, b2_scale=1.0)
    return mlp2_ref.normal_weights(rng, D, 1, widths[0], widths[1], scale, w3_scale=10.0, b3_scale=1.0)


def flags(rng, K, n, p_done=0.05, p_trunc=0.1):
    """done, trunc uint8 [K, n] at the given rates (so done masks some truncations), then the first waves — kValueWaveEnvs consecutive environments — patched by
    hand into known positions, done 0 throughout them so that the classes hold with done passed or NULL:
      wave 0: no env-step selected;  wave 1: exactly 1, at (K - 1, its environment 77);  wave 2: exactly 64, at t = 0 in its environments 3 k;
      wave 3: exactly 65, at t = 0 in its environments 0 .. 64;  wave 4 (what n leaves of it): every env-step selected over all K"""
    W = wave_envs()
    assert n > 4 * W
    d = (rng.random((K, n)) < p_done).astype(np.uint8)
    u = (rng.random((K, n)) < p_trunc).astype(np.uint8)
    d[:, : min(n, 5 * W)] = 0
    u[:, : 4 * W] = 0
    u[K - 1, W + 77] = 1
    u[0, 2 * W: 2 * W + 192: 3] = 1
    u[0, 3 * W: 3 * W + 65] = 1
    u[:, 4 * W: 5 * W] = 1
    return d, u


def check_coverage(d, u):
    """the classes a case claims, asserted on its own flags, with done passed and with done NULL"""
    W = wave_envs()
    K, n = np.shape(u)
    for dd in (d, None):
        sel = selection(dd, u)
        per_wave = [int(sel[:, w * W: (w + 1) * W].sum()) for w in range((n + W - 1) // W)]
        assert per_wave[:4] == [0, 1, 64, 65], per_wave[:4]
        assert sel[:, 4 * W: 5 * W].all() and sel[:, 4 * W: 5 * W].size >= K, "a wave with every env-step selected over all K"
        assert sel[K - 1].any() and sel[0].any()
    if n > 5 * W:
        assert (selection(d, u) != selection(None, u)).any(), "done masks a truncation somewhere"


def poisoned_final_obs(final_obs, sel):
    """final_obs with the poison NaN in every word outside the selected env-steps"""
    out = np.where(np.asarray(sel, bool)[:, None, :], np.asarray(final_obs, F), np.full(np.shape(final_obs), POISON, np.uint32).view(F))
    return np.ascontiguousarray(out, F)


@functools.lru_cache(maxsize=None)
def case(family, K, n, seed=0):
    """the buffers of one shape, computed once and never modified: obs_first, obs, final_obs (clean), done, trunc (flag bytes of any non-zero value), and
    final_obs poisoned outside the selection under (done, trunc) and under (NULL, trunc)"""
    rng = np.random.default_rng(7000 + 100 * K + n + seed)
    D = families.FAMILIES[family].D
    d, u = flags(rng, K, n)
    check_coverage(d, u)
    d, u = (d * rng.integers(1, 256, (K, n))).astype(np.uint8), (u * rng.integers(1, 256, (K, n))).astype(np.uint8)
    c = dict(D=D, obs_first=observations(rng, family, (), n), obs=observations(rng, family, (K,), n), final_obs=observations(rng, family, (K,), n), d=d, u=u)
    c["final_obs_d"] = poisoned_final_obs(c["final_obs"], selection(d, u))
    c["final_obs_nd"] = poisoned_final_obs(c["final_obs"], selection(None, u))
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def critic(family, widths, seed=0):
    """(packed critic, weights tuple) for a family and widths, drawn once"""
    w = critic_weights(np.random.default_rng(900 + 7 * sum(widths) + len(widths) + seed), family, widths)
    p = packed(w)
    p.setflags(write=False)
    return p, w
