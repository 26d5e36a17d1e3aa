"""The text of mgym_ppo_grad_mlp and mgym_value_grad_mlp (include/mgym.h) restated twice, and the cases the host and the GPU tests share.
grad64: the whole network, the loss and the analytic gradient in float64 from the same weights (np.tanh for both tanh forms), with S, per output word the mean
absolute per-env-step term the bounds are stated against.  words32 / grad32: the per-env-step f32 words of the header's text in numpy — the scores and
pre-activations of mlp_ref.scores (glibc fmaf), logprob_ref's log-probability, glibc expm1f — and their sums taken with np.sum in float64.  header_words /
header_grad: modurl_gym_amd/csrc/grad.h compiled by g++ (tests/native/grad_check.cpp).  No test here."""
import ctypes as C
import functools
import types

import numpy as np

import families
import logprob_ref as R
import mlp_ref
import mlp_sample_ref as S
import native_build
import value_ref
from glibc_f32 import expm1f

F = np.float32
RELU, TANH, TANH_FAST = R.RELU, R.TANH, R.TANH_FAST
ACTS = (RELU, TANH, TANH_FAST)
PPO, VALUE = "ppo", "value"
CLIP, ENT_COEF, SIGMA = 0.2, 0.01, 0.5
TARGET_RATIOS = (0.5, 0.7, 0.95, 1.0, 1.05, 1.3, 2.0)
KINK_RATIO, KINK_PRE = 1e-3, 1e-4   # every case keeps its ratios this far from 1 +- clip and its ReLU pre-activations this far from 0
GAUSS_ENT = 1.4189385332046727
STAT_NAMES = ("loss", "entropy", "kl", "clipped", "ratio")
# the largest |grad32_w - grad64_w| / S_w over the cases of test_grad_host.py::test_the_bound, gradient words and statistics, as that test measures and
# records them; the bounds are 4 x those (the margin of test_logprob_host.py)
GRAD_MEASURED, STAT_MEASURED = 3.17e-06, 1.57e-07
GRAD_BOUND, STAT_BOUND = 4 * GRAD_MEASURED, 4 * STAT_MEASURED
# torch's own f32 autograd of the textbook loss against grad64, the same measure on the CPU: the network-rounding bound of the device's torch comparison
TORCH32_MEASURED = 1.03e-06
TORCH32_BOUND = 4 * TORCH32_MEASURED


def n_params(D, A, H):
    return mlp_ref.n_floats(D, A, H)


def views(grad, D, A, H):
    """(dw1 [H, D], db1 [H], dw2 [A, H], db2 [A], last word) of a gradient vector"""
    w1, b1, w2, b2 = mlp_ref.split(np.asarray(grad)[:-1], D, A, H)
    return w1, b1, w2, b2, grad[-1]


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------------
def _pre64(pol, D, A, H, rows):
    w1, b1, _, _ = (np.asarray(x, np.float64) for x in mlp_ref.split(pol, D, A, H))
    return np.einsum("hd,kdn->khn", w1, np.asarray(rows, F).astype(np.float64)) + b1[None, :, None]


@functools.lru_cache(maxsize=None)
def case(family, K, n, H, act, head=PPO, seed=0, all_clipped=False):
    """one call's inputs, computed once and never modified: logprob_ref's observations and actor (value_ref's critic for the value head); under ReLU every
    observation with a |pre_j| < KINK_PRE redrawn (seeded); actions as the heads draw them; logp_old = the float64 logp_new less the log of target ratios
    cycling through TARGET_RATIOS (all_clipped: 2 where adv > 0, 0.5 where adv < 0); adv standard normal, both signs; ret = the float64 value plus noise"""
    D, fam_A = R.dims(family)
    A = 1 if head == VALUE else fam_A
    base = R.case(family, K, n, seed)
    of, ob = base["obs_first"].copy(), base["obs"].copy()
    pol = (value_ref.critic(family, (H,), seed) if head == VALUE else R.actor(family, (H,), seed))[0]
    rng = np.random.default_rng(4100 + 13 * K + n + 7 * H + act + seed)
    if act == RELU:
        for _ in range(64):
            rows = np.concatenate([of[None], ob])   # every row, the last included: it is only redrawn more than needed
            near = (np.abs(_pre64(pol, D, A, H, rows)) < 4 * KINK_PRE).any(axis=1)   # [K + 1, n]
            if not near.any():
                break
            fresh = value_ref.observations(rng, family, (K + 1,), n)
            rows = np.where(near[:, None, :], fresh, rows)
            of, ob = rows[0].copy(), rows[1:].copy()
        else:
            raise AssertionError("could not move the observations off the ReLU kinks")
    c = types.SimpleNamespace(family=family, D=D, A=A, H=H, act=act, head=head, K=K, n=n, pol=pol, obs_first=of, obs=ob, sigma=SIGMA, clip=CLIP,
                              ent_coef=ENT_COEF if head == PPO else 0.0, gauss=head == PPO and fam_A == 1, actions=None, x1=None)
    if head == VALUE:
        v = R.scores64(pol, D, 1, (H,), act, R.acted_rows(of, ob))[0]
        c.x0 = (v + rng.standard_normal((K, n))).astype(F)
    else:
        c.actions = R.actions_for(rng, family, pol, (H,), act, of, ob, SIGMA)
        new = R.logprob64(pol, D, A, (H,), act, of, ob, c.actions, SIGMA)
        adv = rng.standard_normal((K, n)).astype(F)
        adv[adv == 0] = F(0.5)
        target = np.asarray(TARGET_RATIOS)[(np.arange(K * n) % len(TARGET_RATIOS)).reshape(K, n)]
        if all_clipped:
            target = np.where(adv > 0, 2.0, 0.5)
        c.x0, c.x1 = (new - np.log(target)).astype(F), adv
    for a in (c.obs_first, c.obs, c.actions, c.x0, c.x1):
        if a is not None:
            a.setflags(write=False)
    return c


def variant(c, **kw):
    out = types.SimpleNamespace(**vars(c))
    for k, v in kw.items():
        setattr(out, k, v)
    return out


def _range(c, first, count):
    first, count = (0, c.n) if first is None else (first, count)
    return first, count, slice(first, first + count)


# ---- float64 -------------------------------------------------------------------------------------------------------------------------------------
def grad64(c, first=None, count=None):
    """-> namespace(grad [P + 1], stats [8], S_grad [P + 1], S_stats [8], ratio [K, count], pre [K, H, count]) over environments first .. first + count - 1"""
    D, A, H = c.D, c.A, c.H
    first, count, sl = _range(c, first, count)
    w1, b1, w2, b2 = (np.asarray(x, np.float64) for x in mlp_ref.split(c.pol, D, A, H))
    rows = R.acted_rows(c.obs_first, c.obs)[:, :, sl].astype(np.float64)   # [K, D, m]
    X = np.moveaxis(rows, 1, 2).reshape(-1, D)                              # [B, D]
    B = X.shape[0]
    pre = X @ w1.T + b1
    h = np.maximum(pre, 0.0) if c.act == RELU else np.tanh(pre)
    s = h @ w2.T + b2                                                       # [B, A]
    x0 = np.asarray(c.x0, F)[:, sl].astype(np.float64).reshape(-1)
    stat = np.zeros((5, B))
    dls = np.zeros(B)
    ratio = np.ones(B)
    if c.head == VALUE:
        e = s[:, 0] - x0
        ds = e[:, None]
        stat[0] = 0.5 * e * e
    else:
        adv = np.asarray(c.x1, F)[:, sl].astype(np.float64).reshape(-1)
        lo, hi = float(F(1.0) - F(c.clip)), float(F(1.0) + F(c.clip))
        ent = float(F(c.ent_coef))
        if c.gauss:
            sg = float(F(c.sigma))
            a = np.asarray(c.actions, F)[:, sl].astype(np.float64).reshape(-1)
            z = (a - s[:, 0]) / sg
            logp = -0.5 * z * z - np.log(sg) - 0.5 * np.log(2.0 * np.pi)
            stat[1] = np.log(sg) + GAUSS_ENT
        else:
            act = np.asarray(c.actions, np.int64)[:, sl].reshape(-1)
            dlt = s - s.max(axis=1, keepdims=True)
            lp = dlt - np.log(np.exp(dlt).sum(axis=1, keepdims=True))
            p = np.exp(lp)
            logp = lp[np.arange(B), act]
            hent = -(p * lp).sum(axis=1)
            stat[1] = hent
        d = logp - x0
        ratio = np.exp(d)
        clipped = ((adv > 0) & (ratio > hi)) | ((adv < 0) & (ratio < lo))
        g = np.where(clipped, 0.0, -adv * ratio)
        stat[0] = -np.minimum(ratio * adv, np.clip(ratio, lo, hi) * adv)
        stat[2], stat[3], stat[4] = ratio - 1.0 - d, clipped, ratio
        if c.gauss:
            ds = (g * z / sg)[:, None]
            dls = g * (z * z - 1.0)
        else:
            ds = g[:, None] * (np.eye(A)[act] - p) + ent * p * (lp + hent[:, None])
    dh = ds @ w2
    dpre = dh * ((pre > 0) if c.act == RELU else 1.0 - h * h)
    grad = np.concatenate([(dpre.T @ X).ravel(), dpre.sum(0), (ds.T @ h).ravel(), ds.sum(0), [dls.sum()]]) / B
    S = np.concatenate([(np.abs(dpre).T @ np.abs(X)).ravel(), np.abs(dpre).sum(0), (np.abs(ds).T @ np.abs(h)).ravel(), np.abs(ds).sum(0), [np.abs(dls).sum()]]) / B
    if c.gauss:
        grad[-1] -= float(F(c.ent_coef))
        S[-1] += abs(float(F(c.ent_coef)))
    stats, S_stats = np.zeros(8), np.zeros(8)
    stats[:5], S_stats[:5] = stat.mean(axis=1), np.abs(stat).mean(axis=1)
    stats[5] = S_stats[5] = float(F(B))
    m = count
    return types.SimpleNamespace(grad=grad, stats=stats, S_grad=S, S_stats=S_stats, ratio=ratio.reshape(c.K, m), pre=np.moveaxis(pre.reshape(c.K, m, H), 1, 2), B=B)


# ---- the header's text in f32 --------------------------------------------------------------------------------------------------------------------
def words32(c):
    """the per-env-step words over the whole [K, n]: dict(ds [A, B], g, r, hent [B], p [A, B], stat [5, B], dls [B], o [D, B], h, pre [H, B])"""
    D, A, H = c.D, c.A, c.H
    B = c.K * c.n
    flat = np.ascontiguousarray(np.moveaxis(R.acted_rows(c.obs_first, c.obs), 1, 0).reshape(D, B))
    s, pre = mlp_ref.scores(c.pol, D, A, H, flat, c.act, want_pre=True)
    zero, one = np.zeros(B, F), np.ones(B, F)
    x0 = np.ascontiguousarray(c.x0, F).reshape(-1)
    out = dict(o=flat, pre=pre, g=zero, r=zero, hent=zero, p=np.ones((A, B), F), dls=zero)
    with np.errstate(all="ignore"):
        out["h"] = mlp_ref._activation(c.act)(pre).astype(F)
        if c.head == VALUE:
            e = (s[0] - x0).astype(F)
            out["ds"] = e[None]
            out["stat"] = np.stack([(F(0.5) * (e * e).astype(F)).astype(F), zero, zero, zero, zero])
            return out
        adv = np.ascontiguousarray(c.x1, F).reshape(-1)
        lo, hi, ent = F(1.0) - F(c.clip), F(1.0) + F(c.clip), F(c.ent_coef)
        if c.gauss:
            a = np.ascontiguousarray(c.actions, F).reshape(-1)
            logp = R.logp_gauss(s[0], a, c.sigma).view(F)
        else:
            act = np.ascontiguousarray(c.actions, np.uint32).reshape(-1)
            logp = R.logp_discrete(s, act).view(F)
        d = (logp - x0).astype(F)
        r = (expm1f(d) + F(1.0)).astype(F)
        clipped = ((adv > 0) & (r > hi)) | ((adv < 0) & (r < lo))
        g = np.where(clipped, F(0.0), ((-adv) * r).astype(F)).astype(F)
        rc = np.where(r < lo, lo, np.where(r > hi, hi, r)).astype(F)
        u, uc = (r * adv).astype(F), (rc * adv).astype(F)
        loss = (-np.where(uc < u, uc, u)).astype(F)
        kl = ((r - F(1.0)).astype(F) - d).astype(F)
        if c.gauss:
            sg = F(c.sigma)
            z = ((a - s[0]).astype(F) / sg).astype(F)
            out["ds"] = (((g * z).astype(F)) / sg).astype(F)[None]
            out["dls"] = (g * ((z * z).astype(F) - F(1.0)).astype(F)).astype(F)
            hent = np.full(B, F(R.log_pos(np.array([c.sigma], F))[0] + GAUSS_ENT), F)
        else:
            _, cum = S.draw(s, np.zeros(B, np.uint32))
            m = s[0].copy()
            for k in range(1, A):
                m = np.where(s[k] > m, s[k], m).astype(F)
            total = cum[A - 1]
            lse = R.log_pos(total).astype(F)
            p = np.stack([((expm1f((s[k] - m).astype(F)) + F(1.0)).astype(F) / total).astype(F) for k in range(A)])
            lp = np.stack([((s[k] - m).astype(F) - lse).astype(F) for k in range(A)])
            t = (p[0] * lp[0]).astype(F)
            for k in range(1, A):
                t = (t + (p[k] * lp[k]).astype(F)).astype(F)
            hent = (-t).astype(F)
            out["ds"] = np.stack([((g * ((act == k).astype(F) - p[k]).astype(F)).astype(F) + ((ent * p[k]).astype(F) * (lp[k] + hent).astype(F)).astype(F)).astype(F)
                                  for k in range(A)])
            out["p"] = p
        out.update(g=g, r=r, hent=hent, stat=np.stack([loss, hent, kl, clipped.astype(F), r]))
    return out


def grad32(c, first=None, count=None, words=None):
    """the words of words32 summed over the range with np.sum in float64, divided by B and rounded to f32 -> (grad [P + 1] float32, stats [8] float32)"""
    D, A, H = c.D, c.A, c.H
    first, count, _ = _range(c, first, count)
    w = words32(c) if words is None else words
    _, _, w2, _ = mlp_ref.split(c.pol, D, A, H)
    sel = np.zeros((c.K, c.n), bool)
    sel[:, first: first + count] = True
    sel = sel.reshape(-1)
    B = float(c.K * count)
    tot = lambda x: float(np.sum(np.asarray(x, F)[sel].astype(np.float64)))
    gw1, gb1, gw2 = np.zeros((H, D)), np.zeros(H), np.zeros((A, H))
    ds, o, h, pre = w["ds"], w["o"], w["h"], w["pre"]
    with np.errstate(all="ignore"):
        for j in range(H):
            dh = (w2[0, j] * ds[0]).astype(F)
            for a in range(1, A):
                dh = (dh + (w2[a, j] * ds[a]).astype(F)).astype(F)
            dact = np.where(pre[j] > 0, F(1.0), F(0.0)).astype(F) if c.act == RELU else (F(1.0) - (h[j] * h[j]).astype(F)).astype(F)
            dpre = (dh * dact).astype(F)
            for q in range(D):
                gw1[j, q] = tot((dpre * o[q]).astype(F))
            gb1[j] = tot(dpre)
            for a in range(A):
                gw2[a, j] = tot((ds[a] * h[j]).astype(F))
    last = tot(w["dls"])
    if c.gauss:
        last -= float(F(c.ent_coef)) * B
    grad = np.concatenate([gw1.ravel(), gb1, gw2.ravel(), [tot(ds[a]) for a in range(A)], [last if c.gauss else 0.0]]) / B
    stats = np.zeros(8)
    stats[:5] = [tot(w["stat"][k]) / B for k in range(5)]
    stats[5] = B
    return grad.astype(F), stats.astype(F)


def worst(got, ref, S):
    """the largest |got - ref| / S over the words with S > 0, and whether every word with S == 0 is exactly ref"""
    got, ref, S = (np.asarray(x, np.float64) for x in (got, ref, S))
    nz = S > 0
    return (float(np.max(np.abs(got - ref)[nz] / S[nz])) if nz.any() else 0.0), bool(np.all(got[~nz] == ref[~nz]))


def within(got_grad, got_stats, ref, extra=0.0):
    """the gradient words within (GRAD_BOUND + extra) S_w of grad64's and the statistics within (STAT_BOUND + extra) S_w; a word whose terms are all zero is
    exactly zero.  -> (ok, the two measured figures)"""
    wg, zg = worst(got_grad, ref.grad, ref.S_grad)
    ws, zs = worst(np.asarray(got_stats)[:5], ref.stats[:5], ref.S_stats[:5])
    tail = np.asarray(got_stats, np.float64)[5:]
    ok = wg <= GRAD_BOUND + extra and ws <= STAT_BOUND + extra and zg and zs and tail[0] == ref.stats[5] and (tail[1:] == 0).all()
    return ok, (wg, ws)


# ---- csrc/grad.h on the host ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def check_lib():
    lib = C.CDLL(native_build.shared("grad_check.cpp"))
    vp = C.c_void_p
    head = [C.c_int] * 5 + [vp, C.c_float, C.c_float, C.c_float, C.c_int32, C.c_uint64]
    lib.grad_words.restype, lib.grad_words.argtypes = C.c_int, head + [vp] * 6
    lib.grad_full.restype, lib.grad_full.argtypes = C.c_int, head + [C.c_uint64, C.c_uint64] + [vp] * 7
    lib.grad_slab_bytes_of.restype, lib.grad_slab_bytes_of.argtypes = C.c_int, [C.c_int] * 3
    lib.grad_clip_ok_of.restype, lib.grad_clip_ok_of.argtypes = C.c_int, [C.c_float]
    lib.grad_ent_coef_ok_of.restype, lib.grad_ent_coef_ok_of.argtypes = C.c_int, [C.c_float]
    return lib


def _call_args(c):
    head = 2 if c.head == VALUE else (1 if c.gauss else 0)
    keep = [np.ascontiguousarray(c.pol, F), np.ascontiguousarray(c.obs_first, F), np.ascontiguousarray(c.obs, F),
            None if c.actions is None else np.ascontiguousarray(c.actions, F if c.gauss else np.uint32), np.ascontiguousarray(c.x0, F),
            None if c.x1 is None else np.ascontiguousarray(c.x1, F)]
    p = lambda a: None if a is None else a.ctypes.data
    return [c.D, c.A, c.act, head, c.H, p(keep[0]), float(c.sigma), float(c.clip), float(c.ent_coef), c.K, c.n], [p(a) for a in keep[1:]], keep


def header_words(c):
    """grad.h's heads over every env-step -> dict(ds [A, B], g, r, hent [B], p [A, B], stat [5, B])"""
    A, B = c.A, c.K * c.n
    head, ptrs, keep = _call_args(c)
    out = np.zeros((B, 2 * A + 3 + 5), F)
    assert check_lib().grad_words(*head, *ptrs, out.ctypes.data) == 0
    return dict(ds=out[:, :A].T.copy(), g=out[:, A].copy(), r=out[:, A + 1].copy(), hent=out[:, A + 2].copy(), p=out[:, A + 3: 2 * A + 3].T.copy(),
                stat=out[:, 2 * A + 3:].T.copy())


def header_grad(c, first=None, count=None):
    """the header-driven full call: grad_envs' f64 sums and grad_result's words -> (grad [P + 1] float32, stats [8] float32)"""
    first, count, _ = _range(c, first, count)
    head, ptrs, keep = _call_args(c)
    grad, stats = np.zeros(n_params(c.D, c.A, c.H) + 1, F), np.zeros(8, F)
    assert check_lib().grad_full(*head, first, count, *ptrs, grad.ctypes.data, stats.ctypes.data) == 0
    return grad, stats
