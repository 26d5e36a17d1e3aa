"""The text of mgym_ppo_grad_mlp / mgym_value_grad_mlp and of mgym_ppo_grad_mlp2 / mgym_value_grad_mlp2 (include/mgym.h) restated twice, and the cases the
host and the GPU tests share.  A case carries `widths`, (H,) or (H1, H2); everything here takes its depth from that.
grad64: the whole network, the loss and the analytic gradient in float64 from the same weights (np.tanh for both tanh forms), with S, per output word the mean
absolute per-env-step term the bounds are stated against.  words32 / grad32: the per-env-step f32 words of the header's text in numpy — the scores and
pre-activations of mlp_ref.scores / mlp2_ref.scores (glibc fmaf), logprob_ref's log-probability, glibc expm1f, the backward words of each depth (two layers:
glibc fmaf for the dh1 chain) — and their sums taken with np.sum in float64.  header_words / header_grad: modurl_gym_amd/csrc/grad.h and grad2.h compiled by
g++ (tests/native/grad_check.cpp).  No test here."""
import ctypes as C
import functools
import types

import numpy as np

import logprob_ref as R
import mlp2_ref
import mlp_ref
import mlp_sample_ref as S
import native_build
import value_ref
from glibc_f32 import expm1f, fmaf

F = np.float32
RELU, TANH, TANH_FAST = R.RELU, R.TANH, R.TANH_FAST
ACTS = value_ref.ACTS   # by depth: no exact tanh with two hidden layers
PPO, VALUE = "ppo", "value"
CLIP, ENT_COEF, SIGMA = 0.2, 0.01, 0.5
TARGET_RATIOS = (0.5, 0.7, 0.95, 1.0, 1.05, 1.3, 2.0)
KINK_RATIO, KINK_PRE = 1e-3, 1e-4   # every case keeps its ratios this far from 1 +- clip and its ReLU pre-activations this far from 0
GAUSS_ENT = 1.4189385332046727
STAT_NAMES = ("loss", "entropy", "kl", "clipped", "ratio")
WIDTHS = ((64, 64), (17, 9), (1, 1), (8, 64), (64, 17))   # the two-layer widths of the host and the device tests
SLAB_CAP = 256                                             # the most slabs a two-layer launch uses
# One hidden layer.  The largest |grad32_w - grad64_w| / S_w over the cases of test_grad_host.py::test_the_bound, gradient words and statistics, as that test
# measures and records them; the bounds are 4 x those (the margin of test_logprob_host.py)
GRAD_MEASURED, STAT_MEASURED = 3.17e-06, 1.57e-07
GRAD_BOUND, STAT_BOUND = 4 * GRAD_MEASURED, 4 * STAT_MEASURED
# torch's own f32 autograd of the textbook loss against grad64, the same measure on the CPU: the network-rounding bound of the device's torch comparison
TORCH32_MEASURED = 1.03e-06
TORCH32_BOUND = 4 * TORCH32_MEASURED
# Two hidden layers.  The same figures over the two-layer cases of test_the_bound; the bounds are 4 x those (the margin every learner call uses).  The gradient
# figure is one word (LunarLander's actor, (8, 64), ReLU, K = 2) whose few terms hold an h1_j = pre1_j just beyond the kink margin of 4e-4, where the chain's
# absolute rounding of 1e-6 is the word's error; the tanh_fast cases stay below 1e-5.  A second layer behind a ReLU makes such words: the one-layer figure
# (3.17e-06) does not carry over.
GRAD2_MEASURED, STAT2_MEASURED = 7.97e-03, 2.26e-07
GRAD2_BOUND, STAT2_BOUND = 4 * GRAD2_MEASURED, 4 * STAT2_MEASURED
# torch's own f32 autograd of the textbook loss against grad64, the same measure on the CPU (test_grad_host.py::test_torch_f32_against_float64)
TORCH32_2_MEASURED = 9.45e-05
TORCH32_2_BOUND = 4 * TORCH32_2_MEASURED
# by depth, len(widths)
BOUNDS = {1: types.SimpleNamespace(grad_measured=GRAD_MEASURED, stat_measured=STAT_MEASURED, grad=GRAD_BOUND, stat=STAT_BOUND, torch32_measured=TORCH32_MEASURED,
                                   torch32=TORCH32_BOUND),
          2: types.SimpleNamespace(grad_measured=GRAD2_MEASURED, stat_measured=STAT2_MEASURED, grad=GRAD2_BOUND, stat=STAT2_BOUND,
                                   torch32_measured=TORCH32_2_MEASURED, torch32=TORCH32_2_BOUND)}
# The kernels against grad32, the same per-env-step words summed in float64: they differ by the sums alone.  A product is rounded once (2^-24 of its size), an
# f32 accumulator of the matrix pipe carries at most 128 env-steps (each addition at most 2^-24 of the partial sum, which the terms' magnitudes bound), and the
# result is rounded to f32 once, as grad32's is: at most (1 + 128 + 2) 2^-24 of S_w, from the number formats alone; 132 with float64's own sums.
SUM_BOUND = 132 * 2.0 ** -24


def n_params(D, A, widths):
    return R.n_floats(D, A, widths)


def split(pol, D, A, widths):
    """[w1, b1, w2, b2] or [w1, b1, w2, b2, w3, b3] of a packed net"""
    return list(mlp_ref.split(pol, D, A, widths[0]) if len(widths) == 1 else mlp2_ref.split(pol, D, A, *widths))


def views(grad, D, A, widths):
    """(dw1, db1, dw2, db2[, dw3, db3], last word) of a gradient vector"""
    return (*split(np.asarray(grad)[:-1], D, A, widths), grad[-1])


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------------
def _pre64(pol, D, A, widths, rows):
    """every hidden layer's ReLU pre-activations in float64 -> [R, sum(widths), n]"""
    ws = [np.asarray(x, np.float64) for x in split(pol, D, A, widths)]
    x, pres = np.asarray(rows, F).astype(np.float64), []
    for k in range(len(widths)):
        pres.append(np.einsum("hd,kdn->khn", ws[2 * k], x) + ws[2 * k + 1][None, :, None])
        x = np.maximum(pres[-1], 0.0)
    return np.concatenate(pres, axis=1)


@functools.lru_cache(maxsize=None)
def case(family, K, n, widths, act, head=PPO, seed=0, all_clipped=False):
    """one call's inputs, computed once and never modified: logprob_ref's observations and actor (value_ref's critic for the value head) at the widths (H,) or
    (H1, H2); under ReLU every observation with a hidden |pre| < 4 KINK_PRE redrawn (seeded); actions as the heads draw them; logp_old = the float64 logp_new
    less the log of target ratios cycling through TARGET_RATIOS (all_clipped: 2 where adv > 0, 0.5 where adv < 0); adv standard normal, both signs; ret = the
    float64 value plus noise.  Each depth keeps the seed formula its recorded figures were measured with."""
    D, fam_A = R.dims(family)
    A = 1 if head == VALUE else fam_A
    base = R.case(family, K, n, seed)
    of, ob = base["obs_first"].copy(), base["obs"].copy()
    pol = (value_ref.critic(family, widths, seed) if head == VALUE else R.actor(family, widths, seed))[0]
    if len(widths) == 1:
        rng = np.random.default_rng(4100 + 13 * K + n + 7 * widths[0] + act + seed)
    else:
        rng = np.random.default_rng(5200 + 13 * K + n + 7 * widths[0] + 3 * widths[1] + act + seed)
    if act == RELU:
        for _ in range(64):
            rows = np.concatenate([of[None], ob])   # every row, the last included: it is only redrawn more than needed
            near = (np.abs(_pre64(pol, D, A, widths, rows)) < 4 * KINK_PRE).any(axis=1)   # [K + 1, n]
            if not near.any():
                break
            fresh = value_ref.observations(rng, family, (K + 1,), n)
            rows = np.where(near[:, None, :], fresh, rows)
            of, ob = rows[0].copy(), rows[1:].copy()
        else:
            raise AssertionError("could not move the observations off the ReLU kinks")
    c = types.SimpleNamespace(family=family, D=D, A=A, widths=tuple(widths), act=act, head=head, K=K, n=n, pol=pol, obs_first=of, obs=ob, sigma=SIGMA, clip=CLIP,
                              ent_coef=ENT_COEF if head == PPO else 0.0, gauss=head == PPO and fam_A == 1, actions=None, x1=None)
    if head == VALUE:
        v = R.scores64(pol, D, 1, widths, act, R.acted_rows(of, ob))[0]
        c.x0 = (v + rng.standard_normal((K, n))).astype(F)
    else:
        c.actions = R.actions_for(rng, family, pol, widths, act, of, ob, SIGMA)
        new = R.logprob64(pol, D, A, widths, act, of, ob, c.actions, SIGMA)
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
def _heads64(c, s, sl):
    """the loss's terms in float64 from the scores s [B, A] over the environments sl -> (ds [B, A], dls [B], stat [5, B], ratio [B])"""
    B, A = s.shape
    x0 = np.asarray(c.x0, F)[:, sl].astype(np.float64).reshape(-1)
    stat = np.zeros((5, B))
    dls = np.zeros(B)
    ratio = np.ones(B)
    if c.head == VALUE:
        e = s[:, 0] - x0
        ds = e[:, None]
        stat[0] = 0.5 * e * e
        return ds, dls, stat, ratio
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
    return ds, dls, stat, ratio


def grad64(c, first=None, count=None):
    """-> namespace(grad [P + 1], stats [8], S_grad [P + 1], S_stats [8], ratio [K, count], pre [K, sum(widths), count], bounds) over environments
    first .. first + count - 1"""
    D, A = c.D, c.A
    first, count, sl = _range(c, first, count)
    ws = [np.asarray(x, np.float64) for x in split(c.pol, D, A, c.widths)]
    rows = R.acted_rows(c.obs_first, c.obs)[:, :, sl].astype(np.float64)   # [K, D, m]
    X = np.moveaxis(rows, 1, 2).reshape(-1, D)                              # [B, D]
    B = X.shape[0]
    xs, pres = [X], []   # each layer's input and the hidden layers' pre-activations
    for k in range(len(c.widths)):
        pres.append(xs[-1] @ ws[2 * k].T + ws[2 * k + 1])
        xs.append(np.maximum(pres[-1], 0.0) if c.act == RELU else np.tanh(pres[-1]))
    s = xs[-1] @ ws[-2].T + ws[-1]                                          # [B, A]
    ds, dls, stat, ratio = _heads64(c, s, sl)
    deltas = [ds]   # d loss / d each layer's output before its activation, the first layer's first
    for k in reversed(range(len(c.widths))):
        deltas.insert(0, (deltas[0] @ ws[2 * k + 2]) * ((pres[k] > 0) if c.act == RELU else 1.0 - xs[k + 1] * xs[k + 1]))
    ab = np.abs
    grad = np.concatenate([w for d, x in zip(deltas, xs) for w in ((d.T @ x).ravel(), d.sum(0))] + [[dls.sum()]]) / B
    S_ = np.concatenate([w for d, x in zip(deltas, xs) for w in ((ab(d).T @ ab(x)).ravel(), ab(d).sum(0))] + [[ab(dls).sum()]]) / B
    if c.gauss:
        grad[-1] -= float(F(c.ent_coef))
        S_[-1] += abs(float(F(c.ent_coef)))
    stats, S_stats = np.zeros(8), np.zeros(8)
    stats[:5], S_stats[:5] = stat.mean(axis=1), np.abs(stat).mean(axis=1)
    stats[5] = S_stats[5] = float(F(B))
    pre = np.concatenate(pres, axis=1)
    return types.SimpleNamespace(grad=grad, stats=stats, S_grad=S_, S_stats=S_stats, ratio=ratio.reshape(c.K, count),
                                 pre=np.moveaxis(pre.reshape(c.K, count, sum(c.widths)), 1, 2), B=B, bounds=BOUNDS[len(c.widths)])


# ---- the header's text in f32 --------------------------------------------------------------------------------------------------------------------
def _heads32(c, s):
    """the heads' words from the scores s [A, B] over the whole [K, n] -> dict(ds [A, B], dls, g, r, hent [B], p [A, B], stat [5, B])"""
    A, B = s.shape
    zero = np.zeros(B, F)
    x0 = np.ascontiguousarray(c.x0, F).reshape(-1)
    out = dict(g=zero, r=zero, hent=zero, p=np.ones((A, B), F), dls=zero)
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


def _dact(act, pre, h):
    return np.where(pre > 0, F(1.0), F(0.0)).astype(F) if act == RELU else (F(1.0) - (h * h).astype(F)).astype(F)


def _dpre_last(c, w, ds, pre, h):
    """the last hidden layer's backward words, the same text at both depths: dh_k = the sum over a of w[a][k] ds_a, products and additions each rounded,
    and dpre_k = dh_k * act'(pre_k) -> [H, B]"""
    out = []
    for k in range(w.shape[1]):
        dh = (w[0, k] * ds[0]).astype(F)
        for a in range(1, c.A):
            dh = (dh + (w[a, k] * ds[a]).astype(F)).astype(F)
        out.append((dh * _dact(c.act, pre[k], h[k])).astype(F))
    return np.stack(out)


def words32(c):
    """the per-env-step words over the whole [K, n]: the heads' words of _heads32, s [A, B], o [D, B], and per hidden layer, the first one first, the lists
    pre, h and dpre ([H, B] each); with two layers also dpre2 [H2, B], dh1 and dpre1 [H1, B] by name"""
    D, A, B = c.D, c.A, c.K * c.n
    flat = np.ascontiguousarray(np.moveaxis(R.acted_rows(c.obs_first, c.obs), 1, 0).reshape(D, B))
    ws = split(c.pol, D, A, c.widths)
    if len(c.widths) == 1:
        s, *pre = mlp_ref.scores(c.pol, D, A, c.widths[0], flat, c.act, want_pre=True)
    else:
        s, *pre = mlp2_ref.scores(c.pol, D, A, *c.widths, flat, c.act, want_pre=True)
    with np.errstate(all="ignore"):
        f = mlp_ref._activation(c.act)
        h = [f(x).astype(F) for x in pre]
        out = dict(o=flat, s=s, pre=pre, h=h, **_heads32(c, s))
        dpre = [_dpre_last(c, ws[-2], out["ds"], pre[-1], h[-1])]
        if len(c.widths) == 2:   # dh1_j: one fmaf chain over k ascending from +0
            H1, H2 = c.widths
            dh1 = np.zeros((H1, B), F)
            for k in range(H2):
                for j in range(H1):
                    dh1[j] = fmaf(ws[2][k, j], dpre[0][k], dh1[j])
            dpre.insert(0, np.stack([(dh1[j] * _dact(c.act, pre[0][j], h[0][j])).astype(F) for j in range(H1)]))
            out.update(dpre2=dpre[1], dh1=dh1, dpre1=dpre[0])
    out["dpre"] = dpre
    return out


def grad32(c, first=None, count=None, words=None):
    """the words of words32, their products taken in f32, summed over the range with np.sum in float64, divided by B and rounded to f32
    -> (grad [P + 1] float32, stats [8] float32)"""
    first, count, _ = _range(c, first, count)
    w = words32(c) if words is None else words
    sel = np.zeros((c.K, c.n), bool)
    sel[:, first: first + count] = True
    sel = sel.reshape(-1)
    B = float(c.K * count)
    tot = lambda x: np.sum(np.asarray(x, F)[..., sel].astype(np.float64), axis=-1)
    outer = lambda a, b: np.concatenate([tot((row[None, :] * b).astype(F)) for row in a])   # [Ra, Rb] of f32 products, f64 sums
    last = float(tot(w["dls"]))
    if c.gauss:
        last -= float(F(c.ent_coef)) * B
    with np.errstate(all="ignore"):
        grad = np.concatenate([x for d, inp in zip(w["dpre"] + [w["ds"]], [w["o"]] + w["h"]) for x in (outer(d, inp), tot(d))] + [[last if c.gauss else 0.0]]) / B
    stats = np.zeros(8)
    stats[:5] = tot(w["stat"]) / B
    stats[5] = B
    return grad.astype(F), stats.astype(F)


def worst(got, ref, S):
    """the largest |got - ref| / S over the words with S > 0, and whether every word with S == 0 is exactly ref"""
    got, ref, S = (np.asarray(x, np.float64) for x in (got, ref, S))
    nz = S > 0
    return (float(np.max(np.abs(got - ref)[nz] / S[nz])) if nz.any() else 0.0), bool(np.all(got[~nz] == ref[~nz]))


def within(got_grad, got_stats, ref, extra=0.0):
    """the gradient words within (ref.bounds.grad + extra) S_w of grad64's and the statistics within (ref.bounds.stat + extra) S_w — the bounds of the depth
    grad64 ran at; a word whose terms are all zero is exactly zero.  -> (ok, the two measured figures)"""
    wg, zg = worst(got_grad, ref.grad, ref.S_grad)
    ws, zs = worst(np.asarray(got_stats)[:5], ref.stats[:5], ref.S_stats[:5])
    tail = np.asarray(got_stats, np.float64)[5:]
    ok = wg <= ref.bounds.grad + extra and ws <= ref.bounds.stat + extra and zg and zs and tail[0] == ref.stats[5] and (tail[1:] == 0).all()
    return ok, (wg, ws)


# ---- csrc/grad.h and csrc/grad2.h on the host ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def check_lib():
    lib = C.CDLL(native_build.shared("grad_check.cpp"))
    vp = C.c_void_p
    for name, widths in (("grad", 1), ("grad2", 2)):
        head = [C.c_int] * (4 + widths) + [vp, C.c_float, C.c_float, C.c_float, C.c_int32, C.c_uint64]
        for fn, args in ((f"{name}_words", head + [vp] * 6), (f"{name}_full", head + [C.c_uint64, C.c_uint64] + [vp] * 7), (f"{name}_slab_bytes_of", [C.c_int] * (2 + widths))):
            getattr(lib, fn).restype, getattr(lib, fn).argtypes = C.c_int, args
    lib.grad2_slab_cap.restype, lib.grad2_slab_cap.argtypes = C.c_int, []
    lib.grad_clip_ok_of.restype, lib.grad_clip_ok_of.argtypes = C.c_int, [C.c_float]
    lib.grad_ent_coef_ok_of.restype, lib.grad_ent_coef_ok_of.argtypes = C.c_int, [C.c_float]
    return lib


def _call_args(c):
    head = 2 if c.head == VALUE else (1 if c.gauss else 0)
    keep = [np.ascontiguousarray(c.pol, F), np.ascontiguousarray(c.obs_first, F), np.ascontiguousarray(c.obs, F),
            None if c.actions is None else np.ascontiguousarray(c.actions, F if c.gauss else np.uint32), np.ascontiguousarray(c.x0, F),
            None if c.x1 is None else np.ascontiguousarray(c.x1, F)]
    p = lambda a: None if a is None else a.ctypes.data
    return [c.D, c.A, c.act, head, *c.widths, p(keep[0]), float(c.sigma), float(c.clip), float(c.ent_coef), c.K, c.n], [p(a) for a in keep[1:]], keep


def header_words(c):
    """the headers' per-env-step words.  grad.h's heads -> dict(ds [A, B], g, r, hent [B], p [A, B], stat [5, B]); grad2.h's env-step ->
    dict(ds [A, B], dls [B], stat [5, B], dpre2 [H2, B], dh1 [H1, B], dpre1 [H1, B], s [A, B])"""
    A, B = c.A, c.K * c.n
    head, ptrs, keep = _call_args(c)
    if len(c.widths) == 1:
        fn, rows = check_lib().grad_words, (("ds", A), ("g", 1), ("r", 1), ("hent", 1), ("p", A), ("stat", 5))
    else:
        H1, H2 = c.widths
        fn, rows = check_lib().grad2_words, (("ds", A), ("dls", 1), ("stat", 5), ("dpre2", H2), ("dh1", H1), ("dpre1", H1), ("s", A))
    out = np.zeros((B, sum(r for _, r in rows)), F)
    assert fn(*head, *ptrs, out.ctypes.data) == 0
    at, res = 0, {}
    for name, r in rows:
        res[name] = out[:, at: at + r].T.copy()
        at += r
    for name in ("g", "r", "hent", "dls"):
        if name in res:
            res[name] = res[name][0]
    return res


def header_grad(c, first=None, count=None):
    """the header-driven full call: grad_envs' / grad2_envs' f64 sums and grad_result's words -> (grad [P + 1] float32, stats [8] float32)"""
    first, count, _ = _range(c, first, count)
    head, ptrs, keep = _call_args(c)
    grad, stats = np.zeros(n_params(c.D, c.A, c.widths) + 1, F), np.zeros(8, F)
    fn = check_lib().grad_full if len(c.widths) == 1 else check_lib().grad2_full
    assert fn(*head, first, count, *ptrs, grad.ctypes.data, stats.ctypes.data) == 0
    return grad, stats
