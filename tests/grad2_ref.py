"""The text of mgym_ppo_grad_mlp2 and mgym_value_grad_mlp2 (include/mgym.h) restated twice, and the cases the host and the GPU tests share: grad_ref.py for
the two-hidden-layer net.  grad64: the whole network, the loss and the analytic gradient in float64 (np.tanh for tanh_fast), with S, per output word the mean
absolute per-env-step term the bounds are stated against.  words32 / grad32: the per-env-step f32 words of the header's text in numpy — the scores and
pre-activations of mlp2_ref.scores (glibc fmaf), the heads' words as grad_ref.words32 states them, the backward words with glibc fmaf for the dh1 chain — and
their sums taken with np.sum in float64.  header_words / header_grad: modurl_gym_amd/csrc/grad2.h compiled by g++ (tests/native/grad2_check.cpp).  No test
here."""
import ctypes as C
import functools
import types

import numpy as np

import grad_ref as G
import logprob_ref as R
import mlp2_ref
import mlp_ref
import mlp_sample_ref as S
import native_build
import value_ref
from glibc_f32 import expm1f, fmaf

F = np.float32
RELU, TANH_FAST = R.RELU, R.TANH_FAST
ACTS = (RELU, TANH_FAST)
PPO, VALUE = G.PPO, G.VALUE
CLIP, ENT_COEF, SIGMA = G.CLIP, G.ENT_COEF, G.SIGMA
KINK_RATIO, KINK_PRE = G.KINK_RATIO, G.KINK_PRE
WIDTHS = ((64, 64), (17, 9), (1, 1), (8, 64), (64, 17))
SLAB_CAP = 256
# the largest |grad32_w - grad64_w| / S_w over the cases of test_grad2_host.py::test_the_bound, gradient words and statistics, as that test measures and
# records them; the bounds are 4 x those (the margin every learner call uses).  The gradient figure is one word (LunarLander's actor, (8, 64), ReLU, K = 2) whose
# few terms hold an h1_j = pre1_j just beyond the kink margin of 4e-4, where the chain's absolute rounding of 1e-6 is the word's error; the tanh_fast cases stay
# below 1e-5.  A second layer behind a ReLU makes such words: the one-layer figure (3.17e-06) does not carry over.
GRAD2_MEASURED, STAT2_MEASURED = 7.97e-03, 2.26e-07
GRAD2_BOUND, STAT2_BOUND = 4 * GRAD2_MEASURED, 4 * STAT2_MEASURED
# torch's own f32 autograd of the textbook loss against grad64, the same measure on the CPU (test_grad2_host.py::test_torch_f32_against_float64)
TORCH32_2_MEASURED = 9.45e-05
TORCH32_2_BOUND = 4 * TORCH32_2_MEASURED
# The kernels against grad32, the same per-env-step words summed in float64: they differ by the sums alone.  A product is rounded once (2^-24 of its size), an
# f32 accumulator of the matrix pipe carries at most 128 env-steps (each addition at most 2^-24 of the partial sum, which the terms' magnitudes bound), and the
# result is rounded to f32 once, as grad32's is: at most (1 + 128 + 2) 2^-24 of S_w, from the number formats alone; 132 with float64's own sums.
SUM_BOUND = 132 * 2.0 ** -24


def n_params(D, A, H1, H2):
    return mlp2_ref.n_floats(D, A, H1, H2)


def views(grad, D, A, H1, H2):
    """(dw1, db1, dw2, db2, dw3, db3, last word) of a gradient vector"""
    return (*mlp2_ref.split(np.asarray(grad)[:-1], D, A, H1, H2), grad[-1])


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------------
def _pre64(pol, D, A, H1, H2, rows):
    """both layers' ReLU pre-activations in float64 -> [R, H1 + H2, n]"""
    w1, b1, w2, b2, _, _ = (np.asarray(x, np.float64) for x in mlp2_ref.split(pol, D, A, H1, H2))
    pre1 = np.einsum("hd,kdn->khn", w1, np.asarray(rows, F).astype(np.float64)) + b1[None, :, None]
    pre2 = np.einsum("gh,khn->kgn", w2, np.maximum(pre1, 0.0)) + b2[None, :, None]
    return np.concatenate([pre1, pre2], axis=1)


@functools.lru_cache(maxsize=None)
def case2(family, K, n, H1, H2, act, head=PPO, seed=0):
    """one call's inputs, computed once and never modified, as grad_ref.case builds them for one layer: logprob_ref's observations and actor (value_ref's critic
    for the value head) at the widths (H1, H2); under ReLU every observation with a |pre1_j| or |pre2_k| < 4 KINK_PRE redrawn (seeded); actions as the heads
    draw them; logp_old = the float64 logp_new less the log of target ratios cycling through grad_ref.TARGET_RATIOS; adv standard normal, both signs; ret = the
    float64 value plus noise"""
    D, fam_A = R.dims(family)
    A = 1 if head == VALUE else fam_A
    base = R.case(family, K, n, seed)
    of, ob = base["obs_first"].copy(), base["obs"].copy()
    widths = (H1, H2)
    pol = (value_ref.critic(family, widths, seed) if head == VALUE else R.actor(family, widths, seed))[0]
    rng = np.random.default_rng(5200 + 13 * K + n + 7 * H1 + 3 * H2 + act + seed)
    if act == RELU:
        for _ in range(64):
            rows = np.concatenate([of[None], ob])
            near = (np.abs(_pre64(pol, D, A, H1, H2, rows)) < 4 * KINK_PRE).any(axis=1)   # [K + 1, n]
            if not near.any():
                break
            fresh = value_ref.observations(rng, family, (K + 1,), n)
            rows = np.where(near[:, None, :], fresh, rows)
            of, ob = rows[0].copy(), rows[1:].copy()
        else:
            raise AssertionError("could not move the observations off the ReLU kinks")
    c = types.SimpleNamespace(family=family, D=D, A=A, H1=H1, H2=H2, act=act, head=head, K=K, n=n, pol=pol, obs_first=of, obs=ob, sigma=SIGMA, clip=CLIP,
                              ent_coef=ENT_COEF if head == PPO else 0.0, gauss=head == PPO and fam_A == 1, actions=None, x1=None)
    if head == VALUE:
        v = R.scores64(pol, D, 1, widths, act, R.acted_rows(of, ob))[0]
        c.x0 = (v + rng.standard_normal((K, n))).astype(F)
    else:
        c.actions = R.actions_for(rng, family, pol, widths, act, of, ob, SIGMA)
        new = R.logprob64(pol, D, A, widths, act, of, ob, c.actions, SIGMA)
        adv = rng.standard_normal((K, n)).astype(F)
        adv[adv == 0] = F(0.5)
        target = np.asarray(G.TARGET_RATIOS)[(np.arange(K * n) % len(G.TARGET_RATIOS)).reshape(K, n)]
        c.x0, c.x1 = (new - np.log(target)).astype(F), adv
    for a in (c.obs_first, c.obs, c.actions, c.x0, c.x1):
        if a is not None:
            a.setflags(write=False)
    return c


variant = G.variant


def _range(c, first, count):
    first, count = (0, c.n) if first is None else (first, count)
    return first, count, slice(first, first + count)


# ---- float64 -------------------------------------------------------------------------------------------------------------------------------------
def grad64(c, first=None, count=None):
    """-> namespace(grad [P2 + 1], stats [8], S_grad [P2 + 1], S_stats [8], ratio [K, count], pre [K, H1 + H2, count]) over environments first .. first + count - 1"""
    D, A, H1, H2 = c.D, c.A, c.H1, c.H2
    first, count, sl = _range(c, first, count)
    w1, b1, w2, b2, w3, b3 = (np.asarray(x, np.float64) for x in mlp2_ref.split(c.pol, D, A, H1, H2))
    rows = R.acted_rows(c.obs_first, c.obs)[:, :, sl].astype(np.float64)   # [K, D, m]
    X = np.moveaxis(rows, 1, 2).reshape(-1, D)                              # [B, D]
    B = X.shape[0]
    f = (lambda x: np.maximum(x, 0.0)) if c.act == RELU else np.tanh
    df = (lambda pre, h: (pre > 0).astype(np.float64)) if c.act == RELU else (lambda pre, h: 1.0 - h * h)
    pre1 = X @ w1.T + b1
    h1 = f(pre1)
    pre2 = h1 @ w2.T + b2
    h2 = f(pre2)
    s = h2 @ w3.T + b3                                                      # [B, A]
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
            stat[1] = np.log(sg) + G.GAUSS_ENT
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
    dpre2 = (ds @ w3) * df(pre2, h2)
    dpre1 = (dpre2 @ w2) * df(pre1, h1)
    ab = np.abs
    grad = np.concatenate([(dpre1.T @ X).ravel(), dpre1.sum(0), (dpre2.T @ h1).ravel(), dpre2.sum(0), (ds.T @ h2).ravel(), ds.sum(0), [dls.sum()]]) / B
    S_ = np.concatenate([(ab(dpre1).T @ ab(X)).ravel(), ab(dpre1).sum(0), (ab(dpre2).T @ ab(h1)).ravel(), ab(dpre2).sum(0), (ab(ds).T @ ab(h2)).ravel(),
                         ab(ds).sum(0), [ab(dls).sum()]]) / B
    if c.gauss:
        grad[-1] -= float(F(c.ent_coef))
        S_[-1] += abs(float(F(c.ent_coef)))
    stats, S_stats = np.zeros(8), np.zeros(8)
    stats[:5], S_stats[:5] = stat.mean(axis=1), np.abs(stat).mean(axis=1)
    stats[5] = S_stats[5] = float(F(B))
    pre = np.concatenate([pre1, pre2], axis=1)
    return types.SimpleNamespace(grad=grad, stats=stats, S_grad=S_, S_stats=S_stats, ratio=ratio.reshape(c.K, count),
                                 pre=np.moveaxis(pre.reshape(c.K, count, H1 + H2), 1, 2), B=B)


# ---- the header's text in f32 --------------------------------------------------------------------------------------------------------------------
def _dact(act, pre, h):
    return np.where(pre > 0, F(1.0), F(0.0)).astype(F) if act == RELU else (F(1.0) - (h * h).astype(F)).astype(F)


def words32(c):
    """the per-env-step words over the whole [K, n]: dict(s [A, B], ds [A, B], dls [B], stat [5, B], o [D, B], h1 [H1, B], h2 [H2, B], dpre2 [H2, B],
    dh1 [H1, B], dpre1 [H1, B]).  The heads' words are grad_ref.words32's lines on these scores."""
    D, A, H1, H2 = c.D, c.A, c.H1, c.H2
    B = c.K * c.n
    flat = np.ascontiguousarray(np.moveaxis(R.acted_rows(c.obs_first, c.obs), 1, 0).reshape(D, B))
    s, pre1, pre2 = mlp2_ref.scores(c.pol, D, A, H1, H2, flat, c.act, want_pre=True)
    _, _, w2, _, w3, _ = mlp2_ref.split(c.pol, D, A, H1, H2)
    zero = np.zeros(B, F)
    x0 = np.ascontiguousarray(c.x0, F).reshape(-1)
    out = dict(o=flat, s=s, dls=zero)
    with np.errstate(all="ignore"):
        f = mlp_ref._activation(c.act)
        h1, h2 = f(pre1).astype(F), f(pre2).astype(F)
        if c.head == VALUE:
            e = (s[0] - x0).astype(F)
            ds = e[None]
            out["stat"] = np.stack([(F(0.5) * (e * e).astype(F)).astype(F), zero, zero, zero, zero])
        else:
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
                ds = (((g * z).astype(F)) / sg).astype(F)[None]
                out["dls"] = (g * ((z * z).astype(F) - F(1.0)).astype(F)).astype(F)
                hent = np.full(B, F(R.log_pos(np.array([c.sigma], F))[0] + G.GAUSS_ENT), F)
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
                ds = np.stack([((g * ((act == k).astype(F) - p[k]).astype(F)).astype(F) + ((ent * p[k]).astype(F) * (lp[k] + hent).astype(F)).astype(F)).astype(F)
                               for k in range(A)])
            out["stat"] = np.stack([loss, hent, kl, clipped.astype(F), r])
        dpre2 = np.zeros((H2, B), F)
        dh1 = np.zeros((H1, B), F)
        for k in range(H2):
            dh = (w3[0, k] * ds[0]).astype(F)
            for a in range(1, A):
                dh = (dh + (w3[a, k] * ds[a]).astype(F)).astype(F)
            dpre2[k] = (dh * _dact(c.act, pre2[k], h2[k])).astype(F)
            for j in range(H1):
                dh1[j] = fmaf(w2[k, j], dpre2[k], dh1[j])
        dpre1 = np.stack([(dh1[j] * _dact(c.act, pre1[j], h1[j])).astype(F) for j in range(H1)])
    out.update(ds=ds, h1=h1, h2=h2, dpre2=dpre2, dh1=dh1, dpre1=dpre1)
    return out


def grad32(c, first=None, count=None, words=None):
    """the words of words32, their products taken in f32, summed over the range with np.sum in float64, divided by B and rounded to f32
    -> (grad [P2 + 1] float32, stats [8] float32)"""
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
        grad = np.concatenate([outer(w["dpre1"], w["o"]), tot(w["dpre1"]), outer(w["dpre2"], w["h1"]), tot(w["dpre2"]), outer(w["ds"], w["h2"]), tot(w["ds"]),
                               [last if c.gauss else 0.0]]) / B
    stats = np.zeros(8)
    stats[:5] = tot(w["stat"]) / B
    stats[5] = B
    return grad.astype(F), stats.astype(F)


worst = G.worst


def within(got_grad, got_stats, ref, extra=0.0):
    """the gradient words within (GRAD2_BOUND + extra) S_w of grad64's and the statistics within (STAT2_BOUND + extra) S_w; a word whose terms are all zero is
    exactly zero.  -> (ok, the two measured figures)"""
    wg, zg = worst(got_grad, ref.grad, ref.S_grad)
    ws, zs = worst(np.asarray(got_stats)[:5], ref.stats[:5], ref.S_stats[:5])
    tail = np.asarray(got_stats, np.float64)[5:]
    ok = wg <= GRAD2_BOUND + extra and ws <= STAT2_BOUND + extra and zg and zs and tail[0] == ref.stats[5] and (tail[1:] == 0).all()
    return ok, (wg, ws)


# ---- csrc/grad2.h on the host --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def check_lib():
    lib = C.CDLL(native_build.shared("grad2_check.cpp"))
    vp = C.c_void_p
    head = [C.c_int] * 6 + [vp, C.c_float, C.c_float, C.c_float, C.c_int32, C.c_uint64]
    lib.grad2_words.restype, lib.grad2_words.argtypes = C.c_int, head + [vp] * 6
    lib.grad2_full.restype, lib.grad2_full.argtypes = C.c_int, head + [C.c_uint64, C.c_uint64] + [vp] * 7
    lib.grad2_slab_bytes_of.restype, lib.grad2_slab_bytes_of.argtypes = C.c_int, [C.c_int] * 4
    lib.grad2_slab_cap.restype, lib.grad2_slab_cap.argtypes = C.c_int, []
    return lib


def _call_args(c):
    head = 2 if c.head == VALUE else (1 if c.gauss else 0)
    keep = [np.ascontiguousarray(c.pol, F), np.ascontiguousarray(c.obs_first, F), np.ascontiguousarray(c.obs, F),
            None if c.actions is None else np.ascontiguousarray(c.actions, F if c.gauss else np.uint32), np.ascontiguousarray(c.x0, F),
            None if c.x1 is None else np.ascontiguousarray(c.x1, F)]
    p = lambda a: None if a is None else a.ctypes.data
    return [c.D, c.A, c.act, head, c.H1, c.H2, p(keep[0]), float(c.sigma), float(c.clip), float(c.ent_coef), c.K, c.n], [p(a) for a in keep[1:]], keep


def header_words(c):
    """grad2.h's env-step over every env-step -> dict(ds [A, B], dls [B], stat [5, B], dpre2 [H2, B], dh1 [H1, B], dpre1 [H1, B], s [A, B])"""
    A, H1, H2, B = c.A, c.H1, c.H2, c.K * c.n
    head, ptrs, keep = _call_args(c)
    out = np.zeros((B, 2 * A + 6 + H2 + 2 * H1), F)
    assert check_lib().grad2_words(*head, *ptrs, out.ctypes.data) == 0
    at, res = 0, {}
    for name, rows in (("ds", A), ("dls", 1), ("stat", 5), ("dpre2", H2), ("dh1", H1), ("dpre1", H1), ("s", A)):
        res[name] = out[:, at: at + rows].T.copy()
        at += rows
    res["dls"] = res["dls"][0]
    return res


def header_grad(c, first=None, count=None):
    """the header-driven full call: grad2_envs' f64 sums and grad_result's words -> (grad [P2 + 1] float32, stats [8] float32)"""
    first, count, _ = _range(c, first, count)
    head, ptrs, keep = _call_args(c)
    grad, stats = np.zeros(n_params(c.D, c.A, c.H1, c.H2) + 1, F), np.zeros(8, F)
    assert check_lib().grad2_full(*head, first, count, *ptrs, grad.ctypes.data, stats.ctypes.data) == 0
    return grad, stats
