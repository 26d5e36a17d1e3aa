"""The hidden-layer policy of include/mgym.h (mgym_rollout_mlp and the entry points built on it), restated once on numpy float32 arrays: the fmaf chains in
ascending index order from the bias, every link one glibc fmaf (tests/glibc_f32.py), the hidden activation, and the strict argmax.  Also the packed weight
layout and the families' dimensions.  The draws built on the scores stay with their subjects: mlp_sample_ref.draw, mlp_gauss_ref.gauss_pair,
tanh_fast_ref.tanh_fast.  No test here."""
import numpy as np

import families
import glibc_f32 as G

F = np.float32
RELU, TANH, TANH_FAST = 0, 1, 3   # MGYM_ACT_RELU, MGYM_ACT_TANH, MGYM_ACT_TANH_FAST
# (D, A, continuous) of tests/families.py: a continuous family has A = 1 and its score is the action
FAMILIES = {name: (f.D, f.A, int(f.box is not None)) for name, f in families.FAMILIES.items()}


def n_floats(D, A, H):
    return H * (D + 1) + A * (H + 1)


def split(policy, D, A, H):
    """the packed policy -> (w1 [H, D], b1 [H], w2 [A, H], b2 [A]); a policy [n_floats, n] is one policy per column, and every part gains a last axis n"""
    p = np.asarray(policy, F)
    tail = p.shape[1:]
    assert p.shape[0] == n_floats(D, A, H) and len(tail) <= 1
    return p[: H * D].reshape(H, D, *tail), p[H * D: H * D + H], p[H * D + H: H * D + H + A * H].reshape(A, H, *tail), p[H * D + H + A * H:]


def packed(w):
    """nn.Linear-layout weights (w1, b1, w2, b2) -> the packed policy"""
    return np.concatenate([w[0].ravel(), w[1], w[2].ravel(), w[3]]).astype(F)


def normal_weights(rng, D, A, H, in_scale, w2_scale=1.0, b2_scale=0.1):
    """nn.Linear-layout float32 weights drawn from rng: w1 ~ N(0, 1) times what a unit of each observation component is worth (in_scale [D]),
    b1 ~ N(0, 0.5), w2 ~ N(0, w2_scale) / sqrt(H), b2 ~ N(0, b2_scale)"""
    w1 = (rng.normal(0, 1, (H, D)) * np.array(in_scale)).astype(F)
    b1 = rng.normal(0, 0.5, H).astype(F)
    w2 = (rng.normal(0, w2_scale, (A, H)) / np.sqrt(H)).astype(F)
    b2 = rng.normal(0, b2_scale, A).astype(F)
    return w1, b1, w2, b2


def _activation(activation):
    if callable(activation):
        return activation
    if activation == TANH_FAST:
        from tanh_fast_ref import tanh_fast   # (tanh_fast_ref imports this module)
        return tanh_fast
    return {RELU: lambda pre: np.where(pre > F(0), pre, F(0)).astype(F), TANH: G.tanhf}[activation]


def scores(policy, D, A, H, obs, activation, want_pre=False):
    """scores [A, n] over an observation [D, n] (with want_pre: and the hidden pre-activations [H, n]) under one policy, or under one policy per
    environment (policy [n_floats, n]).  activation: RELU, TANH, TANH_FAST or a function of a float32 array"""
    w1, b1, w2, b2 = split(policy, D, A, H)
    obs = np.ascontiguousarray(obs, F)
    act, n = _activation(activation), obs.shape[1]
    s, pres = [np.full(n, b2[a], F) for a in range(A)], []
    with np.errstate(all="ignore"):
        for j in range(H):
            pre = np.full(n, b1[j], F)
            for q in range(D):
                pre = G.fmaf(w1[j, q], obs[q], pre)
            pres.append(pre)
            h = act(pre)
            for a in range(A):
                s[a] = G.fmaf(w2[a, j], h, s[a])
    return (np.stack(s), np.stack(pres)) if want_pre else np.stack(s)


def argmax_words(s):
    """the sequential strict argmax over scores [A, n]: the first of equal scores wins, a NaN never replaces an earlier score"""
    best, act = s[0].copy(), np.zeros(s.shape[1], np.uint32)
    with np.errstate(all="ignore"):
        for a in range(1, s.shape[0]):
            m = s[a] > best
            best, act = np.where(m, s[a], best).astype(F), np.where(m, np.uint32(a), act).astype(np.uint32)
    return act
