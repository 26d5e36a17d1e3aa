"""The two-hidden-layer policy of include/mgym.h (mgym_rollout_mlp2) restated on numpy float32 arrays: three fmaf chains in ascending index order from the
bias, every link one glibc fmaf (tests/glibc_f32.py), the one hidden activation of both layers (tests/mlp_ref.py's), and the heads of the one-layer entry points
(mlp_ref.argmax_words, mlp_sample_ref.draw, mlp_gauss_ref.gauss_actions).  Shared by test_mlp2_host.py and test_gpu_mlp2.py (the host-compiled header is
tests/policy_header.py's).  No test here."""
import numpy as np

import glibc_f32 as G
import mlp_gauss_ref as GA
import mlp_ref as M
import mlp_sample_ref as S
from mlp_ref import FAMILIES, RELU, TANH_FAST   # noqa: F401  (re-exported)
from words import words_of

F = np.float32
GREEDY, SAMPLE, GAUSS = range(3)   # MGYM_HEAD_*
SHAPES = ((1, 1), (3, 5), (1, 64), (64, 1), (17, 33), (64, 64))


def n_floats(D, A, H1, H2):
    return H1 * (D + 1) + H2 * (H1 + 1) + A * (H2 + 1)


def packed(w):
    """nn.Linear-layout weights (w1, b1, w2, b2, w3, b3) -> the packed policy"""
    return np.concatenate([np.asarray(w[0], F).ravel(), w[1], np.asarray(w[2], F).ravel(), w[3], np.asarray(w[4], F).ravel(), w[5]]).astype(F)


def split(policy, D, A, H1, H2):
    p = np.asarray(policy, F)
    assert p.shape == (n_floats(D, A, H1, H2),)
    at, out = 0, []
    for shape in ((H1, D), (H1,), (H2, H1), (H2,), (A, H2), (A,)):
        size = int(np.prod(shape))
        out.append(p[at: at + size].reshape(shape))
        at += size
    return out


def normal_weights(rng, D, A, H1, H2, in_scale, w3_scale=1.0, b3_scale=0.1):
    """nn.Linear-layout float32 weights: w1 ~ N(0, 1) times what a unit of each observation component is worth, b1 ~ N(0, 0.5), w2 ~ N(0, 1.5) / sqrt(H1),
    b2 ~ N(0, 0.5), w3 ~ N(0, w3_scale) / sqrt(H2), b3 ~ N(0, b3_scale)"""
    w1 = (rng.normal(0, 1, (H1, D)) * np.array(in_scale)).astype(F)
    b1 = rng.normal(0, 0.5, H1).astype(F)
    w2 = (rng.normal(0, 1.5, (H2, H1)) / np.sqrt(H1)).astype(F)
    b2 = rng.normal(0, 0.5, H2).astype(F)
    w3 = (rng.normal(0, w3_scale, (A, H2)) / np.sqrt(H2)).astype(F)
    b3 = rng.normal(0, b3_scale, A).astype(F)
    return w1, b1, w2, b2, w3, b3


def scores(policy, D, A, H1, H2, obs, activation, want_pre=False):
    """scores [A, n] over an observation [D, n] (with want_pre: and the pre-activations [H1, n], [H2, n]): the text of include/mgym.h"""
    w1, b1, w2, b2, w3, b3 = split(policy, D, A, H1, H2)
    obs = np.ascontiguousarray(obs, F)
    act, n = M._activation(activation), obs.shape[1]
    with np.errstate(all="ignore"):
        pre1, h1 = [], []
        for j in range(H1):
            pre = np.full(n, b1[j], F)
            for q in range(D):
                pre = G.fmaf(w1[j, q], obs[q], pre)
            pre1.append(pre)
            h1.append(act(pre))
        s, pre2 = [np.full(n, b3[a], F) for a in range(A)], []
        for k in range(H2):
            pre = np.full(n, b2[k], F)
            for j in range(H1):
                pre = G.fmaf(w2[k, j], h1[j], pre)
            pre2.append(pre)
            h2 = act(pre)
            for a in range(A):
                s[a] = G.fmaf(w3[a, k], h2, s[a])
    return (np.stack(s), np.stack(pre1), np.stack(pre2)) if want_pre else np.stack(s)


def head_actions(head, s, sigma=0.0, seed=0, call=0, g=None, t=0):
    """the action words [n] uint32 of env ids g at step t from scores [A, n]: the heads of the one-layer entry points"""
    A = s.shape[0]
    if head == GREEDY:
        return words_of(s[0]).copy() if A == 1 else M.argmax_words(s)
    if head == SAMPLE:
        assert A > 1
        return S.draw(s, S.words(seed, call, g, t))[0]
    assert A == 1
    return words_of(GA.gauss_actions(s[0], sigma, seed, call, g, t)).copy()


def identity_middle(one_layer, H):
    """one-layer weights (w1, b1, w2, b2) -> the two-layer policy with W2 = I, b2 = +0 that computes the same scores under ReLU for finite h1"""
    w1, b1, w2, b2 = one_layer
    return w1, b1, np.eye(H, dtype=F), np.zeros(H, F), w2, b2


def signed_zero_policy(D, activation):
    """(H1, H2) = (3, 5), A = 1: the policy whose action word is 0x80000000 at every observation, and 0 under a chain padded with zero weights.
    tanh_fast: W1 = 0, b1 = +0 -> h1 = +0; W2 = -1, b2 = -0 -> pre2 = -0 -> h2 = -0; W3 = +1, b3 = -0 -> s = -0.
    ReLU: h2 = +0 (ReLU of -0); W3 = -1, b3 = -0 -> every product -0 -> s = -0."""
    w3 = F(1.0) if activation == TANH_FAST else F(-1.0)
    return (np.zeros((3, D), F), np.zeros(3, F), np.full((5, 3), F(-1.0)), np.full(5, F(-0.0)), np.full((1, 5), w3), np.full(1, F(-0.0)))
