"""No-GPU check of the MLP policy header with MGYM_ACT_TANH_FAST: modurl_gym_amd/csrc/mlp_policy.h compiled for the host with ACT = MLP_ACT_TANH_FAST
(tests/native/policy_check.cpp, g++ -ffp-contract=off) against the restated fmaf chains of include/mgym.h with tests/tanh_fast_ref.py as the hidden
activation — every score and every action word, for the argmax, the categorical draw and the Gaussian draw where the family has them."""
import numpy as np
import pytest

import mlp_ref as M
import policy_header as P
import tanh_fast_ref as T
from words import same_words

F = np.float32
HIDDEN = (1, 7, 64)
N = 64   # environments per case (a multiple of 4: the Gaussian form works on lanes of four)
CASES = [(fam, form, H) for fam, (D, A, _) in M.FAMILIES.items() for form in ((T.ARGMAX, T.GAUSS) if A == 1 else (T.ARGMAX, T.SAMPLE)) for H in HIDDEN]


def make_case(rng, D, A, H):
    """weights that put pre-activations across the activation's whole range: the linear part near 0, the bend, the clamp; some +-0, huge and NaN inputs"""
    pol = rng.normal(0, 1.5, T.n_floats(D, A, H)).astype(F)
    w1, b1, w2, b2 = M.split(pol, D, A, H)
    w1 *= rng.choice(np.array([1e-3, 0.3, 1.0, 4.0, 30.0], F), (H, 1))
    obs = rng.normal(0, 1.0, (D, N)).astype(F)
    obs[:, 0] = 0.0
    obs[:, 1] = -0.0
    obs[0, 2] = 1e30
    obs[0, 3] = np.nan
    obs[:, 4] = 1e-41   # denormal inputs: denormal pre-activations when the bias is 0
    if H > 1:
        b1[0] = 0.0
    return pol, obs


@pytest.mark.parametrize("fam,form,H", CASES, ids=[f"{fam}-{('argmax', 'sample', 'gauss')[form]}-H{H}" for fam, form, H in CASES])
def test_header_matches_the_restated_chains(fam, form, H):
    D, A, _ = M.FAMILIES[fam]
    rng = np.random.default_rng(1000 * D + 100 * A + 10 * form + H)
    for rep in range(3):
        pol, obs = make_case(rng, D, A, H)
        seed, call, g0, t, sigma = 0x1234567887654321 + rep, 7 + rep, 4 * (rep + (1 << 31)), 3 + rep, 0.5 * rep
        g = np.uint64(g0) + np.arange(N, dtype=np.uint64)
        got_a, got_s = P.header_actions(D, A, 1, M.TANH_FAST, form, (H,), pol, obs, sigma, seed, call, g0, t)
        exp_a, exp_s = T.policy_actions(form, pol, D, A, H, obs, sigma, seed, call, g, t)
        assert same_words(got_s, exp_s), (fam, form, H, rep)
        if A == 1:   # action words are floats: NaNs compare as a class
            assert same_words(got_a, exp_a), (fam, form, H, rep)
        else:
            assert np.array_equal(got_a, exp_a), (fam, form, H, rep)
            assert got_a.max() < A


def test_discrete_actions_all_occur_and_the_activation_is_not_relu_or_exact_tanh():
    """the scores really go through mg_tanhf_fast: on ordinary inputs they differ from the exact-tanh chain in some last bits and are nowhere ReLU's"""
    assert len(CASES) == 6 * 2 * len(HIDDEN)   # every family's (D, A) with the argmax and with the draw it has
    rng = np.random.default_rng(5)
    D, A, H = 3, 1, 64
    pol = rng.normal(0, 1.0, T.n_floats(D, A, H)).astype(F)
    obs = rng.normal(0, 1.0, (D, 256)).astype(F)
    _, s = P.header_actions(D, A, 1, M.TANH_FAST, P.GREEDY, (H,), pol, obs)
    exact, relu = M.scores(pol, D, 1, H, obs, M.TANH)[0], M.scores(pol, D, 1, H, obs, M.RELU)[0]
    assert np.abs(s[0] - exact).max() < 1e-4 and not np.array_equal(s[0], exact)
    assert np.abs(s[0] - relu).max() > 1e-2
    seen = set()
    for fam in ("cartpole", "mountain_car", "acrobot", "lunar_lander"):
        D, A, _ = M.FAMILIES[fam]
        pol = rng.normal(0, 1.5, T.n_floats(D, A, 7)).astype(F)
        a, _ = P.header_actions(D, A, 1, M.TANH_FAST, P.GREEDY, (7,), pol, rng.normal(0, 2.0, (D, 256)).astype(F))
        seen.add((fam, len(set(a.tolist())) == A))
    assert all(ok for _, ok in seen), seen
