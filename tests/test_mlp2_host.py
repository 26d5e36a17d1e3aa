"""No-GPU check of the two-hidden-layer policy header: modurl_gym_amd/csrc/mlp2_policy.h (the lines the rollout kernels and LunarLander's policy kernel compile)
built for the host by tests/native/policy_check.cpp with -ffp-contract=off, against the numpy restatement of include/mgym.h's mgym_rollout_mlp2 text in
tests/mlp2_ref.py (glibc fmaf) — every score and every action word, bit for bit, no tolerance.  The header is evaluated one environment at a time (LunarLander's
form) and, by the check itself, four to a lane (the classic kernels' packed pairs); a difference between the two forms fails header_actions."""
import numpy as np
import pytest

import mlp2_ref as R
import mlp_ref as M
import policy_header as P
from words import words_of

F = np.float32
ACTS = (R.RELU, R.TANH_FAST)
# the observation box each family's observations are drawn over (an unbounded component: a few units of it)
OBS_BOX = {"cartpole": ((-4.8, 4.8), (-5, 5), (-0.42, 0.42), (-5, 5)), "mountain_car": ((-1.2, 0.6), (-0.07, 0.07)),
       "mountain_car_continuous": ((-1.2, 0.6), (-0.07, 0.07)), "pendulum": ((-1, 1), (-1, 1), (-8, 8)),
       "acrobot": ((-1, 1), (-1, 1), (-1, 1), (-1, 1), (-12.57, 12.57), (-28.27, 28.27)),
       "lunar_lander": ((-2.5, 2.5), (-2.5, 2.5), (-10, 10), (-10, 10), (-6.28, 6.28), (-10, 10), (0, 1), (0, 1))}
NAN_COLUMNS = 4   # the last columns of observations(): a NaN in one component


def observations(rng, fam, n=24):
    """[D, n] over the family's box; then columns with +0, -0 and a denormal in one component each, and NAN_COLUMNS columns with a NaN in one component"""
    lo, hi = np.array(OBS_BOX[fam], np.float64).T
    D = len(lo)
    o = rng.uniform(lo[:, None], hi[:, None], (D, n)).astype(F)
    for col, v in zip(range(n - NAN_COLUMNS - 6, n - NAN_COLUMNS), (0.0, -0.0, 1e-40, -1e-40, 0.0, -0.0)):
        o[rng.integers(0, D), col] = F(v)
    for col in range(n - NAN_COLUMNS, n):
        o[rng.integers(0, D), col] = F(np.nan)
    return o


def in_scale(fam):
    return [2.0 / (hi - lo) for lo, hi in OBS_BOX[fam]]


def same_words(got, exp):
    """equal bit patterns; two NaNs are equal whatever their sign and payload"""
    g, e = np.asarray(got, F), np.asarray(exp, F)
    return bool(np.all((words_of(g) == words_of(e)) | (np.isnan(g) & np.isnan(e))))


@pytest.mark.parametrize("fam", list(R.FAMILIES))
def test_header_scores_equal_the_restatement(fam):
    D, A, cont = R.FAMILIES[fam]
    rng = np.random.default_rng(200 + D * 10 + A)
    seen = {"neg1": 0, "pos1": 0, "neg2": 0, "pos2": 0, "nan": 0}
    for H1, H2 in R.SHAPES:
        for act in ACTS:
            pol = R.packed(R.normal_weights(rng, D, A, H1, H2, in_scale(fam)))
            obs = observations(rng, fam)
            s, pre1, pre2 = R.scores(pol, D, A, H1, H2, obs, act, want_pre=True)
            assert pre1.shape == (H1, obs.shape[1]) and pre2.shape == (H2, obs.shape[1])
            got_a, got_s = P.header_actions(D, A, 2, act, P.GREEDY, (H1, H2), pol, obs)
            assert same_words(got_s, s), f"{fam} ({H1}, {H2}) act {act}: header\n{words_of(got_s)}\nrestatement\n{words_of(s)}"
            exp_a = R.head_actions(R.GREEDY, s)
            assert same_words(got_a.view(F), exp_a.view(F)) if cont else np.array_equal(got_a, exp_a)
            seen["neg1"] += int((pre1 < 0).sum()); seen["pos1"] += int((pre1 > 0).sum())
            seen["neg2"] += int((pre2 < 0).sum()); seen["pos2"] += int((pre2 > 0).sum())
            seen["nan"] += int(np.isnan(s).any(axis=0).sum())
    assert all(v > 20 for v in seen.values()), seen   # units of both layers take both signs, and the NaN columns reach the scores


@pytest.mark.parametrize("fam", list(R.FAMILIES))
def test_heads_equal_the_one_layer_heads_on_the_scores(fam):
    D, A, cont = R.FAMILIES[fam]
    rng = np.random.default_rng(300 + D * 10 + A)
    head = R.GAUSS if cont else R.SAMPLE
    n, seed, call, g0, t, sigma = 24, 0x1234567811, 5, 4096, 3, 0.75
    g = np.uint64(g0) + np.arange(n, dtype=np.uint64)
    actions = set()
    for (H1, H2), act in (((3, 5), R.RELU), ((64, 64), R.TANH_FAST), ((17, 33), R.RELU), ((1, 1), R.TANH_FAST)):
        pol = R.packed(R.normal_weights(rng, D, A, H1, H2, in_scale(fam), w3_scale=3.0))
        obs = observations(rng, fam, n)
        s = R.scores(pol, D, A, H1, H2, obs, act)
        # under mg_tanhf_fast a NaN observation component reaches every score (no weight is zero); ReLU turns a NaN pre-activation into +0
        nan = np.isnan(obs).any(axis=0) if act == R.TANH_FAST else np.zeros(n, bool)
        assert act != R.TANH_FAST or (nan[-NAN_COLUMNS:].all() and np.isnan(s[:, nan]).all())
        got, _ = P.header_actions(D, A, 2, act, P.GREEDY, (H1, H2), pol, obs)
        exp = R.head_actions(R.GREEDY, s)
        assert same_words(got.view(F), exp.view(F)) if cont else np.array_equal(got, exp)
        if not cont:
            assert (got[nan] == 0).all()                    # nothing compares greater than a NaN s_0
        else:
            assert np.isnan(got.view(F)[nan]).all()
        got, _ = P.header_actions(D, A, 2, act, head, (H1, H2), pol, obs, sigma, seed, call, g0, t)
        exp = R.head_actions(head, s, sigma, seed, call, g, t)
        if cont:
            assert same_words(got.view(F), exp.view(F)) and np.isnan(got.view(F)[nan]).all()   # NaN + sigma * z
        else:
            assert np.array_equal(got, exp) and (got[nan] == A - 1).all()                        # every comparison with a NaN threshold is false
            actions |= set(int(v) for v in got[~nan])
    if not cont:
        assert actions == set(range(A))


@pytest.mark.parametrize("H", (1, 7, 64))
def test_identity_middle_layer_gives_the_one_layer_scores(H):
    """ReLU, H1 = H2 = H, W2 = I, b2 = +0: pre2_k = fmaf(1, h1_k, ...) over zeros = h1_k exactly (h1 >= +0 and finite), ReLU keeps it, and the last chain is the
    one-layer policy's second chain — so the scores are mlp_policy.h's, word for word"""
    for fam, (D, A, cont) in R.FAMILIES.items():
        rng = np.random.default_rng(400 + H + D)
        one = M.normal_weights(rng, D, A, H, in_scale(fam))
        obs = observations(rng, fam)[:, :-NAN_COLUMNS]   # finite h1
        two = R.packed(R.identity_middle(one, H))
        _, got = P.header_actions(D, A, 2, R.RELU, P.GREEDY, (H, H), two, obs)
        _, exp = P.header_actions(D, A, 1, R.RELU, P.GREEDY, (H,), M.packed(one), obs)
        assert np.isfinite(exp).all()
        assert np.array_equal(words_of(got), words_of(exp)), (fam, H)
        assert np.array_equal(words_of(got), words_of(M.scores(M.packed(one), D, A, H, obs, M.RELU)))


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("fam", ("mountain_car_continuous", "pendulum"))
def test_signed_zero_reaches_the_action_word(fam, act):
    """(H1, H2) = (3, 5): every chain ends in -0 only if it runs over exactly its own terms — fmaf(+0, +0, -0) is +0, so a chain padded with zero weights gives 0"""
    D, A, _ = R.FAMILIES[fam]
    pol = R.packed(R.signed_zero_policy(D, act))
    obs = observations(np.random.default_rng(5), fam)[:, :8]
    exp = R.head_actions(R.GREEDY, R.scores(pol, D, A, 3, 5, obs, act))
    got, _ = P.header_actions(D, A, 2, act, P.GREEDY, (3, 5), pol, obs)
    assert [f"{v:08x}" for v in exp] == ["80000000"] * 8
    assert [f"{v:08x}" for v in got] == ["80000000"] * 8


def test_pack_layout_and_refusals():
    """the check refuses what no family has: a draw on a continuous family, a Gaussian on a discrete one, widths outside 1 .. 64, the exact tanh"""
    lib = P.check_lib()
    z = np.zeros(8192, F)
    out = np.zeros(8, np.uint32)
    call = lambda D, A, act, head, H1, H2: lib.policy_eval(D, A, 2, act, head, H1, H2, z.ctypes.data, 0.0, 4, 4, z.ctypes.data, out.ctypes.data, out.ctypes.data, None)
    assert call(4, 2, R.RELU, R.GREEDY, 64, 64) == 0
    assert call(4, 2, R.RELU, R.GAUSS, 3, 5) == 1 and call(3, 1, R.RELU, R.SAMPLE, 3, 5) == 1
    assert call(4, 2, R.RELU, R.GREEDY, 0, 5) == 1 and call(4, 2, R.RELU, R.GREEDY, 5, 65) == 1
    assert call(4, 2, M.TANH, R.GREEDY, 3, 5) == 1 and call(4, 2, 2, R.GREEDY, 3, 5) == 1
