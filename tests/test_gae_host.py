"""No-GPU check of the advantage / episode-return scans: modurl_gym_amd/csrc/gae.h (the lines the kernels of gae.hip compile) built for the host by
tests/native/gae_check.cpp with -ffp-contract=off, against the numpy restatement of include/mgym.h's mgym_gae / mgym_episode_returns texts in tests/gae_ref.py
(glibc fmaf) — every word, no tolerance; the restatement itself against exact integer cases, a poison case and the float64 form of the recurrence.

The float64 bound.  On the draws of f64_case (rewards in [-16, 1], values in +-100, gamma 0.99, lambda 0.95, flag rates 0.08, |adv| <= 270) the restatement's
largest deviation from gae64 over 8 seeds x 4096 environments, adv or ret, was measured as
    K = 1: 1.15e-5    K = 2: 2.49e-5    K = 17: 7.02e-5    K = 64: 8.64e-5
(a link rounds three times at magnitudes up to 256, half a spacing of 1.5e-5 each, and gl = 0.94 damps what it inherits: the deviation saturates in K).  The
asserted bound is 4 x the measured maximum, the margin of test_mountain_car_cont_ref.py."""
import numpy as np
import pytest

import gae_ref as R
from words import same

F = np.float32
KS = (1, 2, 17, 64)
F64_MEASURED = {1: 1.15e-5, 2: 2.49e-5, 17: 7.02e-5, 64: 8.64e-5}
F64_BOUND = {K: 4 * v for K, v in F64_MEASURED.items()}
N = 1028


def f64_case(K, seed=0, n=4096):
    rng = np.random.default_rng(1000 + K * 10 + seed)
    r, v = rng.uniform(-16, 1, (K, n)).astype(F), rng.uniform(-100, 100, (K, n)).astype(F)
    lv = rng.uniform(-100, 100, n).astype(F)
    d, u = R.flags(rng, K, n)
    fv = rng.uniform(-100, 100, (K, n)).astype(F)
    return r, d, u, v, lv, fv


def exact_case(K, n=N, seed=7):
    rng = np.random.default_rng(seed + K)
    r = rng.integers(-3, 4, (K, n)).astype(F)
    d = (rng.random((K, n)) < 0.15).astype(np.uint8)
    return r, d


def both_equal(got, exp):
    return same(got[0], exp[0]) and same(got[1], exp[1])


@pytest.mark.parametrize("K", KS)
def test_header_equals_the_restatement(K):
    r, d, u, v, lv, fv = f64_case(K, n=N)
    R.check_coverage(d, u)
    for dd, uu, ff in ((d, u, fv), (d, u, None), (None, u, fv), (d, None, fv), (None, None, None), (None, None, fv)):
        for gamma, lam in ((0.99, 0.95), (1.0, 1.0), (0.9, 0.0), (0.0, 0.5)):
            assert both_equal(R.header_gae(r, dd, uu, v, lv, ff, gamma, lam), R.gae(r, dd, uu, v, lv, ff, gamma, lam)), (K, gamma, lam)
    acc0, len0 = np.random.default_rng(K).uniform(-50, 0, N).astype(F), np.random.default_rng(K).integers(0, 200, N).astype(np.uint32)
    for dd, uu in ((d, u), (d, None), (None, u), (None, None)):
        got, exp = R.header_episode_returns(r, dd, uu, acc0, len0), R.episode_returns(r, dd, uu, acc0, len0)
        assert all(same(g, e) for g, e in zip(got, exp)), K


@pytest.mark.parametrize("K", KS)
def test_integer_rewards_give_exact_sums(K):
    """gamma = lambda = 1, value = 0: ret = adv = the sum of the rewards from t to the episode's end (or the call's), exact in f32"""
    r, d = exact_case(K)
    n = r.shape[1]
    zero = np.zeros((K, n), F)
    expected = np.zeros((K, n), np.int64)
    run = np.zeros(n, np.int64)
    for t in range(K - 1, -1, -1):
        run = np.where(d[t] != 0, 0, run) + r[t].astype(np.int64)
        expected[t] = run
    for impl in (R.gae, R.header_gae):
        adv, ret = impl(r, d, None, zero, np.zeros(n, F), None, 1.0, 1.0)
        assert np.array_equal(adv.astype(np.int64), expected) and np.array_equal(adv, adv.astype(np.int64)) and same(np.abs(ret), np.abs(adv))
    # the forward scan over the same rewards: every finished episode's return is the sum of its rewards, its length the distance to the previous end
    for impl in (R.episode_returns, R.header_episode_returns):
        acc, length, ret_out, len_out = impl(r, d, None, np.zeros(n, F), np.zeros(n, np.uint32))
        run, steps = np.zeros(n, np.int64), np.zeros(n, np.int64)
        for t in range(K):
            run, steps = run + r[t].astype(np.int64), steps + 1
            fin = d[t] != 0
            assert np.array_equal(ret_out[t][fin].view(F).astype(np.int64), run[fin]) and np.array_equal(len_out[t][fin], steps[fin])
            assert (ret_out[t][~fin] == R.NAN_WORD).all() and (len_out[t][~fin] == R.NAN_WORD).all()
            run, steps = np.where(fin, 0, run), np.where(fin, 0, steps)
        assert np.array_equal(acc.astype(np.int64), run) and np.array_equal(length, steps)


@pytest.mark.parametrize("K", KS)
def test_lambda_zero_is_the_td_error(K):
    r, d, u, v, lv, fv = f64_case(K, n=N)
    nxt = np.concatenate([v[1:], lv[None]])
    fin, dn = (d | u) != 0, d != 0
    nv = np.where(fin, np.where(dn, F(0), fv), nxt).astype(F)
    delta = (R.glibc_f32.fmaf(np.full_like(r, F(0.99)), nv, r) - v).astype(F)
    for impl in (R.gae, R.header_gae):
        adv, ret = impl(r, d, u, v, lv, fv, 0.99, 0.0)
        assert np.array_equal(adv, delta) and same(ret, (adv + v).astype(F))   # (fmaf(+0, c, delta) is delta as a value; a -0 delta becomes +0)


@pytest.mark.parametrize("K1,K2", [(1, 1), (5, 12), (17, 64)])
def test_two_calls_leave_the_words_of_one(K1, K2):
    rng = np.random.default_rng(K1 * 100 + K2)
    K = K1 + K2
    r = rng.uniform(-16, 1, (K, N)).astype(F)
    d, u = R.flags(rng, K, N)
    acc0, len0 = rng.uniform(-5, 5, N).astype(F), rng.integers(0, 9, N).astype(np.uint32)
    for impl in (R.episode_returns, R.header_episode_returns):
        for dd, uu in ((d, u), (None, None)):   # (every flag 0: nothing is emitted and the carry alone tells)
            one = impl(r, dd, uu, acc0, len0)
            a = impl(r[:K1], None if dd is None else dd[:K1], None if uu is None else uu[:K1], acc0, len0)
            b = impl(r[K1:], None if dd is None else dd[K1:], None if uu is None else uu[K1:], a[0], a[1])
            assert same(b[0], one[0]) and same(b[1], one[1])
            assert same(np.concatenate([a[2], b[2]]), one[2]) and same(np.concatenate([a[3], b[3]]), one[3])
            if dd is None:
                assert (one[2] == R.NAN_WORD).all() and np.array_equal(one[1], len0 + np.uint32(K))


@pytest.mark.parametrize("K", KS)
def test_unselected_words_reach_no_result(K):
    """final_value is the NaN word except where trunc && !done; value, reward and last_value of the odd environments are NaN: every output of an even
    environment is finite and equals the run without the poison"""
    r, d, u, v, lv, fv = f64_case(K, n=N)
    rng = np.random.default_rng(3)
    clean_fv = fv
    fv = np.where((u != 0) & (d == 0), fv, R.poisoned_final_value(rng, d, u))
    assert np.isnan(fv).sum() >= fv.size // 2 and not np.isnan(fv[(u != 0) & (d == 0)]).any()
    pv, pr, plv = v.copy(), r.copy(), lv.copy()
    pv[:, 1::2], pr[:, 1::2], plv[1::2] = np.nan, np.nan, np.nan
    for impl in (R.gae, R.header_gae):
        clean = impl(r, d, u, v, lv, clean_fv, 0.99, 0.95)
        got = impl(pr, d, u, pv, plv, fv, 0.99, 0.95)
        for g, c in zip(got, clean):
            assert np.isfinite(g[:, 0::2]).all() and same(g[:, 0::2], c[:, 0::2])
            assert np.isnan(g[:, 1::2]).all()
    # a NaN carried into an episode's end stops there: env 0 of a 2-step call ends at t = 0 with NaN everywhere after it
    rr, vv = np.array([[1.0], [np.nan]], F), np.array([[2.0], [np.nan]], F)
    for impl in (R.gae, R.header_gae):
        adv, ret = impl(rr, np.array([[1], [0]], np.uint8), None, vv, np.array([np.nan], F), None, 0.99, 0.95)
        assert adv[0, 0] == F(-1.0) and ret[0, 0] == F(1.0) and np.isnan(adv[1, 0])


@pytest.mark.parametrize("K", KS)
def test_against_float64(K):
    worst = 0.0
    for seed in range(2):
        r, d, u, v, lv, fv = f64_case(K, seed)
        a64, t64 = R.gae64(r, d, u, v, lv, fv, 0.99, 0.95)
        for impl in (R.gae, R.header_gae):
            adv, ret = impl(r, d, u, v, lv, fv, 0.99, 0.95)
            worst = max(worst, float(np.abs(adv - a64).max()), float(np.abs(ret - t64).max()))
        assert np.abs(a64).max() <= 270
    print(f"K = {K}: largest |f32 - f64| = {worst:.3g}, bound {F64_BOUND[K]:.3g}")
    assert worst <= F64_BOUND[K]
