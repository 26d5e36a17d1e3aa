"""No-GPU check of mgym_logprob_mlp's words: modurl_gym_amd/csrc/logprob.h over the policy headers (the lines the kernels of logprob.hip compile) built for the
host by tests/native/logprob_check.cpp with -ffp-contract=off, against the numpy restatement of include/mgym.h's text in tests/logprob_ref.py (glibc fmaf and
expm1f, float64 operation by operation for mg_log_pos) — every word, no tolerance; the logarithm against libm's float64 log; and the restatement against
float64 log-probabilities of its own f32 scores.

mg_log_pos against libm's float64 log, measured with the native program (log_pos_sweep / log_pos_stats of tests/native/logprob_check.cpp):
    every f32 pattern in [1, 4] (2^24 + 1 of them): largest |error| 1.18e-14, roundings to f32 that differ: 0
    2^20 seeded positive normal floats (uniform over the bit patterns): largest relative error 3.35e-14, roundings to f32 that differ: 0
(the first dropped term of the series, s^17 * 2 / 17 at |s| <= 0.1716, is 3.3e-14 of ln m; every f64 operation adds 1.1e-16).  The asserted bounds are 4 x the
measured figures, the margin of test_gae_host.py and test_value_host.py: 4.72e-14 absolute on [1, 4], 1.34e-13 relative on the sample.

logp against float64 (logprob_ref.logp64_*: numpy float64 log / exp on the restatement's own f32 scores, never the header), on the draws of f64_case — the
widths (64,) and (64, 64), every accepted activation, 2 seeds x 2048 observations per family, scores of order 3, sigma = 0.5:
    categorical head (CartPole, MountainCar, Acrobot, LunarLander; every action of every observation): largest |f32 - f64| = 1.83e-06 at |logp| <= 30.2, largest |sum_a exp(logp_a) - 1| = 2.33e-07
    Gaussian head (MountainCarContinuous, Pendulum): largest |f32 - f64| = 6.96e-07 at |logp| <= 7.49
(d = s_act - m and d - lse each round to f32, half a spacing of 1.9e-6 at magnitude 16 .. 32, on scores that carry their chains' rounding only into both
sides alike; q = z * z and k - 0.5 q each round at half a spacing of 4.8e-7 at magnitude 4 .. 8, and z carries the divide's).  The
asserted bounds are 4 x those, and sum_a exp(logp_a) is within the categorical bound of 1.

logp against the whole network in float64 (logprob_ref.logprob64: dot products, np.tanh, softmax and density in float64 from the same weights — a learner's
own pass), on the draws of net64_case — the same widths and activations, 2 seeds x 2 x 2048 env-steps per family:
    categorical head: largest |f32 - f64| = 5.14e-06 at |logp| <= 27.9        Gaussian head: largest |f32 - f64| = 8.95e-06 at |logp| <= 8.92
(the scores now carry their chains' rounding, about 1e-6 at 64 links of magnitude 3, and mg_tanhf_fast's 2.5 spacings; the Gaussian head multiplies the mean's
error by z / sigma, up to 9 here).  4 x those are logprob_ref.NET64_BOUND, which the torch comparison of test_gpu_logprob_mlp.py uses."""
import numpy as np
import pytest

import families
import logprob_ref as R
from words import same, same_words

F = np.float32
KS = (1, 2, 17)
LOG_ABS_MEASURED, LOG_REL_MEASURED = 1.18e-14, 3.35e-14
LOG_ABS_BOUND, LOG_REL_BOUND = 4 * LOG_ABS_MEASURED, 4 * LOG_REL_MEASURED
F64_MEASURED = {R.SAMPLE: 1.83e-06, R.GAUSS: 6.96e-07}
F64_BOUND = {h: 4 * v for h, v in F64_MEASURED.items()}
NET64_MEASURED, NET64_BOUND = R.NET64_MEASURED, R.NET64_BOUND   # (kept beside the restatement: the device test uses them too)
DISCRETE = [f for f in R.ALL if R.head_of(f) == R.SAMPLE]
CONTINUOUS = [f for f in R.ALL if R.head_of(f) == R.GAUSS]


def test_the_families_are_the_six_pairs():
    assert sorted(R.dims(f) for f in R.ALL) == [(2, 1), (2, 3), (3, 1), (4, 2), (6, 3), (8, 4)]
    assert len(DISCRETE) == 4 and len(CONTINUOUS) == 2


@pytest.mark.parametrize("family", R.ALL)
@pytest.mark.parametrize("K", KS)
def test_header_equals_the_restatement(family, K):
    """every accepted (depth, activation) at small widths, the family's head; n = 1028 also takes the rows four to a lane, n = 1030 only one to a lane"""
    D, A = R.dims(family)
    for n in (1028, 1030):
        for widths in ((17,), (3, 5)):
            for act in R.ACTS[len(widths)]:
                pol, of, ob, acts, exp = R.full_case(family, K, n, widths, act)
                got = R.header_logprob_mlp(pol, D, A, widths, act, of, ob, acts, 0.5)
                assert same(got, exp), (family, K, n, widths, act)
                assert np.isfinite(exp.view(F)).all() and (exp.view(F) <= (0 if A > 1 else 1)).all()   # (a probability, or a density at sigma = 0.5)


@pytest.mark.parametrize("widths", R.WIDTHS, ids=str)
def test_every_width_class(widths):
    """H = 1, a partial chunk of 8, 64; (1, 1), (3, 5), (17, 33), (64, 64) — on LunarLander (categorical, D = 8, A = 4) and Pendulum (Gaussian) at K = 2"""
    for family in ("lunar_lander", "pendulum"):
        D, A = R.dims(family)
        for act in R.ACTS[len(widths)]:
            pol, of, ob, acts, exp = R.full_case(family, 2, 1028, widths, act)
            assert same(R.header_logprob_mlp(pol, D, A, widths, act, of, ob, acts, 0.5), exp), (family, widths, act)


def _constant_call(family, widths, b, actions, impl):
    D, A = R.dims(family)
    c = R.case(family, 1, 8)
    pol = R.packed(R.constant_actor(family, widths, b))
    acts = np.asarray(actions, np.uint32).reshape(1, 8)
    return impl(pol, D, A, widths, R.TANH_FAST, c["obs_first"], c["obs"], acts)[0]


@pytest.mark.parametrize("family", DISCRETE)
@pytest.mark.parametrize("widths", ((3,), (3, 5)), ids=str)
def test_hand_built_scores(family, widths):
    """constant scores: 17, 18 and 104 apart (weight 2^-24 or 0), equal, a NaN, an infinity; and action words >= A"""
    A = R.dims(family)[1]
    cyc = (np.arange(8) % A).astype(np.uint32)
    for gap in (17.0, 18.0, 104.0):
        for best in range(A):
            b = np.full(A, -gap, F)
            b[best] = 0.0
            got = [_constant_call(family, widths, b, cyc, impl) for impl in (R.logprob_mlp, R.header_logprob_mlp)]
            assert same(*got), (gap, best)
            lp = got[0].view(F)
            assert (lp[cyc == best] <= 0).all() and (lp[cyc == best] > -1e-6).all() and (np.abs(lp[cyc != best] + gap) < 1e-5).all(), (gap, best, lp)
            if gap >= 18.0:   # the other weights are 0: c = 1, lse = +0, logp = d exactly
                assert (got[0][cyc == best] == 0).all() and same(lp[cyc != best], np.full(int((cyc != best).sum()), -gap, F))
    for v in (0.0, -0.0, 1.5, -3.0e30):   # equal scores: logp = -(float)ln A for every action
        got = [_constant_call(family, widths, np.full(A, v, F), cyc, impl) for impl in (R.logprob_mlp, R.header_logprob_mlp)]
        assert same(*got) and same(got[0].view(F), np.full(8, -F(R.log_pos(np.array([A], F))[0]), F)), v
    for v in (np.nan, np.inf, -np.inf):   # non-finite scores in every position
        for p in range(A):
            b = np.linspace(-1, 1, A).astype(F)
            b[p] = v
            got = [_constant_call(family, widths, b, cyc, impl) for impl in (R.logprob_mlp, R.header_logprob_mlp)]
            assert same(*got), (v, p)
            if v != -np.inf:
                assert (got[0] == R.NAN_WORD).all(), (v, p)   # a NaN or a +inf score: no softmax sum in [1, A]
            else:
                assert (got[0][cyc == p].view(F) == -np.inf).all() and np.isfinite(got[0][cyc != p].view(F)).all()
    bad = np.array([0, A, A + 1, 0xFFFFFFFF, 1, 0x80000000, A - 1, 1 << 31 | 1], np.uint32)   # action words >= A: the NaN word, no error
    got = [_constant_call(family, widths, np.linspace(-1, 1, A).astype(F), bad, impl) for impl in (R.logprob_mlp, R.header_logprob_mlp)]
    assert same(*got) and ((got[0] == R.NAN_WORD) == (bad >= A)).all()


@pytest.mark.parametrize("family", CONTINUOUS)
@pytest.mark.parametrize("sigma", (R.SIGMA_MIN, R.SIGMA_MAX, 1.0, 0.5), ids=("2^-126", "FLT_MAX", "1", "0.5"))
def test_the_ends_of_sigma(family, sigma):
    """sigma at the smallest normal float and at FLT_MAX: k is finite, a == mu gives k, and every word is the restatement's"""
    D, A = R.dims(family)
    k = R.gauss_k(sigma)
    assert np.isfinite(k) and same(np.array([k]), np.array([R.check_lib().logprob_k(sigma)], F))
    assert abs(float(k) + np.log(float(F(sigma))) + R.HALF_LOG_2PI) <= 2.0 ** -24 * abs(float(k))
    for widths, act in (((17,), R.TANH), ((3, 5), R.RELU)):
        pol, of, ob, acts, _ = R.full_case(family, 2, 1028, widths, act)
        mu = R.row_scores(pol, D, 1, widths, act, R.acted_rows(of, ob))[0]
        for a in (mu, acts, np.where(np.arange(1028) % 2 == 0, F(np.nan), acts).astype(F)):
            exp = R.logprob_mlp(pol, D, A, widths, act, of, ob, a, sigma)
            assert same_words(R.header_logprob_mlp(pol, D, A, widths, act, of, ob, a, sigma), exp), (widths, act)   # (a NaN action's payload is nobody's contract)
        assert same(R.logprob_mlp(pol, D, A, widths, act, of, ob, mu, sigma).view(F), np.full(mu.shape, k, F))


def test_the_sigma_the_call_accepts():
    ok = R.check_lib().logprob_sigma_ok
    for s in (R.SIGMA_MIN, R.SIGMA_MAX, 1.0, 1e-30):
        assert ok(s) == 1, s
    for s in (0.0, -0.0, float(np.nextafter(F(R.SIGMA_MIN), F(0))), 1e-45, -1.0, np.nan, np.inf, -np.inf):
        assert ok(s) == 0, s


def test_log_pos_on_every_float_of_1_to_4():
    """2^24 + 1 patterns in the native program against libm's float64 log: the bound is 4 x the measured 1.18e-14, and no rounding to f32 differs"""
    first, last = int(F(1.0).view(np.uint32)), int(F(4.0).view(np.uint32))
    assert last - first + 1 == (1 << 24) + 1
    worst, _, differ = R.log_pos_sweep(first, last)
    print(f"mg_log_pos on [1, 4]: largest |error| = {worst:.3g} (bound {LOG_ABS_BOUND:.3g}), f32 roundings that differ: {differ}")
    assert worst <= LOG_ABS_BOUND and differ == 0
    x = np.arange(first, last + 1, 16, dtype=np.uint32).view(F)   # the header is the restatement, to the f64 word
    assert np.array_equal(R.header_log_pos(x).view(np.uint64), R.log_pos(x).view(np.uint64))
    assert R.header_log_pos(np.array([1.0], F)).view(np.uint64)[0] == 0   # ln 1 = +0: equal scores 18 apart give lse = +0


def test_log_pos_on_a_sample_of_all_positive_normal_floats():
    """2^20 seeded patterns between the smallest normal float and FLT_MAX, the two ends included: 4 x the measured relative error of 3.35e-14"""
    rng = np.random.default_rng(2024)
    w = rng.integers(0x00800000, 0x7F7FFFFF, 1 << 20, dtype=np.uint64, endpoint=True).astype(np.uint32)
    w[:2] = (0x00800000, 0x7F7FFFFF)
    x = w.view(F)
    _, rel, differ = R.log_pos_stats(x)
    print(f"mg_log_pos on positive normal floats: largest relative error = {rel:.3g} (bound {LOG_REL_BOUND:.3g}), f32 roundings that differ: {differ}")
    assert rel <= LOG_REL_BOUND
    assert np.array_equal(R.header_log_pos(x).view(np.uint64), R.log_pos(x).view(np.uint64))


def f64_case(family, widths, seed):
    rng = np.random.default_rng(150 + seed)
    return R.packed(R.actor_weights(rng, family, widths)), R.value_ref.observations(rng, family, (1,), 2048), rng


@pytest.mark.parametrize("head", (R.SAMPLE, R.GAUSS), ids=("categorical", "gauss"))
def test_against_float64(head):
    worst, top, worst_sum = 0.0, 0.0, 0.0
    for family in (DISCRETE if head == R.SAMPLE else CONTINUOUS):
        D, A = R.dims(family)
        for widths in ((64,), (64, 64)):
            for act in R.ACTS[len(widths)]:
                for seed in range(2):
                    pol, rows, rng = f64_case(family, widths, seed)
                    s = R.row_scores(pol, D, A, widths, act, rows)[:, 0]   # [A, n]
                    if head == R.SAMPLE:
                        l64 = R.logp64_all(s)
                        l32 = np.stack([R.logp_discrete(s, np.full(s.shape[1], a, np.uint32)).view(F) for a in range(A)])
                        worst_sum = max(worst_sum, float(np.abs(np.exp(l32.astype(np.float64)).sum(axis=0) - 1.0).max()))
                    else:
                        a = (s[0] + F(0.5) * rng.standard_normal(s.shape[1]).astype(F)).astype(F)
                        l64, l32 = R.logp64_gauss(s[0], a, 0.5), R.logp_gauss(s[0], a, 0.5).view(F)
                    worst, top = max(worst, float(np.abs(l32 - l64).max())), max(top, float(np.abs(l64).max()))
    print(f"head {head}: largest |f32 - f64| = {worst:.3g} at |logp| <= {top:.3g}, bound {F64_BOUND[head]:.3g}; largest |sum exp(logp) - 1| = {worst_sum:.3g}")
    assert worst <= F64_BOUND[head]
    assert worst_sum <= F64_BOUND[head]


def net64_case(family, widths, seed):
    rng = np.random.default_rng(250 + seed)
    pol = R.packed(R.actor_weights(rng, family, widths))
    return pol, R.value_ref.observations(rng, family, (), 2048), R.value_ref.observations(rng, family, (2,), 2048), rng


@pytest.mark.parametrize("head", (R.SAMPLE, R.GAUSS), ids=("categorical", "gauss"))
def test_against_the_float64_network(head):
    """the restatement against logprob_ref.logprob64 — the whole network, the softmax and the density in float64 from the same weights: what a learner's own
    forward pass gives, and the bound the torch comparison of test_gpu_logprob_mlp.py uses"""
    worst, top = 0.0, 0.0
    for family in (DISCRETE if head == R.SAMPLE else CONTINUOUS):
        D, A = R.dims(family)
        for widths in ((64,), (64, 64)):
            for act in R.ACTS[len(widths)]:
                for seed in range(2):
                    pol, of, ob, rng = net64_case(family, widths, seed)
                    acts = R.actions_for(rng, family, pol, widths, act, of, ob, 0.5)
                    l32 = R.logprob_mlp(pol, D, A, widths, act, of, ob, acts, 0.5).view(F)
                    l64 = R.logprob64(pol, D, A, widths, act, of, ob, acts, 0.5)
                    worst, top = max(worst, float(np.abs(l32 - l64).max())), max(top, float(np.abs(l64).max()))
    print(f"head {head}: largest |f32 - float64 network| = {worst:.3g} at |logp| <= {top:.3g}, bound {NET64_BOUND[head]:.3g}")
    assert worst <= NET64_BOUND[head]
