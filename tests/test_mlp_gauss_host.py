"""No-GPU checks of the draw of mgym_rollout_mlp_gauss: mg_log_u25, mlp_gauss_pair and the GAUSS form of mlp_actions of modurl_gym_amd/csrc/mlp_policy.h
(the lines the rollout kernels compile) built for the host by tests/native/mlp_gauss_check.cpp and policy_check.cpp with -ffp-contract=off, against the numpy restatement of
include/mgym.h's text in tests/mlp_gauss_ref.py — z_even, z_odd and q word for word over every k1; the restated logarithm against numpy's log / log1p; and
the distribution of the specification itself under a constant policy."""
import numpy as np
import pytest

import mlp_gauss_ref as R
import mlp_ref as M
import policy_header as P
from oracle import oracle as ora
from philox_ref import SLOT_POLICY_GAUSS, philox4x32_10
from words import same_words

F = np.float32


@pytest.fixture(scope="module")
def cases():
    wa, wb = R.all_cases()
    return wa, wb, R.gauss_pair(wa, wb), R.header_pair(wa, wb, want_log=True)


def test_header_equals_the_restatement_on_every_k1(cases):
    wa, wb, (rze, rzo, rq), (hze, hzo, hq, hL) = cases
    assert wa.size == (1 << 24) + len(R.K1_HAND) * len(R.K2_HAND)
    assert np.array_equal((wa[: 1 << 24] >> 8), np.arange(1 << 24, dtype=np.uint32))          # every k1
    assert {0, 1, (1 << 23) - 1, 1 << 23, (1 << 24) - 1, 3, 5, (1 << 22) - 1, (1 << 22) + 1} <= set(R.K1_HAND)
    for nm, h, r in (("q", hq, rq), ("z_even", hze, rze), ("z_odd", hzo, rzo)):
        bad = np.nonzero(h.view(np.uint32) != r.view(np.uint32))[0]
        assert bad.size == 0, f"{nm}: {bad.size} words differ; first at wa {wa[bad[0]]:#x} wb {wb[bad[0]]:#x}: header {h[bad[0]]!r}, restatement {r[bad[0]]!r}"
    # the header's f64 logarithm is the restated one to the last bit
    n = (wa >> np.uint32(8)).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    assert np.array_equal(hL.view(np.uint64), R.log_u25(n).view(np.uint64))
    # the low 8 bits of a word do not matter
    lo = R.header_pair(wa[:4096] ^ np.uint32(0xA5), wb[:4096] ^ np.uint32(0x5A))
    assert all(np.array_equal(a.view(np.uint32), b[:4096].view(np.uint32)) for a, b in zip(lo, (hze, hzo, hq)))


def test_axis_angles_and_extremes(cases):
    wa, wb, (rze, rzo, rq), _ = cases
    k1, k2 = wa >> np.uint32(8), wb >> np.uint32(8)
    assert np.all(rq > 0) and np.all(np.isfinite(rze)) and np.all(np.isfinite(rzo))
    r = np.sqrt(rq)
    print(f"largest r {r.max():.6f} (k1 = {int(k1[np.argmax(r)])}), smallest q {rq.min():.3e}")
    assert int(k1[np.argmax(r)]) == 0 and abs(float(r.max()) - np.sqrt(50.0 * np.log(2.0))) < 1e-6 and float(r.max()) < R.R_MAX
    assert max(np.abs(rze).max(), np.abs(rzo).max()) <= R.R_MAX
    # k2 = 0: phi = 0, so z_even = r and z_odd = 0; k2 = 2^23: phi = pi_f, z_even = -r to the word (cosf(pi_f) = -1)
    z0 = k2 == 0
    assert z0.sum() >= len(R.K1_HAND) and np.array_equal(rze[z0], r[z0]) and np.all(rzo[z0] == 0)
    zp = k2 == (1 << 23)
    assert zp.sum() >= len(R.K1_HAND) and np.array_equal(rze[zp], -r[zp]) and np.all(np.abs(rzo[zp]) < 1e-6 * r[zp])
    # the mean of q over all k1 is E[-2 ln U] = 2
    assert abs(float(rq[: 1 << 24].astype(np.float64).mean()) - 2.0) < 1e-6


def test_restated_logarithm_is_within_2_pow_minus_40_of_float64_log():
    """3.3e-14 of truncation (s^16 / 17 at s = 0.1716) plus about 10 roundings of 2^-53, against 2^-40 = 9.1e-13"""
    n = np.arange(1 << 24, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    L, ref = R.log_u25(n), R.log_reference(n)
    assert np.all(L < 0) and np.all(ref < 0)
    rel = np.abs((L - ref) / ref)
    print(f"largest relative error of mg_log_u25 against log / log1p: {rel.max():.3e} at n = {int(n[np.argmax(rel)])}")
    assert rel.max() <= 2.0 ** -40


def test_gauss_philox_words_are_the_oracles():
    ora.build()
    seed, call, t = 0x1234567811, 3, 5
    for g in (0, 1, 2, 3, 4, 7, 4096 + 2, (1 << 32) - 1, (1 << 32) + 5, (1 << 32) + 6):
        blk = ora.philox([(g & ~3) & 0xFFFFFFFF, (g & ~3) >> 32, call, 0x60000000 + t], (seed & 0xFFFFFFFF, seed >> 32))
        wa, wb, odd = R.pair_words(seed, call, [g], t)
        assert (int(wa[0]), int(wb[0]), bool(odd[0])) == (blk[2 * ((g >> 1) & 1)], blk[2 * ((g >> 1) & 1) + 1], bool(g & 1)), g


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("act", [M.RELU, M.TANH])
def test_lane_form_equals_the_restatement(D, act):
    """the GAUSS form of mlp_actions (four environments per Philox block) against mu from the restated fmaf chains and a = mu + sigma * z; ids straddle 2^32"""
    rng = np.random.default_rng(40 + D + act)
    n, g0 = 512, (1 << 32) - 256
    g = np.uint64(g0) + np.arange(n, dtype=np.uint64)
    for H in (1, 5, 64):
        w1, b1 = rng.normal(0, 1, (H, D)).astype(F), rng.normal(0, 0.5, H).astype(F)
        w2, b2 = (rng.normal(0, 1, (1, H)) / np.sqrt(H)).astype(F), rng.normal(0, 0.3, 1).astype(F)
        pol = np.concatenate([w1.ravel(), b1, w2.ravel(), b2]).astype(F)
        obs = rng.uniform(-2, 2, (D, n)).astype(F)
        obs[0, :4] = [np.nan, np.inf, -0.0, 0.0]
        mu = M.scores(pol, D, 1, H, obs, act)[0]
        for sigma in (0.0, 0.3, 2.5):
            got = P.header_actions(D, 1, 1, act, P.GAUSS, (H,), pol, obs, sigma, 0xC0FFEE1234, 9, g0, 3)[0].view(F)
            exp = R.gauss_actions(mu, sigma, 0xC0FFEE1234, 9, g, 3)
            assert same_words(got, exp), (H, sigma)
            if sigma == 0.0:
                assert np.array_equal(got[4:], mu[4:])          # a = mu as values
            else:
                assert (got[4:] != mu[4:]).sum() > n - 16
        assert np.isnan(got[0]) == (act == M.TANH)              # a NaN mu gives a NaN action (ReLU turns a NaN pre-activation into +0)


def test_the_specified_draw_is_standard_normal():
    """the specification itself, under the constant policy (mu = 0, sigma = 1) the GPU test reuses, over 4096 ids x 64 steps: mean within 5 / sqrt(N), variance
    within 5 sqrt(2 / N) of 1, even / odd pair correlation within 5 / sqrt(N / 2) of 0, Kolmogorov-Smirnov distance to Phi below 1.95 / sqrt(N)"""
    z = R.dist_actions()
    assert z.shape == (R.DIST_K, R.DIST_N) and z.dtype == F
    mean, var, corr, ks = R.dist_deviations(z)
    print(f"mean {mean:+.2f}, variance {var:+.2f}, pair correlation {corr:+.2f} standard errors; KS distance {ks:.3f} / sqrt(N)")
    assert abs(mean) <= 5.0 and abs(var) <= 5.0 and abs(corr) <= 5.0 and ks < 1.95
    # another call word draws other actions, the same pair the same ones, and a population split over two id ranges draws what the whole one does
    other = R.dist_actions(call=R.DIST_CALL + 1, K=4)
    assert not np.array_equal(other, z[:4]) and np.array_equal(R.dist_actions(K=4), z[:4])
    half = R.DIST_N // 2
    assert np.array_equal(np.concatenate([R.dist_actions(n=half, K=4), R.dist_actions(n=half, K=4, base=half)], axis=1), z[:4])


def test_ids_beyond_2_pow_32_use_the_high_counter_word():
    seed, call, t = 77, 1, 2
    lo, hi = np.arange(8, dtype=np.uint64), np.uint64(1 << 32) + np.arange(8, dtype=np.uint64)
    zl, zh = R.normals(seed, call, lo, t), R.normals(seed, call, hi, t)
    assert not np.array_equal(zl, zh)
    w = philox4x32_10(np.uint64(4), np.uint64(1), np.uint64(call), np.uint64(SLOT_POLICY_GAUSS + t), seed, 0)
    ze, zo, _ = R.gauss_pair(np.array([w[0][()], w[2][()]], np.uint32), np.array([w[1][()], w[3][()]], np.uint32))
    assert same_words(zh[4:], np.array([ze[0], zo[0], ze[1], zo[1]], F))
    # a population straddling 2^32 draws what its two halves draw
    base = (1 << 32) - 4
    whole = R.dist_actions(n=8, K=3, base=base)
    assert np.array_equal(np.concatenate([R.dist_actions(n=4, K=3, base=base), R.dist_actions(n=4, K=3, base=1 << 32)], axis=1), whole)
