"""No-GPU checks of the draw of mgym_rollout_mlp_sample: mlp_sample of modurl_gym_amd/csrc/mlp_policy.h (the lines the rollout kernels compile) built for
the host by tests/native/mlp_sample_check.cpp with -ffp-contract=off, against the Python restatement of include/mgym.h's text in tests/mlp_sample_ref.py —
the action and every c_a, word for word (NaN as a class); mg_expm1f against glibc's expm1f on every pattern with the sign bit set; and the distribution of
the specification itself under a constant policy."""
import os
import subprocess

import numpy as np
import pytest

import glibc_f32
import mlp_sample_ref as R
import philox_ref
from oracle import oracle as ora
from words import same_words

needs_fdlibm = pytest.mark.skipif(not glibc_f32.glibc_has_fdlibm_expm1f(), reason="this glibc's expm1f is not the fdlibm one that mg_expm1f restates")


def test_vectorised_philox_equals_the_oracle():
    ora.build()
    rng = np.random.default_rng(5)
    ctr = rng.integers(0, 1 << 32, (64, 4), dtype=np.uint64)
    ctr[:4] = [[0, 0, 0, 0], [0xFFFFFFFF] * 4, [4, 0, 3, philox_ref.SLOT_POLICY_SAMPLE], [0xFFFFFFFC, 1, 0, philox_ref.SLOT_POLICY_SAMPLE + 63]]
    key = (0x34567811, 0x12)
    got = np.stack(philox_ref.philox4x32_10(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], *key), axis=1)
    for row, c in zip(got, ctr):
        assert [int(v) for v in row] == ora.philox([int(v) for v in c], key)
    # words(): env g takes word g % 4 of the block of g & ~3, the key is the seed's two halves, the counter carries call and slot + t
    seed, call, t = 0x1234567811, 3, 5
    for g in (0, 1, 2, 3, 4, 7, 4096 + 2, (1 << 32) + 5):
        blk = ora.philox([(g & ~3) & 0xFFFFFFFF, (g & ~3) >> 32, call, 0x50000000 + t], (seed & 0xFFFFFFFF, seed >> 32))
        assert int(R.words(seed, call, [g], t)[0]) == blk[g % 4]


@needs_fdlibm
def test_bulk_expm1f_is_the_libm_call():
    x = np.concatenate([-np.exp2(np.random.default_rng(1).uniform(-150, 7, 4000)), [0.0, -0.0, -np.inf, np.nan, -104.0, -17.0]]).astype(np.float32)
    assert same_words(glibc_f32.expm1f(x), np.array([glibc_f32.expm1f_scalar(v) for v in x], np.float32))


@needs_fdlibm
@pytest.mark.parametrize("A", [2, 3, 4])
def test_header_equals_the_restatement_on_seeded_cases(A):
    s, w = R.seeded_cases(A)
    assert s.shape == (A, 1 << 16) and np.abs(s).max() <= 20.0
    act, cum = R.header_draw(s, w)
    ract, rcum = R.draw(s, w)
    assert np.array_equal(act, ract) and same_words(cum, rcum)
    assert set(np.unique(act)) == set(range(A))
    assert (act != np.argmax(s, axis=0)).sum() > 1000   # a draw, not the argmax
    assert np.array_equal(R.header_draw(s, w, want_cum=False)[0], act)


@needs_fdlibm
@pytest.mark.parametrize("A", [2, 3, 4])
def test_header_equals_the_restatement_on_hand_built_cases(A):
    s, w = R.hand_cases(A)
    act, cum = R.header_draw(s, w)
    ract, rcum = R.draw(s, w)
    bad = np.nonzero(act != ract)[0]
    assert bad.size == 0, f"case {bad[0]}: scores {s[:, bad[0]]}, word {w[bad[0]]:#x}: header {act[bad[0]]}, restatement {ract[bad[0]]}"
    assert same_words(cum, rcum)
    # facts of the text, on the restatement: a NaN anywhere in c_{A-1} gives A - 1; equal scores give c_a = a + 1; a gap of 104 has weight 0, 17 has 2^-24
    nan_last = np.isnan(rcum[A - 1])
    assert nan_last.sum() > 50 and np.all(ract[nan_last] == A - 1)
    eq = np.all(s == s[0], axis=0) & np.isfinite(s[0])
    assert eq.sum() >= 5 * len(R.SPECIAL_WORDS) and all(np.all(rcum[a, eq] == a + 1) for a in range(A))
    assert np.all(ract[eq & (w == 0)] == 0) and np.all(ract[eq & (w == 0xFFFFFFFF)] == A - 1)
    assert glibc_f32.expm1f_scalar(-104.0) + np.float32(1) == 0.0 and glibc_f32.expm1f_scalar(-17.0) + np.float32(1) == np.float32(2.0 ** -24)
    assert glibc_f32.expm1f_scalar(-16.5) + np.float32(1) == np.float32(2.0 ** -24) and glibc_f32.expm1f_scalar(-18.0) + np.float32(1) == 0.0


@needs_fdlibm
@pytest.mark.parametrize("A", [2, 3, 4])
def test_header_equals_the_restatement_on_the_gap_sweep(A):
    """the probe test's dense sweep of (-104, 0], smaller here"""
    s, w = R.gap_sweep_cases(A, 1 << 17)
    gap = s - s.max(axis=0)
    assert gap.min() > -112.0 and (gap == 0).any(axis=0).all() and ((gap < 0) & (gap > -1e-38)).sum() > 1000
    act, cum = R.header_draw(s, w)
    ract, rcum = R.draw(s, w)
    assert np.array_equal(act, ract) and same_words(cum, rcum)


@needs_fdlibm
def test_expm1f_equals_glibc_on_every_negative_pattern():
    """mg_expm1f(x) and mg_expm1f(x) + 1.0f against glibc on all 2^31 patterns with the sign bit set (NaN results as a class): the draw is specified to the word"""
    exe = R.check_program()
    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    r = subprocess.run([exe, str(threads)], capture_output=True, text=True)
    rows = {l.split()[0]: dict(kv.split("=") for kv in l.split()[1:]) for l in r.stdout.strip().splitlines()}
    assert sorted(rows) == ["expm1f", "expm1f_plus1"], r.stdout + r.stderr
    for fn, row in rows.items():
        assert int(row["total"]) == 1 << 31 and int(row["bad"]) == 0, r.stdout
    assert r.returncode == 0


@needs_fdlibm
@pytest.mark.parametrize("A", [2, 3, 4])
def test_the_specified_draw_follows_the_softmax(A):
    """the specification itself, under the constant policy the GPU test reuses: every action's frequency over 4096 ids x 64 steps within 5 binomial standard
    deviations of the float64 softmax (these seeds stay within 1.9)"""
    acts = R.dist_actions(A)
    assert acts.shape == (R.DIST_K, R.DIST_N)
    dev = R.dist_deviation(acts, A)
    print(f"A={A}: largest deviation {dev:.2f} standard deviations")
    assert dev <= 5.0
    # another call word draws other actions, the same pair the same ones, and a population split over two id ranges draws what the whole one does
    other = R.dist_actions(A, call=R.DIST_CALL + 1, K=4)
    assert not np.array_equal(other, acts[:4]) and np.array_equal(R.dist_actions(A, K=4), acts[:4])
    half = R.DIST_N // 2
    assert np.array_equal(np.concatenate([R.dist_actions(A, n=half, K=4), R.dist_actions(A, n=half, K=4, base=half)], axis=1), acts[:4])
