"""No-GPU check of MGYM_ACT_TANH_FAST: mg_tanhf_fast of modurl_gym_amd/csrc/mgym_math.h compiled for the host with g++ -ffp-contract=off
(tests/native/tanh_fast_check.cpp, OpenMP) against float64 tanh over all 2^31 non-negative patterns, and against the restatement of include/mgym.h's
text in tests/tanh_fast_ref.py (glibc's fmaf), bit for bit.

The two error bounds are conditions on fitness for purpose, not measurements: a hidden unit feeds an fmaf chain whose own terms round at 2^-24 relative,
and an activation within 2^-22 absolute (4 f32 spacings of the exact value) is of the same order.  Measured with true fmaf: 2.498 spacings and 1.489e-7,
both at x = 4.5050907 (0x409029b4); the first x with result 1.0f is 8.4910536 (0x4107db5b)."""
import numpy as np
import pytest

import tanh_fast_ref as T
from philox_ref import philox4x32_10

F = np.float32
MAX_SPACINGS = 4.0
MAX_ABS = 2.0 ** -22


@pytest.fixture(scope="module")
def stats():
    st = T.enumerate_all()
    f32 = lambda u: float(np.uint32(u).view(F))   # noqa: E731
    print(f"\nmg_tanhf_fast over 2^31 patterns against float64 tanh: largest error {st.max_ulp:.4f} f32 spacings at x = {f32(st.max_ulp_at)!r} "
          f"({st.max_ulp_at:#010x}), largest absolute error {st.max_abs:.4e} at x = {f32(st.max_abs_at)!r} ({st.max_abs_at:#010x}), largest result "
          f"{f32(st.max_result)!r}, first x with result 1.0f {f32(st.first_one)!r} ({st.first_one:#010x}), n in {st.n_min} .. {st.n_max}, "
          f"decreases {st.decreases}, NaN inputs without a NaN result {st.nan_not_nan}, patterns that break oddness {st.not_odd}")
    return st


def test_error_against_float64_tanh_on_every_non_negative_pattern(stats):
    assert stats.max_ulp <= MAX_SPACINGS, (stats.max_ulp, hex(stats.max_ulp_at))
    assert stats.max_abs <= MAX_ABS, (stats.max_abs, hex(stats.max_abs_at))


def test_no_result_above_one_none_negative_and_never_decreasing(stats):
    assert stats.max_result == 0x3F800000   # 1.0f is reached and never exceeded
    assert stats.negative == 0
    assert stats.decreases == 0
    assert 0 < stats.first_one < 0x41200000   # below the clamp


def test_n_stays_within_the_exponent_range_of_the_text(stats):
    assert (stats.n_min, stats.n_max) == (-29, 0)


def test_infinity_gives_one_and_every_nan_gives_a_nan(stats):
    assert stats.inf_result == 0x3F800000
    assert stats.nan_not_nan == 0


def test_odd_on_every_pattern(stats):
    """the result for x with the sign bit set is the result for x with its sign bit set, -0 included"""
    assert stats.not_odd == 0
    assert T.words_of(T.header_tanh_fast(np.array([0.0, -0.0], F))).tolist() == [0, 0x80000000]


def n_change_patterns():
    """the 29 a at which n steps down (the ties of u * log2e), each with both f32 neighbours: n is non-increasing in a, so each step is found by bisection"""
    out = []
    for k in range(1, 30):
        lo, hi = 0, 0x41200000   # n(lo) > -k, n(hi) = -29 <= -k
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if float(T.n_of(np.array([mid], np.uint32).view(F))[0]) <= -k:
                hi = mid
            else:
                lo = mid
        out += [hi - 2, hi - 1, hi, hi + 1]
    return out


def fixed_cases():
    bits = [0x00000000, 0x80000000, 0x00000001, 0x007FFFFF, 0x80000001, 0x807FFFFF, 0x33000000, 0xB3000000]   # +-0, the denormals' ends, 2^-25
    steps = n_change_patterns()
    assert len(steps) == 29 * 4
    bits += steps + [b | 0x80000000 for b in steps]
    bits += [0x411FFFFF, 0x41200000, 0x41200001, 0xC11FFFFF, 0xC1200000, 0xC1200001]   # 10.0f and its neighbours
    bits += [int(F(12.0).view(np.uint32)), int(F(1e30).view(np.uint32)), int(F(-12.0).view(np.uint32)), int(F(-1e30).view(np.uint32))]
    bits += [0x7F800000, 0xFF800000, 0x7FC00000, 0x7FA00000, 0xFFC00000, 0xFF800001]   # +-inf, quiet and signalling NaNs
    idx = np.arange(1 << 18, dtype=np.uint64)
    drawn = np.concatenate(philox4x32_10(idx, 0, 0, 0, 0x7A6E4866, 0x61737400))   # 2^20 Philox-drawn patterns
    assert drawn.size == 1 << 20
    return np.concatenate([np.array(bits, np.uint32), drawn])


def test_header_equals_the_restatement_of_the_text_bit_for_bit():
    w = fixed_cases()
    x = w.view(F)
    got, exp = T.header_tanh_fast(x), T.tanh_fast(x)
    same = (T.words_of(got) == T.words_of(exp)) | (np.isnan(got) & np.isnan(exp))
    bad = np.flatnonzero(~same)
    assert bad.size == 0, [(hex(int(w[i])), hex(int(T.words_of(got)[i])), hex(int(T.words_of(exp)[i]))) for i in bad[:8]]
    # the set reaches what it names: every n, NaNs, both signs, denormal inputs
    n = T.n_of(x[np.isfinite(x)])
    assert set(np.unique(n).astype(int)) == set(range(-29, 1))
    assert np.isnan(got).sum() >= 4 and (w >> 31).any() and ((w & 0x7FFFFFFF) < 0x00800000).sum() > 6
