// Host check of mg_tanhf_fast (MGYM_ACT_TANH_FAST, include/mgym.h): modurl_gym_amd/csrc/mgym_math.h compiled for the host by
//   g++ -O2 -std=c++17 -ffp-contract=off -fno-fast-math -fopenmp -shared -fPIC tanh_fast_check.cpp -lm
// (every cp_fmaf is then glibc's fmaf or the CPU's own FMA instruction: one correctly rounded operation either way).
//   tanh_fast_enumerate  all 2^31 non-negative patterns against float64 tanh: the largest error in f32 spacings of the exact value and in absolute
//                        terms with where they occur, the largest result, the number of places where the result decreases as x grows, the range
//                        of n, the first x whose result is 1.0f, the number of NaN inputs that do not give a NaN, and the number of patterns whose
//                        result with the sign bit set is not the result with its sign bit set (oddness)
//   tanh_fast_bulk       the result words for an array of input words
//   tanh_fast_compare    result words of the patterns first .. first + count - 1 (from the device: mgym_act_probe) against this build's, NaNs as a class:
//                        the number that differ and the first such pattern
// Used by tests/tanh_fast_ref.py; run by tests/test_tanh_fast_host.py.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../modurl_gym_amd/csrc/mgym_math.h"

using namespace mgym;

struct TanhFastStats {
    double max_ulp, max_abs;          // against float64 tanh, over the finite inputs
    uint32_t max_ulp_at, max_abs_at;  // input patterns
    uint32_t max_result;              // the largest result word over the finite inputs and the infinity
    uint32_t first_one;               // the first pattern whose result is 1.0f
    uint32_t inf_result;              // the result word of +inf
    int32_t n_min, n_max;             // the range of n = rintf(u * log2e)
    uint64_t decreases;               // patterns p >= 1 (finite) with result(p) < result(p - 1)
    uint64_t nan_not_nan;             // NaN inputs whose result is not a NaN
    uint64_t not_odd;                 // patterns whose result for -x is not -(result for x), NaNs as a class
    uint64_t negative;                // finite inputs with a result below +0 (sign bit set)
};

// the f32 spacing at the exact value t >= 0: 2^(e - 23) with 2^e <= t < 2^(e+1), 2^-149 below the smallest normal number
static double spacing_at(double t) {
    if (t < 0x1p-126) return 0x1p-149;
    int e;
    frexp(t, &e);   // t = m 2^e, m in [0.5, 1)
    return ldexp(1.0, e - 1 - 23);
}

// n of the text for a = |x| (the one line of the definition this file restates, to report its range)
static int32_t n_of(float a) {
    a = a < 10.0f ? a : 10.0f;
    const float u = -2.0f * a;
    return (int32_t)rintf(u * 0x1.715476p+0f);
}

static void merge(TanhFastStats& s, const TanhFastStats& t) {
    if (t.max_ulp > s.max_ulp || (t.max_ulp == s.max_ulp && t.max_ulp_at < s.max_ulp_at)) { s.max_ulp = t.max_ulp; s.max_ulp_at = t.max_ulp_at; }
    if (t.max_abs > s.max_abs || (t.max_abs == s.max_abs && t.max_abs_at < s.max_abs_at)) { s.max_abs = t.max_abs; s.max_abs_at = t.max_abs_at; }
    if (t.max_result > s.max_result) s.max_result = t.max_result;
    if (t.first_one < s.first_one) s.first_one = t.first_one;
    if (t.n_min < s.n_min) s.n_min = t.n_min;
    if (t.n_max > s.n_max) s.n_max = t.n_max;
    s.decreases += t.decreases;
    s.nan_not_nan += t.nan_not_nan;
    s.not_odd += t.not_odd;
    s.negative += t.negative;
}

extern "C" int tanh_fast_enumerate(TanhFastStats* out) {
    TanhFastStats total;
    memset(&total, 0, sizeof total);
    total.first_one = 0xffffffffu;
    total.n_min = 1 << 30;
    total.n_max = -(1 << 30);
    total.inf_result = as_u32(mg_tanhf_fast(as_f32(0x7f800000u)));
    constexpr uint32_t kChunk = 1u << 16, kChunks = 0x80000000u / kChunk;
#pragma omp parallel
    {
        TanhFastStats s = total;
#pragma omp for schedule(dynamic, 16) nowait
        for (uint32_t c = 0; c < kChunks; ++c) {
            const uint32_t lo = c * kChunk;
            uint32_t prev = lo ? as_u32(mg_tanhf_fast(as_f32(lo - 1u))) : 0u;
            for (uint32_t p = lo; p < lo + kChunk; ++p) {
                const float x = as_f32(p);
                const uint32_t r = as_u32(mg_tanhf_fast(x)), rn = as_u32(mg_tanhf_fast(as_f32(p | 0x80000000u)));
                if (p > 0x7f800000u) {   // a NaN
                    s.nan_not_nan += (r & 0x7fffffffu) > 0x7f800000u ? 0 : 1;
                    s.not_odd += (rn & 0x7fffffffu) > 0x7f800000u ? 0 : 1;
                    continue;
                }
                s.not_odd += rn == (r | 0x80000000u) ? 0 : 1;
                s.negative += r >> 31;
                if (r > s.max_result && !(r >> 31)) s.max_result = r;
                if (r == 0x3f800000u && p < s.first_one) s.first_one = p;
                const int32_t n = n_of(x);
                if (n < s.n_min) s.n_min = n;
                if (n > s.n_max) s.n_max = n;
                if (p == 0x7f800000u) continue;   // the infinity: its result is reported, not compared
                s.decreases += (p >= 1u && r < prev) ? 1 : 0;   // (results are non-negative: the words order as the values do)
                prev = r;
                const double t = tanh((double)x), err = fabs((double)as_f32(r) - t), ulp = err / spacing_at(t);
                if (ulp > s.max_ulp) { s.max_ulp = ulp; s.max_ulp_at = p; }
                if (err > s.max_abs) { s.max_abs = err; s.max_abs_at = p; }
            }
        }
#pragma omp critical
        merge(total, s);
    }
    *out = total;
    return 0;
}

extern "C" void tanh_fast_bulk(uint64_t count, const uint32_t* in, uint32_t* out) {
#pragma omp parallel for
    for (uint64_t i = 0; i < count; ++i) out[i] = as_u32(mg_tanhf_fast(as_f32(in[i])));
}

extern "C" uint64_t tanh_fast_compare(uint32_t first, uint64_t count, const uint32_t* words, uint32_t* first_bad) {
    uint64_t bad = 0;
    uint64_t where = ~0ull;
#pragma omp parallel for reduction(+ : bad) reduction(min : where)
    for (uint64_t i = 0; i < count; ++i) {
        const uint32_t e = as_u32(mg_tanhf_fast(as_f32(first + (uint32_t)i))), g = words[i];
        const bool both_nan = (e & 0x7fffffffu) > 0x7f800000u && (g & 0x7fffffffu) > 0x7f800000u;
        if (g != e && !both_nan) {
            ++bad;
            if (i < where) where = i;
        }
    }
    if (bad && first_bad) *first_bad = first + (uint32_t)where;
    return bad;
}
