// Exhaustive comparison of modurl_gym_amd/csrc/mgym_math.h with the host's glibc: every one of the 2^32 f32 bit
// patterns, every sin/cos entry point of the header and mg_tanhf.  Two uses:
//   - executable (tests/test_ll_host.py): the header compiled for the host.  Usage: math_glibc_exhaustive <threads> [stride]
//   - shared library, -DMG_GLIBC_LIB (tests/test_gpu_math_exhaustive.py): mg_glibc_compare() checks result bits the
//     device wrote through mgym_math_probe() against glibc, chunk by chunk.
// Entry points, in the order of MGYM_MATH_* in include/mgym.h:
//   0 sinf  1 cosf  2 sincosf.sin  3 sincosf.cos  4 sincosf_u.sin  5 sincosf_u.cos  6 cosf_u  7 tanhf
// glibc counterparts: sinf, cosf, sincosf, sincosf, sincosf, sincosf, cosf, tanhf (called through pointers, so the
// compiler neither folds nor merges them and the ifunc-selected routine of this host is what runs).
// Compare rule: a NaN result must meet a NaN (any payload: the device's default NaN need not be x86's); every other
// result, infinities included, must be equal bit for bit.  Inputs are classed fast |x| <= 16, mid 16 < |x| < 120,
// large |x| >= 120 (finite), nonfinite (inf / NaN).
// The executable prints "<name> total=<n> bad_fast=<n> bad_mid=<n> bad_large=<n> bad_nonfinite=<n> first=<x,...>" per
// entry point; exit code 0 iff every count is 0.
#define _GNU_SOURCE 1
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include <omp.h>
#include "../../modurl_gym_amd/csrc/mgym_math.h"
using namespace mgym;

namespace {

constexpr int kFns = 8, kClasses = 4, kFirst = 4;
const char* const kNames[kFns] = {"sinf", "cosf", "sincosf.sin", "sincosf.cos", "sincosf_u.sin", "sincosf_u.cos", "cosf_u", "tanhf"};

float (*volatile g_sinf)(float) = sinf;
float (*volatile g_cosf)(float) = cosf;
float (*volatile g_tanhf)(float) = tanhf;
void (*volatile g_sincosf)(float, float*, float*) = sincosf;

void glibc_bits(float x, uint32_t r[kFns]) {
    float s, c;
    g_sincosf(x, &s, &c);
    r[0] = as_u32(g_sinf(x));
    r[1] = as_u32(g_cosf(x));
    r[2] = r[4] = as_u32(s);
    r[3] = r[5] = as_u32(c);
    r[6] = r[1];
    r[7] = as_u32(g_tanhf(x));
}

void header_bits(float x, uint32_t r[kFns]) {
    float s, c, su, cu;
    mg_sincosf(x, &s, &c);
    mg_sincosf_u(x, &su, &cu);
    r[0] = as_u32(mg_sinf(x));
    r[1] = as_u32(mg_cosf(x));
    r[2] = as_u32(s);
    r[3] = as_u32(c);
    r[4] = as_u32(su);
    r[5] = as_u32(cu);
    r[6] = as_u32(mg_cosf_u(x));
    r[7] = as_u32(mg_tanhf(x));
}

bool is_nan(uint32_t b) { return (b & 0x7fffffffu) > 0x7f800000u; }
bool same(uint32_t a, uint32_t b) { return (is_nan(a) || is_nan(b)) ? (is_nan(a) && is_nan(b)) : a == b; }
int input_class(uint32_t u) {
    const uint32_t a = u & 0x7fffffffu;
    return a >= 0x7f800000u ? 3 : (a <= 0x41800000u ? 0 : (a < 0x42f00000u ? 1 : 2));  // 16.0f = 0x41800000, 120.0f = 0x42f00000
}

}  // namespace

// Patterns first, first + stride, ... (count of them).  got: NULL to evaluate the header on the host, else the
// device's result bits, row fn at got + fn * got_stride, column i for pattern first + i * stride.
// bad[fn * 4 + class] receives the mismatch counts; first_bad[fn * 4 + k] the smallest mismatching patterns
// (0xffffffff where fewer).  Both are overwritten.  Returns the total number of mismatches.
extern "C" uint64_t mg_glibc_compare(uint32_t first, uint64_t count, uint32_t stride, const uint32_t* got, uint64_t got_stride,
                                     int nthreads, uint64_t* bad, uint32_t* first_bad) {
    for (int k = 0; k < kFns * kClasses; ++k) bad[k] = 0;
    for (int k = 0; k < kFns * kFirst; ++k) first_bad[k] = 0xffffffffu;
    uint64_t total = 0;
#pragma omp parallel num_threads(nthreads) reduction(+ : total)
    {
        uint64_t lbad[kFns * kClasses] = {0};
        std::vector<uint32_t> lfirst[kFns];
#pragma omp for schedule(static)
        for (int64_t i = 0; i < (int64_t)count; ++i) {
            const uint32_t u = first + (uint32_t)((uint64_t)i * stride);
            const float x = as_f32(u);
            uint32_t ref[kFns], res[kFns];
            glibc_bits(x, ref);
            if (got) {
                for (int f = 0; f < kFns; ++f) res[f] = got[(uint64_t)f * got_stride + (uint64_t)i];
            } else {
                header_bits(x, res);
            }
            for (int f = 0; f < kFns; ++f) {
                if (same(ref[f], res[f])) continue;
                lbad[f * kClasses + input_class(u)]++;
                total++;
                if (lfirst[f].size() < (size_t)kFirst) lfirst[f].push_back(u);
            }
        }
#pragma omp critical
        {
            for (int k = 0; k < kFns * kClasses; ++k) bad[k] += lbad[k];
            for (int f = 0; f < kFns; ++f) {
                std::vector<uint32_t> m(first_bad + f * kFirst, first_bad + (f + 1) * kFirst);
                m.insert(m.end(), lfirst[f].begin(), lfirst[f].end());
                std::sort(m.begin(), m.end());
                std::copy(m.begin(), m.begin() + kFirst, first_bad + f * kFirst);
            }
        }
    }
    return total;
}

// The header's result bits for one entry point (the host twin of the device probe; used by the GPU test's report).
extern "C" uint32_t mg_glibc_header_bits(uint32_t u, int fn) {
    uint32_t r[kFns];
    header_bits(as_f32(u), r);
    return r[fn & 7];
}
extern "C" uint32_t mg_glibc_ref_bits(uint32_t u, int fn) {
    uint32_t r[kFns];
    glibc_bits(as_f32(u), r);
    return r[fn & 7];
}

#ifndef MG_GLIBC_LIB
int main(int argc, char** argv) {
    const int nthreads = argc > 1 ? atoi(argv[1]) : 8;
    const uint32_t stride = argc > 2 ? (uint32_t)atoi(argv[2]) : 1u;
    const uint64_t count = (0x100000000ull + stride - 1) / stride;
    uint64_t bad[kFns * kClasses];
    uint32_t first_bad[kFns * kFirst];
    const uint64_t total = mg_glibc_compare(0u, count, stride, nullptr, 0, nthreads, bad, first_bad);
    for (int f = 0; f < kFns; ++f) {
        printf("%s total=%llu bad_fast=%llu bad_mid=%llu bad_large=%llu bad_nonfinite=%llu first=", kNames[f], (unsigned long long)count,
               (unsigned long long)bad[f * 4 + 0], (unsigned long long)bad[f * 4 + 1], (unsigned long long)bad[f * 4 + 2],
               (unsigned long long)bad[f * 4 + 3]);
        bool any = false;
        for (int k = 0; k < kFirst; ++k)
            if (first_bad[f * kFirst + k] != 0xffffffffu) { printf("%s%a", any ? "," : "", as_f32(first_bad[f * kFirst + k])); any = true; }
        printf("%s\n", any ? "" : "-");
    }
    return total ? 1 : 0;
}
#endif
