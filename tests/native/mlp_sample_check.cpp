// CPU check of the draw of mgym_rollout_mlp_sample (mlp_sample of modurl_gym_amd/csrc/mlp_policy.h, the lines the kernels compile), built with
// g++ -ffp-contract=off.
//   as a shared object (tests/mlp_sample_ref.py): mlp_sample_eval over n cases
//   as a program (tests/test_mlp_sample_host.py; -fopenmp): "mlp_sample_check <threads>" runs mg_expm1f(x) and mg_expm1f(x) + 1.0f against glibc's expm1f
//     on all 2^31 bit patterns with the sign bit set (NaN results compared as a class) and prints "expm1f total=.. bad=.." and "expm1f_plus1 total=.. bad=.."
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../modurl_gym_amd/csrc/mlp_policy.h"

using namespace mgym;

template <int A>
static void eval(uint64_t n, const float* scores, const uint32_t* words, uint32_t* actions, float* cum) {
    for (uint64_t i = 0; i < n; ++i) {
        float s[A], c[A];
        for (int a = 0; a < A; ++a) s[a] = scores[(uint64_t)a * n + i];
        actions[i] = mlp_sample<A>(s, words[i]);
        if (cum) {
            mlp_sample_cum<A>(s, c);
            for (int a = 0; a < A; ++a) cum[(uint64_t)a * n + i] = c[a];
        }
    }
}

// scores: [A][n] floats; words, actions: [n]; cum: [A][n] or NULL.  Returns 0, or 1 for an A outside 2 .. 4.
extern "C" int mlp_sample_eval(int A, uint64_t n, const float* scores, const uint32_t* words, uint32_t* actions, float* cum) {
    if (A == 2) eval<2>(n, scores, words, actions, cum);
    else if (A == 3) eval<3>(n, scores, words, actions, cum);
    else if (A == 4) eval<4>(n, scores, words, actions, cum);
    else return 1;
    return 0;
}

static bool same(float a, float b) {
    if (a != a || b != b) return (a != a) == (b != b);
    uint32_t u, v;
    memcpy(&u, &a, 4);
    memcpy(&v, &b, 4);
    return u == v;
}

int main(int argc, char** argv) {
    const int threads = argc > 1 ? atoi(argv[1]) : 1;
    unsigned long long bad = 0, bad1 = 0;
#pragma omp parallel for num_threads(threads) reduction(+ : bad, bad1) schedule(static)
    for (long long p = 0x80000000ll; p <= 0xffffffffll; ++p) {
        const float x = as_f32((uint32_t)p);
        volatile float xv = x;   // (no constant folding, no builtin expansion of the libm call)
        const float ref = expm1f(xv), got = mg_expm1f(x);
        bad += !same(got, ref);
        bad1 += !same(got + 1.0f, ref + 1.0f);
    }
    printf("expm1f total=%llu bad=%llu\nexpm1f_plus1 total=%llu bad=%llu\n", 1ull << 31, bad, 1ull << 31, bad1);
    return bad || bad1 ? 1 : 0;
}
