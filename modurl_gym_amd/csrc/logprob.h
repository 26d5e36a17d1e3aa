// logprob.h — the words of mgym_logprob_mlp (include/mgym.h): the log-probability of the action a rollout drew, under the distribution it was drawn from.  Shared
// by the kernels of logprob.hip (four environments per lane, or one) and the host check tests/native/logprob_check.cpp, which compiles this header with g++
// (mgym_math.h's MG_HD is empty there).  Compile with -ffp-contract=off: the only fused operations are the cp_fmaf of the policy headers' chains.
//
//   scores   s_a of mlp_scores<D, A, ACT, N> under the actor (mlp_policy.h's MlpPack<D, A>, or mlp2_policy.h's Mlp2Net<D, A>), on the observation row
//            value.h's value_row_in gives step t: t == 0 ? obs_first : obs[t - 1]
//   discrete (A >= 2)   m, e_a, c_{A-1} of mlp_sample_cum;  lse = (float)mg_log_pos(c_{A-1});  d = s_act - m ((m - m) for the best action);  logp = d - lse;
//                       the quiet NaN 0x7fc00000 unless 1 <= c_{A-1} <= A and the action word is below A
//   Gaussian (A == 1)   z = (a - s_0) / sigma;  q = z * z;  logp = k - 0.5f * q,  k = (float)(-(mg_log_pos(sigma) + 0.91893853320467274)) once on the host
// f32 throughout except mg_log_pos, which is f64; nothing reassociated, and every selection is a selection (no branch depends on a lane's data).
#pragma once
#include <stdint.h>
#include "value.h"

namespace mgym {

// ln x in f64 for a positive normal f32 x: the series of mlp_policy.h's mg_log_u25, which stays as it is.  x = m 2^e with m in [1, 2) — read from x's own
// bits, which are those of (double)x: the conversion is exact — then m in (sqrt(1/2), sqrt(2)], s = (m - 1) / (m + 1), ln m = 2 atanh(s) as the odd series up to
// s^15, Horner in s^2 from 2/15 down to 2, and e ln2 + that.  Every operation individually rounded; any other x gives a defined, meaningless double.
MG_HD double mg_log_pos(float x) {
    const uint32_t bx = as_u32(x);
    const int e0 = (int)(bx >> 23) - 127;
    const double m0 = (double)as_f32((bx & 0x007fffffu) | 0x3f800000u);
    const bool big = m0 > 0x1.6a09e667f3bcdp+0;
    const double m = big ? m0 * 0.5 : m0;
    const int e = big ? e0 + 1 : e0;
    const double s = (m - 1.0) / (m + 1.0);
    const double s2 = s * s;
    double p = 2.0 / 15.0;
    p = p * s2 + 2.0 / 13.0;
    p = p * s2 + 2.0 / 11.0;
    p = p * s2 + 2.0 / 9.0;
    p = p * s2 + 2.0 / 7.0;
    p = p * s2 + 2.0 / 5.0;
    p = p * s2 + 2.0 / 3.0;
    p = p * s2 + 2.0;
    p = p * s;
    return (double)e * 0x1.62e42fefa39efp-1 + p;
}

constexpr uint32_t kLogpNaN = 0x7fc00000u;   // what the call writes where the action has no log-probability

// the categorical head: log softmax(s)[act] through the draw's own weights
template <int A>
MG_HD float logp_discrete(const float (&s)[A], uint32_t act) {
    static_assert(A >= 2, "a categorical distribution needs two actions");
    float c[A];
    mlp_sample_cum<A>(s, c);
    float m = s[0], sa = s[0];   // m and the best index as mlp_sample_cum finds them; sa = s_act (s_0 for an action word that is refused below)
    uint32_t b = 0u;
#pragma unroll
    for (int a = 1; a < A; ++a) {
        const bool up = s[a] > m;
        m = up ? s[a] : m;
        b = up ? (uint32_t)a : b;
        sa = act == (uint32_t)a ? s[a] : sa;
    }
    const float d = act == b ? m - m : sa - m;
    const float lse = (float)mg_log_pos(c[A - 1]);
    const float logp = d - lse;
    const bool ok = c[A - 1] >= 1.0f && c[A - 1] <= (float)A && act < (uint32_t)A;   // (a NaN sum fails the first test)
    return ok ? logp : as_f32(kLogpNaN);
}

// the Gaussian head: k is logp_gauss_k(sigma), the divide the correctly rounded f32 one
MG_HD float logp_gauss(float mu, float a, float sigma, float k) {
    const float z = (a - mu) / sigma;
    const float q = z * z;
    return k - 0.5f * q;
}
MG_HD float logp_gauss_k(float sigma) { return (float)(-(mg_log_pos(sigma) + 0.91893853320467274)); }
// the sigma the call accepts: a finite, normal, positive f32
MG_HD bool logp_sigma_ok(float sigma) { return sigma >= 1.17549435e-38f && sigma <= 3.402823466e+38f; }

// the head the family has: one score is a mean, more are logits
template <int A>
MG_HD float logp_head(const float (&s)[A], uint32_t word, float sigma, float k) {
    if constexpr (A == 1) return logp_gauss(s[0], as_f32(word), sigma, k);
    else return logp_discrete<A>(s, word);
}

// environment i of one [D][n] observation row and its action word
template <int D, int A, int ACT, class Net>
MG_HD float logp_of(const Net& net, const float* row, uint64_t n, uint64_t i, uint32_t word, float sigma, float k) {
    float o[1][D], s[1][A];
#pragma unroll
    for (int q = 0; q < D; ++q) o[0][q] = row[(uint64_t)q * n + i];
    mlp_scores<D, A, ACT, 1>(net, o, s);
    return logp_head<A>(s[0], word, sigma, k);
}

// environment i, every word the call writes for it (the one-environment-per-lane form and the host check)
template <int D, int A, int ACT, class Net>
MG_HD void logprob_env(const Net& net, int32_t K, uint64_t n, uint64_t i, const float* obs_first, const float* obs, const uint32_t* actions, float sigma, float k,
                       float* logp_out) {
    for (int32_t t = 0; t < K; ++t)
        logp_out[(uint64_t)t * n + i] = logp_of<D, A, ACT>(net, value_row_in(t, n, D, obs_first, obs), n, i, actions[(uint64_t)t * n + i], sigma, k);
}

#if defined(__HIPCC__)
// logprob.hip: the launch of mgym_logprob_mlp on `stream`, arguments already checked (abi.hip); n > 0, K >= 1.  `policy`: the caller's host words; hidden2 == 0:
// they travel by value as an MlpPack<D, A>, else `pack_dev` (the handle's third weight pack) holds them by then (Env::mlp2_store_to)
struct LogpCall {
    uint64_t n;
    int32_t K;
    float sigma, k;
    const float *obs_first, *obs;
    const uint32_t* actions;
    float* logp_out;
    // what learner.h's dense kernel asks of a call: steps 0 .. K - 1, the step's action row, the family's head
    static constexpr bool kActions = true;
    __device__ __forceinline__ int32_t rows() const { return K; }
    __device__ __forceinline__ float* out_row(int32_t r) const { return logp_out + (uint64_t)r * n; }
    __device__ __forceinline__ const uint32_t* action_row(int32_t r) const { return actions + (uint64_t)r * n; }
    template <int A> __device__ __forceinline__ float word(const float (&s)[A], uint32_t w) const { return logp_head<A>(s, w, sigma, k); }
};
int logprob_launch(hipStream_t stream, const LogpCall& call, int D, int A, const float* policy, int32_t hidden1, int32_t hidden2, int32_t activation, const float* pack_dev);
#endif

}  // namespace mgym
