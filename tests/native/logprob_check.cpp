// CPU check of mgym_logprob_mlp's words (modurl_gym_amd/csrc/logprob.h over mlp_policy.h, mlp2_policy.h and value.h: the lines the kernels of logprob.hip
// compile), built as a shared object with g++ -ffp-contract=off for tests/logprob_ref.py.
//   logprob_eval(D, A, depth, act, H1, H2, policy, sigma, K, n, obs_first, obs, actions, logp_out)
//     depth 1 (policy: W1[H1][D], b1, W2[A][H1], b2; H2 is ignored) or 2 (W1[H1][D], b1, W2[H2][H1], b2, W3[A][H2], b3; no MLP_ACT_TANH): logprob_env over
//     every environment; A == 1 is the Gaussian head with k = logp_gauss_k(sigma), else the categorical head and sigma is not read.
//     -> 0; 1 for a combination the entry point refuses; 2 where, with n a multiple of 4, the rows taken four to a lane (mlp_scores<D, A, ACT, 4> and the
//        head, the form of learner.h's dense4_kernel) differ from logprob_env's
//   logprob_k(sigma) -> logp_gauss_k;  logprob_sigma_ok(sigma) -> logp_sigma_ok
//   log_pos_eval(n, x, out): out[i] = mg_log_pos(x[i])
//   log_pos_sweep(first, last, &max_abs, &max_rel, &differ): over every f32 bit pattern first .. last (positive normal floats), against libm's float64 log of
//     the same value: the largest |mg_log_pos - log|, the largest |mg_log_pos - log| / |log| (where log != 0) and the number of patterns whose roundings to
//     f32 differ
//   log_pos_stats(n, x, &max_abs, &max_rel, &differ): the same over the n given floats
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../modurl_gym_amd/csrc/logprob.h"

using namespace mgym;

struct Case {
    int32_t K;
    uint64_t n;
    float sigma, k;
    const float *obs_first, *obs;
    const uint32_t* actions;
    float* logp_out;
};

template <int D, int A, int ACT, class Net>
static int eval(const Net& net, const Case& c) {
    for (uint64_t i = 0; i < c.n; ++i) logprob_env<D, A, ACT>(net, c.K, c.n, i, c.obs_first, c.obs, c.actions, c.sigma, c.k, c.logp_out);
    if (c.n % 4) return 0;
    for (int32_t t = 0; t < c.K; ++t) {
        const float* in = value_row_in(t, c.n, D, c.obs_first, c.obs);
        for (uint64_t l = 0; l < c.n / 4; ++l) {
            float o[4][D], s[4][A];
            for (int e = 0; e < 4; ++e)
                for (int q = 0; q < D; ++q) o[e][q] = in[(uint64_t)q * c.n + 4 * l + e];
            mlp_scores<D, A, ACT, 4>(net, o, s);
            for (int e = 0; e < 4; ++e) {
                const uint64_t at = (uint64_t)t * c.n + 4 * l + e;
                const float four = logp_head<A>(s[e], c.actions[at], c.sigma, c.k), one = c.logp_out[at];
                if (as_u32(four) != as_u32(one) && !(four != four && one != one)) return 2;
            }
        }
    }
    return 0;
}

template <int D, int A>
static int eval_family(int depth, int act, int H1, int H2, const float* policy, const Case& c) {
    if (depth == 1) {
        MlpPack<D, A> pack;
        mlp_pack<D, A>(policy, H1, pack);
        if (act == MLP_ACT_RELU) return eval<D, A, MLP_ACT_RELU>(pack, c);
        if (act == MLP_ACT_TANH) return eval<D, A, MLP_ACT_TANH>(pack, c);
        if (act == MLP_ACT_TANH_FAST) return eval<D, A, MLP_ACT_TANH_FAST>(pack, c);
        return 1;
    }
    std::vector<float> pack(mlp2_pack_floats(D, H1, H2));
    mlp2_pack(policy, D, A, H1, H2, pack.data());
    const Mlp2Net<D, A> net{pack.data(), H1, H2, c.sigma};
    if (act == MLP_ACT_RELU) return eval<D, A, MLP_ACT_RELU>(net, c);
    if (act == MLP_ACT_TANH_FAST) return eval<D, A, MLP_ACT_TANH_FAST>(net, c);
    return 1;
}

static void fold(float x, double* max_abs, double* max_rel, uint64_t* differ) {
    const double got = mg_log_pos(x), ref = log((double)x);
    const double err = fabs(got - ref);
    if (err > *max_abs) *max_abs = err;
    if (ref != 0.0 && err / fabs(ref) > *max_rel) *max_rel = err / fabs(ref);
    if (as_u32((float)got) != as_u32((float)ref)) ++*differ;
}

extern "C" {

int logprob_eval(int D, int A, int depth, int act, int H1, int H2, const float* policy, float sigma, int32_t K, uint64_t n, const float* obs_first, const float* obs,
                 const uint32_t* actions, float* logp_out) {
    if (H1 < 1 || H1 > kMlpMaxHidden || (depth == 2 && (H2 < 1 || H2 > kMlpMaxHidden)) || (depth != 1 && depth != 2) || K < 1) return 1;
    if (A == 1 && !logp_sigma_ok(sigma)) return 1;
    const Case c{K, n, sigma, A == 1 ? logp_gauss_k(sigma) : 0.0f, obs_first, obs, actions, logp_out};
    switch (D * 10 + A) {
    case 42: return eval_family<4, 2>(depth, act, H1, H2, policy, c);
    case 23: return eval_family<2, 3>(depth, act, H1, H2, policy, c);
    case 21: return eval_family<2, 1>(depth, act, H1, H2, policy, c);
    case 31: return eval_family<3, 1>(depth, act, H1, H2, policy, c);
    case 63: return eval_family<6, 3>(depth, act, H1, H2, policy, c);
    case 84: return eval_family<8, 4>(depth, act, H1, H2, policy, c);
    }
    return 1;
}

float logprob_k(float sigma) { return logp_gauss_k(sigma); }
int logprob_sigma_ok(float sigma) { return logp_sigma_ok(sigma) ? 1 : 0; }

void log_pos_eval(uint64_t n, const float* x, double* out) {
    for (uint64_t i = 0; i < n; ++i) out[i] = mg_log_pos(x[i]);
}

void log_pos_sweep(uint32_t first, uint32_t last, double* max_abs, double* max_rel, uint64_t* differ) {
    *max_abs = *max_rel = 0.0;
    *differ = 0;
    for (uint64_t b = first; b <= last; ++b) fold(as_f32((uint32_t)b), max_abs, max_rel, differ);
}

void log_pos_stats(uint64_t n, const float* x, double* max_abs, double* max_rel, uint64_t* differ) {
    *max_abs = *max_rel = 0.0;
    *differ = 0;
    for (uint64_t i = 0; i < n; ++i) fold(x[i], max_abs, max_rel, differ);
}

}
