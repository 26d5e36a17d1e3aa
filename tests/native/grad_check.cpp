// CPU check of the words of mgym_ppo_grad_mlp / mgym_value_grad_mlp (modurl_gym_amd/csrc/grad.h over logprob.h and mlp_policy.h: the lines the kernels of
// grad.hip compile) and of mgym_ppo_grad_mlp2 / mgym_value_grad_mlp2 (grad2.h over grad.h and mlp2_policy.h), built as a shared object with g++
// -ffp-contract=off for tests/grad_ref.py.  head: 0 categorical, 1 Gaussian, 2 value (A = 1, x0 = ret, actions and x1 unread).  lo = 1.0f - clip and
// hi = 1.0f + clip are computed here as the entry point computes them.
//   grad_words(D, A, act, head, H, weights, sigma, clip, ent_coef, K, n, obs_first, obs, actions, x0, x1, words)
//     per env-step at = t * n + i, 2 A + 3 + 5 floats: ds[A], g, r, Hent, p[A], then the five statistics' terms (loss, entropy, kl, clipped, ratio)
//   grad2_words(D, A, act, head, H1, H2, weights, ...)
//     per env-step, A + 1 + 5 + H2 + 2 H1 + A floats: ds[A], the log-sigma term, the five statistics' terms, dpre2[H2], dh1[H1], dpre1[H1], s[A]
//   grad_full / grad2_full(..., first, count, grad_out[P + 1], stats_out[8]): the call over environments first .. first + count - 1: grad_envs' / grad2_envs'
//     f64 sums, grad_result's words
//   -> 0; 1 for a combination the entry points refuse
#include <stdint.h>
#include <vector>
#include "../../modurl_gym_amd/csrc/grad2.h"

using namespace mgym;

struct Case {
    int H1, H2;   // H2 = 0: one hidden layer
    const float* weights;
    float sigma, clip, ent_coef;
    int32_t K;
    uint64_t n, first, count;
    const float *obs_first, *obs;
    const uint32_t* actions;
    const float *x0, *x1;
    float *words, *grad_out, *stats_out;
};

// the words of one env-step, o its observation: the one-layer heads' ...
template <int D, int A, int ACT, class Head>
static void step_words(const Case& c, const MlpPack<D, A>& net, const Head& head, const float (&o)[1][D], uint64_t at) {
    float s[1][A];
    mlp_scores<D, A, ACT, 1>(net, o, s);
    GradStep<A> g;
    head.step(s[0], c.actions ? c.actions[at] : 0u, c.x0[at], c.x1 ? c.x1[at] : 0.0f, g);
    float* w = c.words + at * (2 * A + 3 + kGradStats);
    for (int a = 0; a < A; ++a) { w[a] = g.ds[a]; w[A + 3 + a] = g.p[a]; }
    w[A] = g.g; w[A + 1] = g.r; w[A + 2] = g.hent;
    for (int k = 0; k < kGradStats; ++k) w[2 * A + 3 + k] = g.stat[k];
}

// ... and the two-layer env-step's
template <int D, int A, int ACT, class Head>
static void step_words(const Case& c, const std::vector<float>& pack, const Head& head, const float (&o)[1][D], uint64_t at) {
    Grad2Words<A> w;
    grad2_step<D, A, ACT>(pack.data(), c.H1, c.H2, head, o[0], c.actions ? c.actions[at] : 0u, c.x0[at], c.x1 ? c.x1[at] : 0.0f, w);
    float* out = c.words + at * (2 * A + 1 + kGradStats + c.H2 + 2 * c.H1);
    for (int a = 0; a < A; ++a) *out++ = w.g.ds[a];
    *out++ = w.g.dls;
    for (int k = 0; k < kGradStats; ++k) *out++ = w.g.stat[k];
    for (int k = 0; k < c.H2; ++k) *out++ = w.dpre2[k];
    for (int j = 0; j < c.H1; ++j) *out++ = w.dh1[j];
    for (int j = 0; j < c.H1; ++j) *out++ = w.dpre1[j];
    for (int a = 0; a < A; ++a) *out++ = w.s[a];
}

// the f64 sums of the range, by each depth's host form of the call
template <int D, int A, int ACT, class Head>
static void envs(const Case& c, const MlpPack<D, A>& net, const Head& head, double* sums) {
    grad_envs<D, A, ACT>(net, head, c.K, c.n, c.first, c.count, c.obs_first, c.obs, c.actions, c.x0, c.x1, sums);
}

template <int D, int A, int ACT, class Head>
static void envs(const Case& c, const std::vector<float>& pack, const Head& head, double* sums) {
    grad2_envs<D, A, ACT>(pack.data(), c.H1, c.H2, head, c.K, c.n, c.first, c.count, c.obs_first, c.obs, c.actions, c.x0, c.x1, sums);
}

// net: the packed weights of either depth, P their count
template <int D, int A, int ACT, class Head, class Net>
static int run_net(const Case& c, const Net& net, int P, const Head& head, bool gauss) {
    if (c.words) {
        for (int32_t t = 0; t < c.K; ++t)
            for (uint64_t i = 0; i < c.n; ++i) {
                const float* row = value_row_in(t, c.n, D, c.obs_first, c.obs);
                float o[1][D];
                for (int q = 0; q < D; ++q) o[0][q] = row[(uint64_t)q * c.n + i];
                step_words<D, A, ACT>(c, net, head, o, (uint64_t)t * c.n + i);
            }
        return 0;
    }
    std::vector<double> sums(P + kGradTail, 0.0);
    envs<D, A, ACT>(c, net, head, sums.data());
    const double B = (double)c.K * (double)c.count;
    for (int out = 0; out <= P + kGradTail; ++out) {
        const float r = grad_result(out <= P + kGradStats ? sums[out] : 0.0, P, out, B, c.ent_coef, gauss);
        if (out <= P) c.grad_out[out] = r;
        else c.stats_out[out - (P + 1)] = r;
    }
    return 0;
}

template <int D, int A, int ACT, class Head>
static int run(const Case& c, const Head& head, bool gauss) {
    if (c.H2 == 0) {
        MlpPack<D, A> net;
        mlp_pack<D, A>(c.weights, c.H1, net);
        return run_net<D, A, ACT>(c, net, mlp_policy_floats(D, A, c.H1), head, gauss);
    }
    std::vector<float> pack(mlp2_pack_floats(D, c.H1, c.H2));
    mlp2_pack(c.weights, D, A, c.H1, c.H2, pack.data());
    return run_net<D, A, ACT>(c, pack, mlp2_policy_floats(D, A, c.H1, c.H2), head, gauss);
}

template <int D, int A, int ACT>
static int run_head(int head, const Case& c) {
    const PpoTerms terms{1.0f - c.clip, 1.0f + c.clip, c.ent_coef};
    if (head == 2) {
        if constexpr (A == 1) return run<D, 1, ACT>(c, ValueMse{}, false);
        else return 1;
    }
    if constexpr (A == 1) {
        if (head != 1 || !logp_sigma_ok(c.sigma)) return 1;
        return run<D, 1, ACT>(c, PpoGaussian{terms, c.sigma, logp_gauss_k(c.sigma), grad_gauss_entropy(c.sigma)}, true);
    } else {
        if (head != 0) return 1;
        return run<D, A, ACT>(c, PpoCategorical<A>{terms}, false);
    }
}

template <int D, int A>
static int run_act(int act, int head, const Case& c, bool exact_tanh) {
    if (act == MLP_ACT_RELU) return run_head<D, A, MLP_ACT_RELU>(head, c);
    if (act == MLP_ACT_TANH && exact_tanh) return run_head<D, A, MLP_ACT_TANH>(head, c);
    if (act == MLP_ACT_TANH_FAST) return run_head<D, A, MLP_ACT_TANH_FAST>(head, c);
    return 1;
}

static int dispatch(int D, int A, int act, int head, const Case& c, bool two) {
    if (c.H1 < 1 || c.H1 > kMlpMaxHidden || c.H2 < (two ? 1 : 0) || c.H2 > (two ? kMlpMaxHidden : 0) || c.K < 1) return 1;
    if (head != 2 && (!grad_clip_ok(c.clip) || !grad_ent_coef_ok(c.ent_coef))) return 1;
    const bool exact_tanh = !two;   // (no exact tanh with two hidden layers)
    switch (D * 10 + A) {
    case 42: return run_act<4, 2>(act, head, c, exact_tanh);
    case 23: return run_act<2, 3>(act, head, c, exact_tanh);
    case 21: return run_act<2, 1>(act, head, c, exact_tanh);
    case 31: return run_act<3, 1>(act, head, c, exact_tanh);
    case 63: return run_act<6, 3>(act, head, c, exact_tanh);
    case 84: return run_act<8, 4>(act, head, c, exact_tanh);
    case 41: return run_act<4, 1>(act, head, c, exact_tanh);   // the critics of the discrete families
    case 61: return run_act<6, 1>(act, head, c, exact_tanh);
    case 81: return run_act<8, 1>(act, head, c, exact_tanh);
    }
    return 1;
}

extern "C" {

int grad2_words(int D, int A, int act, int head, int H1, int H2, const float* weights, float sigma, float clip, float ent_coef, int32_t K, uint64_t n,
                const float* obs_first, const float* obs, const uint32_t* actions, const float* x0, const float* x1, float* words) {
    return dispatch(D, A, act, head, Case{H1, H2, weights, sigma, clip, ent_coef, K, n, 0, n, obs_first, obs, actions, x0, x1, words, nullptr, nullptr}, true);
}

int grad2_full(int D, int A, int act, int head, int H1, int H2, const float* weights, float sigma, float clip, float ent_coef, int32_t K, uint64_t n, uint64_t first,
               uint64_t count, const float* obs_first, const float* obs, const uint32_t* actions, const float* x0, const float* x1, float* grad_out, float* stats_out) {
    if (count == 0 || first > n || count > n - first) return 1;
    return dispatch(D, A, act, head, Case{H1, H2, weights, sigma, clip, ent_coef, K, n, first, count, obs_first, obs, actions, x0, x1, nullptr, grad_out, stats_out}, true);
}

int grad_words(int D, int A, int act, int head, int H, const float* weights, float sigma, float clip, float ent_coef, int32_t K, uint64_t n, const float* obs_first,
               const float* obs, const uint32_t* actions, const float* x0, const float* x1, float* words) {
    return dispatch(D, A, act, head, Case{H, 0, weights, sigma, clip, ent_coef, K, n, 0, n, obs_first, obs, actions, x0, x1, words, nullptr, nullptr}, false);
}

int grad_full(int D, int A, int act, int head, int H, const float* weights, float sigma, float clip, float ent_coef, int32_t K, uint64_t n, uint64_t first,
              uint64_t count, const float* obs_first, const float* obs, const uint32_t* actions, const float* x0, const float* x1, float* grad_out, float* stats_out) {
    if (count == 0 || first > n || count > n - first) return 1;
    return dispatch(D, A, act, head, Case{H, 0, weights, sigma, clip, ent_coef, K, n, first, count, obs_first, obs, actions, x0, x1, nullptr, grad_out, stats_out}, false);
}

int grad_slab_bytes_of(int D, int A, int H) { return (int)grad_slab_bytes(D, A, H); }
int grad2_slab_bytes_of(int D, int A, int H1, int H2) { return (int)grad2_slab_bytes(D, A, H1, H2); }
int grad2_slab_cap(void) { return kGrad2SlabCap; }
int grad_clip_ok_of(float clip) { return grad_clip_ok(clip) ? 1 : 0; }
int grad_ent_coef_ok_of(float x) { return grad_ent_coef_ok(x) ? 1 : 0; }

}
