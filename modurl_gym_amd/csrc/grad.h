// grad.h — the words of mgym_ppo_grad_mlp and mgym_value_grad_mlp (include/mgym.h): per env-step, the derivative of the loss with respect to the scores (ds),
// the statistics' terms, and one hidden unit's share of the backward pass.  Shared by the kernels of grad.hip (four environments per lane, or one) and the host
// check tests/native/grad_check.cpp, which compiles this header with g++.  Compile with -ffp-contract=off: the only fused operations are the cp_fmaf of the chains and of the lane's sums.
//
//   scores   s_a of mlp_scores<D, A, ACT, N> under the one-hidden-layer net (mlp_policy.h's MlpPack<D, A>) on the row value.h's value_row_in gives step t
//   PPO      logp_new = logp_head<A> of logprob.h;  d = logp_new - logp_old;  r = mg_expm1f(d) + 1.0f
//            clipped = (adv > 0 && r > hi) || (adv < 0 && r < lo);  g = clipped ? +0 : (-adv) * r
//            rc = r < lo ? lo : (r > hi ? hi : r);  u = r * adv;  uc = rc * adv;  loss = -(uc < u ? uc : u);  kl = (r - 1.0f) - d
//   categorical (A >= 2)   m, e_a, c_{A-1} of mlp_sample_cum;  lse = (float)mg_log_pos(c_{A-1});  p_a = e_a / c_{A-1};  lp_a = (s_a - m) - lse
//            t = p_0 * lp_0;  a = 1 .. A-1: t = t + p_a * lp_a;  Hent = -t;  ds_a = g * ((a == act ? 1.0f : 0.0f) - p_a) + (ent_coef * p_a) * (lp_a + Hent)
//   Gaussian (A == 1)      z = (a - s_0) / sigma;  ds_0 = (g * z) / sigma;  the log-sigma term g * (z * z - 1.0f);  the entropy the host's constant
//   value    e = s_0 - ret;  ds_0 = e;  loss = 0.5f * (e * e)
//   unit j   pre_j, h_j of mlp_policy.h;  dh = W2[0][j] * ds_0;  a = 1 .. A-1: dh = dh + W2[a][j] * ds_a;  dpre = dh * act',  act' = pre_j > 0 ? 1.0f : 0.0f
//            (ReLU) or 1.0f - h_j * h_j (both tanh forms);  the terms dW1[j][q] += dpre * o_q, db1[j] += dpre, dW2[a][j] += ds_a * h_j, and db2[a] += ds_a
// f32 throughout, nothing reassociated, every selection a selection.  The SUMS over env-steps are not word-defined: the kernels add a lane's terms with fmaf
// in f32, a wave's in f32, and everything beyond in f64; the host check adds in f64.
//
// Two hidden layers are grad2.h and grad2.hip (dW2[H2][H1] is a tiled product over the batch).  Out of scope, here and in include/mgym.h: the optimizer step,
// advantage normalisation, flat-index minibatches, a clipped value loss, any state of the handle.
#pragma once
#include <stdint.h>
#include "logprob.h"

namespace mgym {

// MG_HD for a member function (MG_HD is `static inline` under g++)
#if defined(__HIPCC__)
#define MG_HDM __host__ __device__ __forceinline__
#else
#define MG_HDM inline
#endif

// statistics' terms of one env-step, in the order of the slab: loss, entropy, kl, clipped, ratio
enum { GRAD_LOSS = 0, GRAD_ENT = 1, GRAD_KL = 2, GRAD_CLIPPED = 3, GRAD_RATIO = 4, kGradStats = 5 };
constexpr int kGradTail = 8;       // words of a slab after the P gradient sums: the log-sigma sum, the five statistics' sums, two spare
constexpr int kGradSlabCap = 1024; // slabs a launch uses at most: four blocks on each of the chip's 256 compute units

// words of one slab (f64 each) and the calls' workspace sizes
MG_HD int grad_slab_words(int D, int A, int H) { return mlp_policy_floats(D, A, H) + kGradTail; }
MG_HD uint64_t grad_slab_bytes(int D, int A, int H) { return (uint64_t)grad_slab_words(D, A, H) * 8u; }

template <int A>
struct GradStep {
    float ds[A];             // dL_i / ds_a
    float dls;               // the log-sigma term (Gaussian head), else +0
    float stat[kGradStats];
    float g, r, hent, p[A];  // named words the host check reads; the kernels drop them
};

struct PpoTerms { float lo, hi, ent_coef; };

// the ratio, the clip and the statistics' terms -> g
template <int A>
MG_HD float ppo_ratio(const PpoTerms& c, float logp_new, float logp_old, float adv, GradStep<A>& o) {
    const float d = logp_new - logp_old;
    const float r = mg_expm1f(d) + 1.0f;
    const bool clipped = (adv > 0.0f && r > c.hi) || (adv < 0.0f && r < c.lo);
    const float g = clipped ? 0.0f : (-adv) * r;
    const float rc = r < c.lo ? c.lo : (r > c.hi ? c.hi : r);
    const float u = r * adv, uc = rc * adv;
    o.stat[GRAD_LOSS] = -(uc < u ? uc : u);
    o.stat[GRAD_KL] = (r - 1.0f) - d;
    o.stat[GRAD_CLIPPED] = clipped ? 1.0f : 0.0f;
    o.stat[GRAD_RATIO] = r;
    o.g = g;
    o.r = r;
    return g;
}

// ---- the three heads: step(scores, action word, x0, x1, out); x0 / x1 are logp_old / adv, or ret / nothing ----
template <int A>
struct PpoCategorical {
    static_assert(A >= 2, "a categorical distribution needs two actions");
    static constexpr bool kPpo = true;
    PpoTerms c;
    MG_HDM void step(const float (&s)[A], uint32_t act, float logp_old, float adv, GradStep<A>& o) const {
        // m, b and the weights e_a as mlp_sample_cum computes them (A - 1 evaluations of mg_expm1f), c_{A-1} as it adds them
        float m = s[0];
        int b = 0;
#pragma unroll
        for (int a = 1; a < A; ++a)
            if (s[a] > m) { m = s[a]; b = a; }
        float ex[A - 1];
#pragma unroll
        for (int k = 0; k < A - 1; ++k) ex[k] = mg_expm1f((k >= b ? s[k + 1] : s[k]) - m) + 1.0f;
        const float eb = (m - m) + 1.0f;
        float e[A], sum = 0.0f;
#pragma unroll
        for (int a = 0; a < A; ++a) {
            const float lo = ex[a > 0 ? a - 1 : 0], hi = ex[a < A - 1 ? a : A - 2];
            e[a] = a == b ? eb : (a > b ? lo : hi);
            sum = a == 0 ? e[a] : sum + e[a];
        }
        const float lse = (float)mg_log_pos(sum);
        const float g = ppo_ratio<A>(c, logp_head<A>(s, act, 0.0f, 0.0f), logp_old, adv, o);
        float lp[A], t = 0.0f;
#pragma unroll
        for (int a = 0; a < A; ++a) {
            o.p[a] = e[a] / sum;
            lp[a] = (s[a] - m) - lse;
            t = a == 0 ? o.p[a] * lp[a] : t + o.p[a] * lp[a];
        }
        const float hent = -t;
#pragma unroll
        for (int a = 0; a < A; ++a) o.ds[a] = g * ((act == (uint32_t)a ? 1.0f : 0.0f) - o.p[a]) + (c.ent_coef * o.p[a]) * (lp[a] + hent);
        o.dls = 0.0f;
        o.stat[GRAD_ENT] = hent;
        o.hent = hent;
    }
};

struct PpoGaussian {
    static constexpr bool kPpo = true;
    PpoTerms c;
    float sigma, k, ent;   // k = logp_gauss_k(sigma), ent = grad_gauss_entropy(sigma), once on the host
    MG_HDM void step(const float (&s)[1], uint32_t word, float logp_old, float adv, GradStep<1>& o) const {
        const float g = ppo_ratio<1>(c, logp_head<1>(s, word, sigma, k), logp_old, adv, o);
        const float z = (as_f32(word) - s[0]) / sigma;
        o.ds[0] = (g * z) / sigma;
        o.dls = g * (z * z - 1.0f);
        o.stat[GRAD_ENT] = ent;
        o.hent = ent;
        o.p[0] = 1.0f;
    }
};
MG_HD float grad_gauss_entropy(float sigma) { return (float)(mg_log_pos(sigma) + 1.4189385332046727); }

struct ValueMse {
    static constexpr bool kPpo = false;
    MG_HDM void step(const float (&s)[1], uint32_t, float ret, float, GradStep<1>& o) const {
        const float e = s[0] - ret;
        o.ds[0] = e;
        o.dls = 0.0f;
        o.stat[GRAD_LOSS] = 0.5f * (e * e);
        o.stat[GRAD_ENT] = o.stat[GRAD_KL] = o.stat[GRAD_CLIPPED] = o.stat[GRAD_RATIO] = 0.0f;
        o.g = o.r = o.hent = 0.0f;
        o.p[0] = 1.0f;
    }
};

// the clip and the entropy coefficient the actor's call accepts
MG_HD bool grad_clip_ok(float clip) { return clip >= 0.0f && clip < 1.0f; }                                       // (a NaN fails the first test)
MG_HD bool grad_ent_coef_ok(float x) { return x >= -3.402823466e+38f && x <= 3.402823466e+38f; }

// act' of a unit from its pre-activation and its activation: the one rule of the backward words at both depths
template <int ACT>
MG_HD float grad_dact(float pre, float h) { return ACT == MLP_ACT_RELU ? (pre > 0.0f ? 1.0f : 0.0f) : 1.0f - h * h; }

// hidden unit j of one env-step, u = W1[j][0 .. D-1], b1[j], W2[0 .. A-1][j]: h_j (recomputed: the chain and the activation of mlp_hidden) and dpre_j
template <int D, int A, int ACT>
MG_HD void grad_unit(const float* u, const float (&o)[D], const float (&ds)[A], float* h_out, float* dpre_out) {
    float pre = u[D];
#pragma unroll
    for (int q = 0; q < D; ++q) pre = cp_fmaf(u[q], o[q], pre);
    const float h = mlp_activate<ACT>(pre);
    float dh = u[D + 1] * ds[0];
#pragma unroll
    for (int a = 1; a < A; ++a) dh = dh + u[D + 1 + a] * ds[a];
    *h_out = h;
    *dpre_out = dh * grad_dact<ACT>(pre, h);
}

// where the sums of a slab stand, the caller's nn.Linear order: dW1[H][D], db1[H], dW2[A][H], db2[A], then the tail
MG_HD int grad_at_w1(int D, int j, int q) { return j * D + q; }
MG_HD int grad_at_b1(int D, int H, int j) { return H * D + j; }
MG_HD int grad_at_w2(int D, int H, int a, int j) { return H * D + H + a * H + j; }
MG_HD int grad_at_b2(int D, int A, int H, int a) { return H * D + H + A * H + a; }

// the word the calls return at `out` = 0 .. P + 8 (grad_out[0 .. P], then stats_out[0 .. 7]) from `sum`, the f64 sum over the B env-steps that stands at
// `out` in the slab (out <= P + kGradStats; unread beyond): divided by B once, the log-sigma word less ent_coef (B times ent_coef before the division)
MG_HD float grad_result(double sum, int P, int out, double B, float ent_coef, bool gauss) {
    if (out < P) return (float)(sum / B);
    if (out == P) return gauss ? (float)((sum - (double)ent_coef * B) / B) : 0.0f;
    const int k = out - (P + 1);
    if (k < kGradStats) return (float)(sum / B);
    return k == 5 ? (float)B : 0.0f;
}

// every env-step of environments first .. first + count - 1 added into sums[P + kGradTail] in f64, steps ascending inside environments ascending: the host
// check's form of the call (the kernels add in another order).  x0 / x1: logp_old / adv, or ret / null
template <int D, int A, int ACT, class Head>
MG_HD void grad_envs(const MlpPack<D, A>& net, const Head& head, int32_t K, uint64_t n, uint64_t first, uint64_t count, const float* obs_first, const float* obs,
                     const uint32_t* actions, const float* x0, const float* x1, double* sums) {
    const int H = net.hidden, P = mlp_policy_floats(D, A, H);
    for (uint64_t i = first; i < first + count; ++i)
        for (int32_t t = 0; t < K; ++t) {
            const float* row = value_row_in(t, n, D, obs_first, obs);
            const uint64_t at = (uint64_t)t * n + i;
            float o[1][D], s[1][A];
            for (int q = 0; q < D; ++q) o[0][q] = row[(uint64_t)q * n + i];
            mlp_scores<D, A, ACT, 1>(net, o, s);
            GradStep<A> g;
            head.step(s[0], actions ? actions[at] : 0u, x0[at], x1 ? x1[at] : 0.0f, g);
            for (int j = 0; j < H; ++j) {
                float h, dpre;
                grad_unit<D, A, ACT>(net.unit[j], o[0], g.ds, &h, &dpre);
                for (int q = 0; q < D; ++q) sums[grad_at_w1(D, j, q)] += (double)(dpre * o[0][q]);
                sums[grad_at_b1(D, H, j)] += (double)dpre;
                for (int a = 0; a < A; ++a) sums[grad_at_w2(D, H, a, j)] += (double)(g.ds[a] * h);
            }
            for (int a = 0; a < A; ++a) sums[grad_at_b2(D, A, H, a)] += (double)g.ds[a];
            sums[P] += (double)g.dls;
            for (int k = 0; k < kGradStats; ++k) sums[P + 1 + k] += (double)g.stat[k];
        }
}

#if defined(__HIPCC__)
// grad.hip: the two launches of a gradient call on `stream`, arguments already checked (abi.hip); n > 0, K >= 1, env_count >= 1, slabs >= 1.  x0 / x1 are
// logp_old / adv (the actor) or ret / null (the critic: actions is null too, A = 1, and the head is the value head)
struct GradCall {
    uint64_t n, env_first, env_count;
    int32_t K, slabs;
    float lo, hi, ent_coef, sigma, k, ent;
    const float *obs_first, *obs;
    const uint32_t* actions;
    const float *x0, *x1;
    double* workspace;
    float *grad_out, *stats_out;
};
enum { GRAD_HEAD_CATEGORICAL = 0, GRAD_HEAD_GAUSS = 1, GRAD_HEAD_VALUE = 2 };
int grad_launch(hipStream_t stream, const GradCall& call, int D, int A, int head, const float* weights, int32_t hidden, int32_t activation);
// grad.hip: the last sum of a gradient call of either depth, grad_finish_kernel over `slabs` slabs of P + kGradTail words
void grad_finish_launch(hipStream_t stream, const GradCall& call, int slabs, int P, bool gauss);
#endif

}  // namespace mgym
