// grad2.h — the words of mgym_ppo_grad_mlp2 and mgym_value_grad_mlp2 (include/mgym.h): the gradient calls of grad.h for the two-hidden-layer net of
// mgym_rollout_mlp2.  The heads (ds, the log-sigma term, the statistics' terms) are grad.h's, unchanged, applied to the scores of mlp2_policy.h; this header
// adds the backward words of the two hidden layers and the host form of the whole call.  Shared by the kernels of grad2.hip and the host check
// tests/native/grad_check.cpp, which compiles it with g++.  Compile with -ffp-contract=off: the only fused operations are the cp_fmaf of the chains.
//
//   pre1_j, h1_j, pre2_k, h2_k, s_a     mlp2_policy.h's three chains, unpadded
//   ds_a, the log-sigma term, the statistics' terms     grad.h's heads on these s_a
//   dh2_k   = W3[0][k] * ds_0;  a = 1 .. A-1: dh2_k = dh2_k + W3[a][k] * ds_a
//   dpre2_k = dh2_k * act'(k)           act' = pre2_k > 0 ? 1.0f : 0.0f (ReLU), 1.0f - h2_k * h2_k (tanh_fast): grad.h's grad_dact
//   dh1_j   = +0.0f;  k = 0 .. H2-1 ascending: dh1_j = fmaf(W2[k][j], dpre2_k, dh1_j)
//   dpre1_j = dh1_j * act'(j)           the same rule on pre1_j / h1_j (under ReLU h1_j > 0 exactly when pre1_j > 0: mlp_activate)
//   terms   dW3[a][k] += ds_a * h2_k;  db3[a] += ds_a;  dW2[k][j] += dpre2_k * h1_j;  db2[k] += dpre2_k;  dW1[j][q] += dpre1_j * o_q;  db1[j] += dpre1_j
// f32 throughout, nothing reassociated, every selection a selection.  The SUMS over env-steps and the products inside them are not word-defined: the kernels
// form them on the f32 matrix pipe over at most 128 env-steps of a wave and add everything beyond in f64; the host check adds in f64.
#pragma once
#include <stdint.h>
#include "grad.h"

namespace mgym {

// slabs a launch uses at most: the kernel's block holds 120 - 160 KB of LDS, so one block is resident on each of the chip's 256 compute units and more slabs
// than that would only add work to the last sum
constexpr int kGrad2SlabCap = 256;

MG_HD int grad2_slab_words(int D, int A, int H1, int H2) { return mlp2_policy_floats(D, A, H1, H2) + kGradTail; }
MG_HD uint64_t grad2_slab_bytes(int D, int A, int H1, int H2) { return (uint64_t)grad2_slab_words(D, A, H1, H2) * 8u; }

// where the sums of a slab stand, the caller's nn.Linear order: dW1[H1][D], db1[H1], dW2[H2][H1], db2[H2], dW3[A][H2], db3[A], then the tail
MG_HD int grad2_at_w1(int D, int j, int q) { return j * D + q; }
MG_HD int grad2_at_b1(int D, int H1, int j) { return H1 * D + j; }
MG_HD int grad2_at_w2(int D, int H1, int k, int j) { return H1 * (D + 1) + k * H1 + j; }
MG_HD int grad2_at_b2(int D, int H1, int H2, int k) { return H1 * (D + 1) + H2 * H1 + k; }
MG_HD int grad2_at_w3(int D, int H1, int H2, int a, int k) { return H1 * (D + 1) + H2 * (H1 + 1) + a * H2 + k; }
MG_HD int grad2_at_b3(int D, int A, int H1, int H2, int a) { return H1 * (D + 1) + H2 * (H1 + 1) + A * H2 + a; }

// dh2_k of one env-step; u = unit k's run of the pack: b2[k], W3[0 .. A-1][k]
template <int A>
MG_HD float grad2_dh2(Mlp2Ptr u, const float (&ds)[A]) {
    float dh = u[1] * ds[0];
#pragma unroll
    for (int a = 1; a < A; ++a) dh = dh + u[1 + a] * ds[a];
    return dh;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// One env-step on the host, every word kept: the forward chains of mlp2_policy.h (the same three lines, the arrays indexed at run time), grad.h's head, and
// the backward words above.  pack: mlp2_pack's words.
template <int A>
struct Grad2Words {
    float pre1[kMlpMaxHidden], h1[kMlpMaxHidden], pre2[kMlpMaxHidden], h2[kMlpMaxHidden], s[A];
    float dpre2[kMlpMaxHidden], dh1[kMlpMaxHidden], dpre1[kMlpMaxHidden];
    GradStep<A> g;
};

template <int D, int A, int ACT, class Head>
static inline void grad2_step(const float* pack, int H1, int H2, const Head& head, const float (&o)[D], uint32_t action, float x0, float x1, Grad2Words<A>& w) {
    const int l2 = mlp2_l2_offset(D, H1), stride = mlp2_l2_stride(H1);
    for (int j = 0; j < H1; ++j) {
        const float* u = pack + kMlp2Head + j * (D + 1);
        float pre = u[D];
        for (int q = 0; q < D; ++q) pre = cp_fmaf(u[q], o[q], pre);
        w.pre1[j] = pre;
        w.h1[j] = mlp_activate<ACT>(pre);
    }
    for (int a = 0; a < A; ++a) w.s[a] = pack[a];
    for (int k = 0; k < H2; ++k) {
        const float* u = pack + l2 + k * stride;
        float pre = u[0];
        for (int j = 0; j < H1; ++j) pre = cp_fmaf(u[kMlp2Head + j], w.h1[j], pre);
        w.pre2[k] = pre;
        w.h2[k] = mlp_activate<ACT>(pre);
        for (int a = 0; a < A; ++a) w.s[a] = cp_fmaf(u[1 + a], w.h2[k], w.s[a]);
    }
    head.step(w.s, action, x0, x1, w.g);
    for (int j = 0; j < H1; ++j) w.dh1[j] = 0.0f;
    for (int k = 0; k < H2; ++k) {
        const float* u = pack + l2 + k * stride;
        w.dpre2[k] = grad2_dh2<A>(u, w.g.ds) * grad_dact<ACT>(w.pre2[k], w.h2[k]);
        for (int j = 0; j < H1; ++j) w.dh1[j] = cp_fmaf(u[kMlp2Head + j], w.dpre2[k], w.dh1[j]);
    }
    for (int j = 0; j < H1; ++j) w.dpre1[j] = w.dh1[j] * grad_dact<ACT>(w.pre1[j], w.h1[j]);
}

// every env-step of environments first .. first + count - 1 added into sums[P2 + kGradTail] in f64, steps ascending inside environments ascending: the host
// check's form of the call, grad_envs' counterpart (the kernels add in another order).  x0 / x1: logp_old / adv, or ret / null
template <int D, int A, int ACT, class Head>
static inline void grad2_envs(const float* pack, int H1, int H2, const Head& head, int32_t K, uint64_t n, uint64_t first, uint64_t count, const float* obs_first,
                              const float* obs, const uint32_t* actions, const float* x0, const float* x1, double* sums) {
    const int P = mlp2_policy_floats(D, A, H1, H2);
    Grad2Words<A> w;
    for (uint64_t i = first; i < first + count; ++i)
        for (int32_t t = 0; t < K; ++t) {
            const float* row = value_row_in(t, n, D, obs_first, obs);
            const uint64_t at = (uint64_t)t * n + i;
            float o[D];
            for (int q = 0; q < D; ++q) o[q] = row[(uint64_t)q * n + i];
            grad2_step<D, A, ACT>(pack, H1, H2, head, o, actions ? actions[at] : 0u, x0[at], x1 ? x1[at] : 0.0f, w);
            for (int j = 0; j < H1; ++j) {
                for (int q = 0; q < D; ++q) sums[grad2_at_w1(D, j, q)] += (double)(w.dpre1[j] * o[q]);
                sums[grad2_at_b1(D, H1, j)] += (double)w.dpre1[j];
            }
            for (int k = 0; k < H2; ++k) {
                for (int j = 0; j < H1; ++j) sums[grad2_at_w2(D, H1, k, j)] += (double)(w.dpre2[k] * w.h1[j]);
                sums[grad2_at_b2(D, H1, H2, k)] += (double)w.dpre2[k];
                for (int a = 0; a < A; ++a) sums[grad2_at_w3(D, H1, H2, a, k)] += (double)(w.g.ds[a] * w.h2[k]);
            }
            for (int a = 0; a < A; ++a) sums[grad2_at_b3(D, A, H1, H2, a)] += (double)w.g.ds[a];
            sums[P] += (double)w.g.dls;
            for (int k = 0; k < kGradStats; ++k) sums[P + 1 + k] += (double)w.g.stat[k];
        }
}
#endif

#if defined(__HIPCC__)
// grad2.hip: the two launches of a two-layer gradient call on `stream`, arguments already checked (abi.hip); the weights stand in `pack_dev` by then
int grad2_launch(hipStream_t stream, const GradCall& call, int D, int A, int head, const float* pack_dev, int32_t hidden1, int32_t hidden2, int32_t activation);
#endif

}  // namespace mgym
