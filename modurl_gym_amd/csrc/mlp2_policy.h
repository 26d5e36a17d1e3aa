// mlp2_policy.h — the two-hidden-layer policy of mgym_rollout_mlp2 (include/mgym.h), shared by the rollout kernels of the classic families (the lane's four
// environments, taken as two packed pairs), LunarLander's ll_policy_mlp2_kernel (one environment per lane) and the host check tests/native/policy_check.cpp,
// which compiles this header with g++ (mgym_math.h's MG_HD is empty there).  Compile with -ffp-contract=off: the only fused operations are the cp_fmaf of
// the three chains.
//
//   pre1_j = b1[j];  q = 0 .. D-1  ascending:  pre1_j = fmaf(W1[j][q], o[q], pre1_j);   h1_j = act(pre1_j)
//   pre2_k = b2[k];  j = 0 .. H1-1 ascending:  pre2_k = fmaf(W2[k][j], h1_j, pre2_k);   h2_k = act(pre2_k)
//   s_a    = b3[a];  k = 0 .. H2-1 ascending:  s_a    = fmaf(W3[a][k], h2_k, s_a)
// act is mlp_policy.h's mlp_activate (ReLU or mg_tanhf_fast).  This header gives the scores only, as an overload of mlp_scores on Mlp2Net: the action call and its
// three heads are mlp_policy.h's mlp_actions, the same function for both depths.
//
// No chain is padded: fmaf(+0, +0, -0) is +0, so a chain run past its length over zero weights would turn a -0 pre-activation into +0, and mg_tanhf_fast
// and the last chain carry that sign into the action word.  The chains over H1 terms run in whole chunks of 8 with a wave-uniform exit, then over the
// H1 % 8 units of the last chunk, which layer 1 keeps in registers of their own: h1 is indexed statically everywhere (a tail that indexes h1 from a run-time
// chunk base puts the whole array in scratch).  The units of layer 2 are a run-time loop, as the units of mlp_scores are.
#pragma once
#include <stdint.h>
#include "mlp_policy.h"

namespace mgym {

// The weights as the kernels read them: a run of floats in device memory, the handle's own (Env::mlp2_dev), addressed in the constant address space — every
// read is a wave-uniform scalar load.  At (64, 64) they are up to 20 768 bytes, five times what a kernel argument may hold.
//   [0 .. 7]                    b3[0 .. A-1], zeros
//   l1 = 8, unit j              W1[j][0 .. D-1], b1[j]                                (D + 1 words; round8(H1) units, those from H1 on zero)
//   l2 = l1 + round8(H1)(D+1)   unit k:  b2[k], W3[0 .. A-1][k], zeros to 8 words,  W2[k][0 .. H1-1], zeros to round8(H1) words
// so one unit of layer 2 is one contiguous, 32-byte aligned run.  The zeros are loaded with their chunk and never enter a chain that is read.
constexpr int kMlp2Head = 8;
constexpr int mlp2_round8(int v) { return (v + 7) & ~7; }
constexpr int mlp2_l2_offset(int D, int H1) { return kMlp2Head + mlp2_round8(H1) * (D + 1); }
constexpr int mlp2_l2_stride(int H1) { return kMlp2Head + mlp2_round8(H1); }
constexpr int mlp2_pack_floats(int D, int H1, int H2) { return mlp2_l2_offset(D, H1) + H2 * mlp2_l2_stride(H1); }
constexpr int kMlp2PackMax = mlp2_pack_floats(8, kMlpMaxHidden, kMlpMaxHidden);   // LunarLander's D: 5 192 floats

// number of floats of the caller's `policy` (nn.Linear order: W1[H1][D], b1[H1], W2[H2][H1], b2[H2], W3[A][H2], b3[A])
constexpr int mlp2_policy_floats(int D, int A, int H1, int H2) { return H1 * (D + 1) + H2 * (H1 + 1) + A * (H2 + 1); }

// the caller's policy -> the pack (out: mlp2_pack_floats(D, H1, H2) floats)
MG_HD void mlp2_pack(const float* policy, int D, int A, int H1, int H2, float* out) {
    const float *w1 = policy, *b1 = w1 + H1 * D, *w2 = b1 + H1, *b2 = w2 + H2 * H1, *w3 = b2 + H2, *b3 = w3 + A * H2;
    const int n = mlp2_pack_floats(D, H1, H2), l2 = mlp2_l2_offset(D, H1), stride = mlp2_l2_stride(H1);
    for (int i = 0; i < n; ++i) out[i] = 0.0f;
    for (int a = 0; a < A; ++a) out[a] = b3[a];
    for (int j = 0; j < H1; ++j) {
        float* u = out + kMlp2Head + j * (D + 1);
        for (int q = 0; q < D; ++q) u[q] = w1[j * D + q];
        u[D] = b1[j];
    }
    for (int k = 0; k < H2; ++k) {
        float* u = out + l2 + k * stride;
        u[0] = b2[k];
        for (int a = 0; a < A; ++a) u[1 + a] = w3[a * H2 + k];
        for (int j = 0; j < H1; ++j) u[kMlp2Head + j] = w2[k * H1 + j];
    }
}

// What a kernel takes by value: the pack's address, the two widths, and the Gaussian head's sigma (D and A only select the overloads)
template <int D, int A>
struct Mlp2Net {
    const float* pack;
    int32_t h1, h2;
    float sigma;
};

#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) float* Mlp2Ptr;
// (the constant-space pointer goes through an empty asm, as in ll_roll.h's roll_decide: a plain cast there and back is folded away and the loads stay global)
__device__ __forceinline__ Mlp2Ptr mlp2_const(const float* p) {
    Mlp2Ptr cp = (Mlp2Ptr)p;
    asm("" : "+s"(cp));
    return cp;
}
// the branch-free activation and the unrolled chunks leave the scheduler free to interleave every unit of a chunk and to issue every chunk's scalar loads at
// once, and it then runs out of both register files (512 registers and spills at 64 tanh_fast units); a scheduling barrier per unit of layer 1 and per chunk of
// the middle layer orders them as written (the barrier mlp_scores places per environment)
#define MLP2_ORDER() __builtin_amdgcn_sched_barrier(0)
#else
typedef const float* Mlp2Ptr;
static inline Mlp2Ptr mlp2_const(const float* p) { return p; }
#define MLP2_ORDER() ((void)0)
#endif

// one unit of layer 1: u = W1[j][0 .. D-1], b1[j]
template <int D, int ACT>
MG_HD float mlp2_hidden1(Mlp2Ptr u, const float (&o)[D]) {
    float pre = u[D];
#pragma unroll
    for (int q = 0; q < D; ++q) pre = cp_fmaf(u[q], o[q], pre);
    return mlp_activate<ACT>(pre);
}

// the A scores of N environments.  N = 4 (a lane of the classic kernels): two pairs, one after the other — a pair's h1 is 128 registers, four environments'
// would be 256 beside the state — each FMA of the middle layer serving both members of the pair with one scalar weight; N = 1: LunarLander and the host.
template <int D, int A, int ACT, int N>
MG_HD void mlp_scores(const Mlp2Net<D, A>& net, const float (&o)[N][D], float (&s)[N][A]) {
    constexpr int P = N >= 2 ? 2 : 1;
    static_assert(N % P == 0, "whole pairs");
    const int H1 = net.h1, H2 = net.h2;
    const Mlp2Ptr p = mlp2_const(net.pack);
    const int l2 = mlp2_l2_offset(D, H1), stride = mlp2_l2_stride(H1);
    const int full = H1 & ~7, rem = H1 & 7;   // the whole chunks of 8 units of layer 1, and the units of its last, partial chunk
#pragma unroll
    for (int g = 0; g < N / P; ++g) {
        float h1[kMlpMaxHidden][P], ht[7][P];   // units 0 .. full - 1, and units full .. H1 - 1
#pragma unroll
        for (int c = 0; c < kMlpMaxHidden; c += 8) {
            if (c >= full) break;   // wave-uniform
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                if (c + jj >= H1) break;   // (never taken in a whole chunk: a wave-uniform branch per unit keeps the units' activations from being batched)
#pragma unroll
                for (int e = 0; e < P; ++e) h1[c + jj][e] = mlp2_hidden1<D, ACT>(p + kMlp2Head + (c + jj) * (D + 1), o[g * P + e]);
                MLP2_ORDER();
            }
        }
#pragma unroll
        for (int jj = 0; jj < 7; ++jj) {
            if (jj >= rem) break;
#pragma unroll
            for (int e = 0; e < P; ++e) ht[jj][e] = mlp2_hidden1<D, ACT>(p + kMlp2Head + (full + jj) * (D + 1), o[g * P + e]);
            MLP2_ORDER();
        }
#pragma unroll
        for (int e = 0; e < P; ++e)
#pragma unroll
            for (int a = 0; a < A; ++a) s[g * P + e][a] = p[a];
        for (int k = 0; k < H2; ++k) {
            const Mlp2Ptr u = p + l2 + k * stride;
            float pre[P];
#pragma unroll
            for (int e = 0; e < P; ++e) pre[e] = u[0];
#pragma unroll
            for (int c = 0; c < kMlpMaxHidden; c += 8) {
                if (c >= full) break;
#pragma unroll
                for (int jj = 0; jj < 8; ++jj)
#pragma unroll
                    for (int e = 0; e < P; ++e) pre[e] = cp_fmaf(u[kMlp2Head + c + jj], h1[c + jj][e], pre[e]);
                MLP2_ORDER();
            }
#pragma unroll
            for (int jj = 0; jj < 7; ++jj) {   // the chain ends at H1 - 1
                if (jj >= rem) break;
#pragma unroll
                for (int e = 0; e < P; ++e) pre[e] = cp_fmaf(u[kMlp2Head + full + jj], ht[jj][e], pre[e]);
            }
#pragma unroll
            for (int e = 0; e < P; ++e) {
                const float h2 = mlp_activate<ACT>(pre[e]);
#pragma unroll
                for (int a = 0; a < A; ++a) s[g * P + e][a] = cp_fmaf(u[1 + a], h2, s[g * P + e][a]);
            }
        }
        MLP2_ORDER();   // one pair's h1 live at a time
    }
}

#if !defined(__HIPCC__)
// Host builds only (g++): the earlier names of the scores, the heads and the action call, forwarding to mlp_scores and mlp_actions; no file of the tree uses them
// (as mlp_policy.h's earlier spellings).
enum { MLP2_HEAD_GREEDY = MLP_HEAD_GREEDY, MLP2_HEAD_SAMPLE = MLP_HEAD_SAMPLE, MLP2_HEAD_GAUSS = MLP_HEAD_GAUSS };
template <int D, int A, int ACT, int N>
MG_HD void mlp2_scores(const Mlp2Net<D, A>& net, const float (&o)[N][D], float (&s)[N][A]) { mlp_scores<D, A, ACT, N>(net, o, s); }
template <int D, int A, int ACT, int HEAD, int N>
MG_HD void mlp2_actions(const Mlp2Net<D, A>& net, const float (&o)[N][D], const uint32_t (&w)[N], float sigma, uint32_t (&act)[N]) {
    mlp_actions<D, A, ACT, HEAD, N>(net, o, w, sigma, act);
}
#endif

}  // namespace mgym
