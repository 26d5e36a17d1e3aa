// mlp_policy.h — the one-hidden-layer policy of mgym_rollout_mlp (include/mgym.h), shared by the rollout kernels of CartPole and MountainCar
// (cartpole.hip, mountain_car.hip: the lane's four environments), LunarLander's policy kernel (lunar_lander.hip: one environment per lane) and the
// host check tests/native/mlp_policy_check.cpp, which compiles this header with g++ (mgym_math.h's MG_HD is empty there).  Compile with
// -ffp-contract=off: the only fused operations are the cp_fmaf of the two chains.
//
//   pre_j = b1[j];  q = 0 .. D-1 ascending:  pre_j = fmaf(W1[j][q], o[q], pre_j)
//   h_j   = pre_j > 0 ? pre_j : +0  (ReLU: NaN and -0 give +0)   |   mg_tanhf(pre_j)
//   s_a   = b2[a];  j = 0 .. H-1 ascending:  s_a = fmaf(W2[a][j], h_j, s_a)
// Every chain is a k-ordered sequence of correctly rounded f32 fused multiply-adds that starts at the bias — which is also what an f32 MFMA
// computes with the bias as its C input, and what glibc's fmaf computes on the host.
#pragma once
#include <stdint.h>
#include "mgym_math.h"

namespace mgym {

constexpr int kMlpMaxHidden = 64;
enum { MLP_ACT_RELU = 0, MLP_ACT_TANH = 1 };   // = MGYM_ACT_RELU / MGYM_ACT_TANH

// The weights as the kernels read them, passed BY VALUE as a kernel argument (wave-uniform: scalar loads from the kernel-argument segment, and a
// captured graph carries them).  Hidden unit j's words are contiguous — W1[j][0 .. D-1], b1[j], W2[0 .. A-1][j] — so one unit is one run of scalar
// loads.  Units hidden .. 63 are zero and never read.  Largest: LunarLander (D = 8, A = 4), 4 + 64 * 13 * 4 + 16 = 3348 bytes.
template <int D, int A>
struct MlpPack {
    int32_t hidden;
    float unit[kMlpMaxHidden][D + 1 + A];
    float b2[A];
};

// number of floats of the caller's `policy` (nn.Linear order: W1[H][D], b1[H], W2[A][H], b2[A])
MG_HD int mlp_policy_floats(int D, int A, int H) { return H * (D + 1) + A * (H + 1); }

template <int D, int A>
MG_HD void mlp_pack(const float* policy, int H, MlpPack<D, A>& p) {
    const float *w1 = policy, *b1 = w1 + H * D, *w2 = b1 + H, *b2 = w2 + A * H;
    p.hidden = H;
    for (int j = 0; j < kMlpMaxHidden; ++j) {
        for (int q = 0; q < D; ++q) p.unit[j][q] = j < H ? w1[j * D + q] : 0.0f;
        p.unit[j][D] = j < H ? b1[j] : 0.0f;
        for (int a = 0; a < A; ++a) p.unit[j][D + 1 + a] = j < H ? w2[a * H + j] : 0.0f;
    }
    for (int a = 0; a < A; ++a) p.b2[a] = b2[a];
}

// the hidden activation: ReLU gives +0 for a NaN and for -0
template <int ACT>
MG_HD float mlp_activate(float pre) {
    if (ACT == MLP_ACT_TANH) return mg_tanhf(pre);
    return pre > 0.0f ? pre : 0.0f;
}

// one hidden unit: u = W1[j][0 .. D-1], b1[j]
template <int D, int ACT>
MG_HD float mlp_hidden(const float* u, const float (&o)[D]) {
    float pre = u[D];
#pragma unroll
    for (int q = 0; q < D; ++q) pre = cp_fmaf(u[q], o[q], pre);
    return mlp_activate<ACT>(pre);
}

// the A scores of N environments, streamed over the hidden units: unit j is computed, activated and folded into the running scores (no h[H] array)
template <int D, int A, int ACT, int N>
MG_HD void mlp_scores(const MlpPack<D, A>& p, const float (&o)[N][D], float (&s)[N][A]) {
#pragma unroll
    for (int k = 0; k < N; ++k)
#pragma unroll
        for (int a = 0; a < A; ++a) s[k][a] = p.b2[a];
    for (int j = 0; j < p.hidden; ++j) {
        const float* u = p.unit[j];
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const float h = mlp_hidden<D, ACT>(u, o[k]);
#pragma unroll
            for (int a = 0; a < A; ++a) s[k][a] = cp_fmaf(u[D + 1 + a], h, s[k][a]);
        }
    }
}

// the sequential strict argmax of ll_linear_action: the first of equal scores wins, a NaN never replaces an earlier score, a NaN s_0 gives 0
template <int A>
MG_HD uint32_t mlp_argmax(const float (&s)[A]) {
    float best = s[0];
    uint32_t a = 0u;
#pragma unroll
    for (int j = 1; j < A; ++j)
        if (s[j] > best) { best = s[j]; a = (uint32_t)j; }
    return a;
}

// the action words of N environments: the argmax (discrete families), or the one score's bits (MountainCarContinuous: CONT, A = 1)
template <int D, int A, int ACT, bool CONT, int N>
MG_HD void mlp_actions(const MlpPack<D, A>& p, const float (&o)[N][D], uint32_t (&act)[N]) {
    float s[N][A];
    mlp_scores<D, A, ACT, N>(p, o, s);
#pragma unroll
    for (int k = 0; k < N; ++k) act[k] = CONT ? as_u32(s[k][0]) : mlp_argmax<A>(s[k]);
}

}  // namespace mgym
