// mlp_policy.h — the one-hidden-layer policy of mgym_rollout_mlp, mgym_rollout_mlp_sample and mgym_rollout_mlp_gauss (include/mgym.h), shared by the rollout
// kernels of CartPole, MountainCar and Pendulum (cartpole.hip, mountain_car.hip, pendulum.hip: the lane's four environments), LunarLander's policy kernel
// (lunar_lander.hip: one environment per lane) and the host checks tests/native/policy_check.cpp, mlp_sample_check.cpp and mlp_gauss_check.cpp, which compile this header with g++ (mgym_math.h's MG_HD is empty there).  Compile with
// -ffp-contract=off: the only fused operations are the cp_fmaf of the two chains.  The header also holds the one action call of both depths, mlp_actions<D, A,
// ACT, HEAD, N>(net, o, w, sigma, act): the scores of `net` (this header's MlpPack, or mlp2_policy.h's Mlp2Net) and then the head, MLP_HEAD_GREEDY / _SAMPLE / _GAUSS.
//
//   pre_j = b1[j];  q = 0 .. D-1 ascending:  pre_j = fmaf(W1[j][q], o[q], pre_j)
//   h_j   = pre_j > 0 ? pre_j : +0  (ReLU: NaN and -0 give +0)   |   mg_tanhf(pre_j)   |   mg_tanhf_fast(pre_j)
//   s_a   = b2[a];  j = 0 .. H-1 ascending:  s_a = fmaf(W2[a][j], h_j, s_a)
// Every chain is a k-ordered sequence of correctly rounded f32 fused multiply-adds that starts at the bias — which is also what an f32 MFMA
// computes with the bias as its C input, and what glibc's fmaf computes on the host.
#pragma once
#include <stdint.h>
#include <type_traits>
#include "mgym_math.h"

namespace mgym {

constexpr int kMlpMaxHidden = 64;
enum { MLP_ACT_RELU = 0, MLP_ACT_TANH = 1, MLP_ACT_TANH_FAST = 3 };   // = MGYM_ACT_RELU / MGYM_ACT_TANH / MGYM_ACT_TANH_FAST (2 is not an activation)
enum { MLP_HEAD_GREEDY = 0, MLP_HEAD_SAMPLE = 1, MLP_HEAD_GAUSS = 2 };     // = MGYM_HEAD_*: how the scores become the action word (mlp_actions, below)

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
    if (ACT == MLP_ACT_TANH_FAST) return mg_tanhf_fast(pre);
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
#if defined(__HIP_DEVICE_COMPILE__) && !defined(MLP_TANH_FAST_NO_BARRIER)
            // the branch-free activation leaves a lane's N environments' chains free to interleave, and the compiler then keeps all of them live at once; a
            // scheduling barrier after each environment (or packed pair) orders them as the branches of mg_tanhf do: up to 16 fewer VGPRs, and the launch
            // measured beside a build without it (make EXTRA=-DMLP_TANH_FAST_NO_BARRIER) in profiles/tanh_fast_kernel_resources.txt
            if (ACT == MLP_ACT_TANH_FAST && N > 1) __builtin_amdgcn_sched_barrier(0);
#endif
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

// ---- mgym_rollout_mlp_sample: the action drawn from the categorical distribution over the scores (include/mgym.h, "The draw") ----
//   m = the running best of mlp_argmax;  e_a = mg_expm1f(s_a - m) + 1;  c_a = c_{a-1} + e_a;  thr = u * c_{A-1};  the first a with thr < c_a, else A - 1
// f32, nothing fused.  The best action b (the index mlp_argmax returns) has s_b - m = m - m, which is +0 for a finite m and a NaN otherwise, and
// mg_expm1f(+0) + 1 = 1, mg_expm1f(NaN) + 1 = NaN: its weight is (m - m) + 1 without the call, the same word for a finite m and a NaN where the text gives
// one.  So an environment-step costs A - 1 evaluations of mg_expm1f: CartPole one, of -|s_0 - s_1|.

// c_0 .. c_{A-1}
template <int A>
MG_HD void mlp_sample_cum(const float (&s)[A], float (&c)[A]) {
    static_assert(A >= 2, "a draw needs two actions");
    float m = s[0];
    int b = 0;
#pragma unroll
    for (int a = 1; a < A; ++a)
        if (s[a] > m) { m = s[a]; b = a; }
    float ex[A - 1];   // the weights of the other actions in ascending order: entry k is action k below b, k + 1 from b on
#pragma unroll
    for (int k = 0; k < A - 1; ++k) ex[k] = mg_expm1f((k >= b ? s[k + 1] : s[k]) - m) + 1.0f;
    const float eb = (m - m) + 1.0f;
    float acc = 0.0f;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        const float lo = ex[a > 0 ? a - 1 : 0], hi = ex[a < A - 1 ? a : A - 2];
        const float e = a == b ? eb : (a > b ? lo : hi);
        acc = a == 0 ? e : acc + e;
        c[a] = acc;
    }
}

// u = (w >> 8) 2^-24 in [0, 1), thr = u * c_{A-1}: the first a in 0 .. A-2 with thr < c_a, else A - 1 (a NaN makes every comparison false)
template <int A>
MG_HD uint32_t mlp_sample_pick(const float (&c)[A], uint32_t w) {
    const float u = (float)(w >> 8) * 5.9604644775390625e-08f;
    const float thr = u * c[A - 1];
    uint32_t act = (uint32_t)(A - 1);
#pragma unroll
    for (int a = A - 2; a >= 0; --a)
        if (thr < c[a]) act = (uint32_t)a;
    return act;
}

template <int A>
MG_HD uint32_t mlp_sample(const float (&s)[A], uint32_t w) {
    float c[A];
    mlp_sample_cum<A>(s, c);
    return mlp_sample_pick<A>(c, w);
}

// ---- mgym_rollout_mlp_gauss: the one score is the mean of a Gaussian, a = mu + sigma * z (include/mgym.h, "The draw of z") ----
// One Box-Muller transform turns a pair of Philox words into two independent normals, r cos(phi) for the even member of an environment pair and r sin(phi)
// for the odd one, with r = sqrt(-2 ln u1).  The logarithm is the project's own: no library's log is defined to the word, and this one is a handful of
// individually rounded f64 operations that numpy restates.

// ln(n 2^-25) for an odd n in 1 .. 2^25 - 1, in f64: n = m 2^e with m in (sqrt(1/2), sqrt(2)], s = (m - 1) / (m + 1), ln m = 2 atanh(s) as the odd series up
// to s^15 (|s| <= 0.1716: the first dropped term is 3.3e-14 of the result), Horner in s^2 from 2/15 down to 2, then (e - 25) ln2 + that.  Nothing fused; when
// e = 25 the first product is 0 and the series is all of L, so nothing cancels.
MG_HD double mg_log_u25(uint32_t n) {
    int e = 31 - __builtin_clz(n);
    double m = (double)(n << (24 - e)) * 0x1p-24;   // the mantissa of (double)n, in [1, 2): both steps exact
    if (m > 0x1.6a09e667f3bcdp+0) { m *= 0.5; e += 1; }
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
    return (double)(e - 25) * 0x1.62e42fefa39efp-1 + p;
}

// q = -2 ln(u1) as an f32, u1 = (2 (wa >> 8) + 1) 2^-25 in (0, 1): one f64 multiply, one rounding to f32; 5.96e-8 <= q <= 34.66
MG_HD float mlp_gauss_q(uint32_t wa) { return (float)(-2.0 * mg_log_u25(2u * (wa >> 8) + 1u)); }

// the correctly rounded f32 square root (hipcc's default for gfx950, sqrtss on the host)
MG_HD float mlp_sqrtf(float x) { return __builtin_sqrtf(x); }

// the two normals of one pair of words
MG_HD void mlp_gauss_pair(uint32_t wa, uint32_t wb, float* z_even, float* z_odd) {
    const float r = mlp_sqrtf(mlp_gauss_q(wa));
    const float phi = ((float)(wb >> 8) * 5.9604644775390625e-08f) * 6.28318548f;   // at most (1 - 2^-24) * 6.28318548f, below 2 pi
    // so mg_sincosf_u (word-equal to mg_sinf / mg_cosf) always takes its lock-step form for |y| < 120; saying so drops its out-of-line path for larger
    // arguments from these kernels, which hands its two results back through memory and would be their only scratch
    if (!(abstop12(phi) < abstop12(120.0f))) __builtin_unreachable();
    float s, c;
    mg_sincosf_u(phi, &s, &c);
    *z_even = r * c;
    *z_odd = r * s;
}

// ---- the action call, the one copy for both depths: the scores of N environments under `net`, then the head that turns them into action words ----
// `net` is an MlpPack here, or mlp2_policy.h's Mlp2Net: mlp_scores is overloaded on it.  The heads (MLP_HEAD_*):
//   GREEDY  the argmax (A > 1) or the one score's bits (A = 1: the continuous families); w and sigma are not read
//   SAMPLE  environment k draws with the word w[k] (A > 1)
//   GAUSS   N = 4, A = 1: the lane's four environments (global ids g .. g + 3, g a multiple of 4) take the four normals of one Philox block w — (w0, w1) for
//           the first pair, (w2, w3) for the second — and the action word is that of mu + sigma * z, an f32 multiply and an f32 add, before any clamp
// The head stands in the function that owns the scores, not in one of its own that takes them: handed on by reference the twelve scores of a lane come out of
// the compiler's scalar replacement in another order, and every SAMPLE kernel of the classic families changes its register allocation.
template <int D, int A> struct Mlp2Net;   // (mlp2_policy.h)
template <int D, int A, int ACT, int HEAD, int N, class Net>
MG_HD void mlp_actions(const Net& net, const float (&o)[N][D], const uint32_t (&w)[N], float sigma, uint32_t (&act)[N]) {
    static_assert(std::is_same_v<Net, MlpPack<D, A>> || std::is_same_v<Net, Mlp2Net<D, A>>, "net: the MlpPack or the Mlp2Net of these D and A");
    float s[N][A];
    mlp_scores<D, A, ACT, N>(net, o, s);
    if constexpr (HEAD == MLP_HEAD_GAUSS) {
        static_assert(A == 1 && N == 4, "the Gaussian head: the continuous families, a lane of four");
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float ze, zo;
            mlp_gauss_pair(w[2 * h], w[2 * h + 1], &ze, &zo);
            act[2 * h] = as_u32(s[2 * h][0] + sigma * ze);
            act[2 * h + 1] = as_u32(s[2 * h + 1][0] + sigma * zo);
        }
    } else if constexpr (HEAD == MLP_HEAD_SAMPLE) {
        static_assert(A >= 2, "a draw needs two actions");
#pragma unroll
        for (int k = 0; k < N; ++k) act[k] = mlp_sample<A>(s[k], w[k]);
    } else {
        static_assert(HEAD == MLP_HEAD_GREEDY, "one of the three heads");
#pragma unroll
        for (int k = 0; k < N; ++k) act[k] = A == 1 ? as_u32(s[k][0]) : mlp_argmax<A>(s[k]);
    }
}

#if !defined(__HIPCC__)
// Host builds only (g++): the three earlier spellings of that call, told apart by their argument lists, forwarding to the one call above.  No file of the tree
// calls them — every host check under tests/native uses the five-argument call; they keep a check program written against the earlier spellings compiling
// against this header.  A kernel's translation unit does not see them: under hipcc mlp_actions is the one template.
//   <D, A, ACT, CONT, N>(p, o, act)        GREEDY (CONT said what A == 1 says)
//   <D, A, ACT, N>(p, o, w, act)            SAMPLE
//   <D, ACT>(p, o, w, sigma, act)           GAUSS, N = 4
template <int D, int A, int ACT, bool CONT, int N>
MG_HD void mlp_actions(const MlpPack<D, A>& p, const float (&o)[N][D], uint32_t (&act)[N]) {
    static_assert(CONT == (A == 1), "the one score is the action exactly when there is one");
    const uint32_t w[N] = {};
    mlp_actions<D, A, ACT, MLP_HEAD_GREEDY, N>(p, o, w, 0.0f, act);
}
template <int D, int A, int ACT, int N>
MG_HD void mlp_actions(const MlpPack<D, A>& p, const float (&o)[N][D], const uint32_t (&w)[N], uint32_t (&act)[N]) {
    mlp_actions<D, A, ACT, MLP_HEAD_SAMPLE, N>(p, o, w, 0.0f, act);
}
template <int D, int ACT>
MG_HD void mlp_actions(const MlpPack<D, 1>& p, const float (&o)[4][D], const uint32_t (&w)[4], float sigma, uint32_t (&act)[4]) {
    mlp_actions<D, 1, ACT, MLP_HEAD_GAUSS, 4>(p, o, w, sigma, act);
}
#endif

// (grad.h restates two pieces of this header line for line, so that these stay as they are: mlp_hidden's chain in grad_unit, which also needs pre_j, and
// mlp_sample_cum's weights in PpoCategorical::step, which needs the e_a themselves.  A change to either belongs in both places; tests/test_grad_host.py
// compares the copies' words with the restatement of these.)

}  // namespace mgym
