// pendulum_step.h — Pendulum-v1 for ONE environment held in registers: the step, the reset draw and the three on-device policy forms, exactly as
// include/mgym.h states them (MGYM_PENDULUM).  Not in the reference: gymnasium's Pendulum-v1 (m = l = 1, dt = 0.05, max_speed 8, max_torque 2) with
// every operation an individually rounded f32 one — parity unpinned.  Plain host + device code like cartpole_step.h and mlp_policy.h: the kernels of
// pendulum.hip and the host check tests/native/pendulum_check.cpp (g++ -ffp-contract=off) compile the SAME lines.
//
// What an environment is here: th (not wrapped), thdot, and (cos th, sin th) of that very th word — the observation's first two components, kept
// beside the state so that the step's sinf(th) is the stored word and one sincos serves an environment-step (Pendulum).  The invariant
// cs == mg_cosf(th), sn == mg_sinf(th) holds after every entry point that writes th (step, every reset form, mgym_set_state, mgym_create).
#pragma once
#include <math.h>
#include <stdint.h>
#include "mgym_math.h"
#include "time_limit.h"   // (also what gives a g++ build its empty __device__ / __forceinline__)
#include "philox.h"
#include "mlp_policy.h"

namespace mgym {

constexpr float kPdPi = 3.14159274f, kPdTwoPi = 6.28318548f;   // PI_F, TWO_PI_F of include/mgym.h
constexpr float kPdMaxSpeed = 8.0f, kPdMaxTorque = 2.0f, kPdDt = 0.05f;

// the one host-side constant: c_g = 1.5f * g (3 g / (2 l) with l = 1), one f32 multiply
MG_HD float pendulum_c_g(float g) { return 1.5f * g; }

// the compare form of u and thdot': a NaN passes through
MG_HD float pd_clamp(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// fmodf is exact by definition (the result is a representable float: no rounding), so the device library's and glibc's give the same word
MG_HD float pd_fmodf(float x, float y) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_fmodf(x, y);
#else
    return fmodf(x, y);
#endif
}

// cos and sin of th, the observation's words.  |th| < 120 (a pendulum that has turned fewer than 19 times): mg_sincosf_u, bit-identical to mg_cosf /
// mg_sinf (glibc's) for every float and lock-step — a wave's pendulums point in every quadrant, so the branchy form would run all of its paths.
// Beyond: the out-of-line table reduction mg_sinf and mg_cosf themselves use, once per output — it returns its word by value, where the shared
// sincos form hands two back through memory, which would be the kernels' only scratch.
MG_HD void pendulum_sincos(float th, float& cs, float& sn) {
    if (abstop12(th) < abstop12(120.0f)) {
        mg_sincosf_u(th, &sn, &cs);
    } else {
        sn = mg_sincosf_large(th, 0);
        cs = mg_sincosf_large(th, 1);
    }
}

// One step (include/mgym.h, "Step with action word a").  `sn` is sinf(th) of the state before the step (the stored word).  Returns false, with reward 0
// and th, thdot, cs, sn untouched, for a NaN action.  done is 0 always and is not an output.
MG_HD bool pendulum_step_one(float c_g, float& th, float& thdot, float& cs, float& sn, uint32_t action_bits, float& reward) {
    const float a = as_f32(action_bits);
    if (a != a) { reward = 0.0f; return false; }
    const float u = pd_clamp(a, -kPdMaxTorque, kPdMaxTorque);
    const float x = th + kPdPi;
    float r = pd_fmodf(x, kPdTwoPi);
    if (r < 0.0f) r += kPdTwoPi;
    const float an = r - kPdPi;
    const float cost = (an * an + 0.1f * (thdot * thdot)) + 0.001f * (u * u);
    const float acc = c_g * sn + 3.0f * u;
    thdot = pd_clamp(thdot + acc * kPdDt, -kPdMaxSpeed, kPdMaxSpeed);
    th = th + thdot * kPdDt;
    pendulum_sincos(th, cs, sn);
    reward = -cost;
    return true;
}

// A caller-visible step with the time limit: the step, then (TL) elapsed += 1 and truncated = elapsed >= limit.  As for MountainCar the count
// advances whether or not the action was valid.  Returns false for a NaN action.
template <bool TL>
MG_HD bool pendulum_env_step(float c_g, uint32_t limit, float& th, float& thdot, float& cs, float& sn, uint32_t& elapsed, uint32_t action_bits,
                             float& reward, uint32_t& truncated) {
    const bool ok = pendulum_step_one(c_g, th, thdot, cs, sn, action_bits, reward);
    truncated = 0u;
    if (TL) { elapsed = tl_advance(elapsed); truncated = tl_truncated(limit, elapsed); }
    return ok;
}

// Reset: th ~ U[-pi, pi), thdot ~ U[-1, 1), each sampled in f64 and rounded to f32, from the env's draw of this episode; the caller then stores
// episode + 1 and elapsed = 0.
__device__ __forceinline__ void pendulum_reset_one(uint64_t seed, uint64_t env_id, uint32_t episode, float& th, float& thdot, float& cs, float& sn) {
    const Philox4 a = env_draw(seed, env_id, episode, SLOT_RESET0);
    th = uniform_f64_to_f32(-3.14159265358979323846, 3.14159265358979323846, a.w[0], a.w[1]);
    thdot = uniform_f64_to_f32(-1.0, 1.0, a.w[2], a.w[3]);
    pendulum_sincos(th, cs, sn);
}

// mgym_rollout_uniform: the four envs with global ids g .. g + 3 (g a multiple of 4) take the four words of one Philox block keyed by the policy
// seed, counter (g lo, g hi, uniform call count, SLOT_POLICY + t); the top 24 bits u of a word give the torque u 2^-22 - 2, exact, over the multiples
// of 2^-22 in [-2, 2)
MG_HD uint32_t pendulum_uniform_action(uint32_t w) { return as_u32((float)(w >> 8) * 2.384185791015625e-07f - 2.0f); }
__device__ __forceinline__ void pendulum_uniform_actions(uint64_t policy_seed, uint32_t call, uint64_t g, uint32_t t, uint32_t (&a)[4]) {
    const Philox4 b = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), call, SLOT_POLICY + t, (uint32_t)policy_seed, (uint32_t)(policy_seed >> 32));
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = pendulum_uniform_action(b.w[k]);
}

// mgym_rollout_linear: policy = (w_cos, w_sin, w_thdot, b); the score is the torque (the step clamps it)
struct PdLinearPolicy { float w[3], b; };
MG_HD uint32_t pendulum_linear_action(const PdLinearPolicy& p, float cs, float sn, float thdot) {
    return as_u32(((p.w[0] * cs + p.w[1] * sn) + p.w[2] * thdot) + p.b);
}

// mgym_rollout_mlp / _mlp2: D = 3, A = 1 in mlp_policy.h's mlp_actions — s_0 is the torque (policy.h's policy_actions4)
#if !defined(__HIPCC__)
// Host builds only (g++): the forwarding function the kernels once called; no file of the tree calls it (as mlp_policy.h's earlier spellings)
template <int ACT, int N>
MG_HD void pendulum_mlp_actions(const MlpPack<3, 1>& p, const float (&o)[N][3], uint32_t (&a)[N]) { mlp_actions<3, 1, ACT, true, N>(p, o, a); }
#endif

// mgym_rollout_mlp_gauss: the torque is s_0 + sigma * z, the four envs with global ids g .. g + 3 (g a multiple of 4) taking the four normals of one Philox
// block keyed by the policy seed, counter (g lo, g hi, call, SLOT_POLICY_GAUSS + t) (mlp_policy.h's GAUSS head; the step clamps the torque).  A forwarding
// function kept on purpose: with this draw and call written into the kernel, or made through policy.h's policy_draw / policy_actions4, the nine Gaussian
// kernels of one hidden layer hoist their Philox key schedule in another order
template <int ACT>
__device__ __forceinline__ void pendulum_gauss_actions(const MlpPack<3, 1>& p, const float (&o)[4][3], uint64_t policy_seed, uint32_t call, uint64_t g, uint32_t t, float sigma,
                                                       uint32_t (&a)[4]) {
    const Philox4 b = env_draw(policy_seed, g, call, SLOT_POLICY_GAUSS + t);
    mlp_actions<3, 1, ACT, MLP_HEAD_GAUSS, 4>(p, o, b.w, sigma, a);
}

}  // namespace mgym
