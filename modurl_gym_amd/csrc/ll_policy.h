// ll_policy.h — the two on-device policies of mgym_rollout_linear / mgym_rollout_uniform for LunarLanderV3 (Discrete(4), obs_dim 8), shared by the
// persistent rollout launch (ll_roll.h), the K-step form's policy kernel (lunar_lander.hip) and the host check tests/native/ll_policy_check.cpp, which
// compiles this header for the CPU (with a shim for the HIP qualifiers, as ll_host_check.cpp does for ll_env.h).  Compile with -ffp-contract=off: the
// scores are f32 products and sums in the documented order, each rounded on its own.
#pragma once
#include <stdint.h>
#include "philox.h"

namespace mgym {

// mgym_rollout_linear: 4 rows of (w_j0 .. w_j7, b_j), passed by value as a kernel argument (wave-uniform: scalar registers)
constexpr int kLLPolicyFloats = 4 * (8 + 1);
struct LLLinearPolicy { float w[4][8]; float b[4]; };

// s_j = (((((((w_j0 o0 + w_j1 o1) + w_j2 o2) + w_j3 o3) + w_j4 o4) + w_j5 o5) + w_j6 o6) + w_j7 o7) + b_j; the action is the first j of the largest s_j
// (strict >: equal scores keep the earlier row; a NaN score never replaces an earlier one, and nothing compares greater than a NaN s_0: action 0)
__device__ __forceinline__ uint32_t ll_linear_action(const LLLinearPolicy& p, const float o[8]) {
    float best = 0.0f;
    uint32_t a = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float s = p.w[j][0] * o[0];
#pragma unroll
        for (int q = 1; q < 8; ++q) s = s + p.w[j][q] * o[q];
        s = s + p.b[j];
        if (j == 0) best = s;
        else if (s > best) { best = s; a = (uint32_t)j; }
    }
    return a;
}

// mgym_rollout_uniform: env with global id g takes, at step t of the call, bits 2 (t % 16) .. 2 (t % 16) + 1 of word g % 4 of
// Philox4x32-10(key = seed; counter = (g & ~3, call, SLOT_POLICY + t / 16)) — the key and counter scheme of CartPole's policy stream
__device__ __forceinline__ uint32_t ll_uniform_action(uint64_t seed, uint32_t call, uint64_t g, uint32_t t) {
    const Philox4 w = env_draw(seed, g & ~3ull, call, SLOT_POLICY + t / 16u);
    const uint32_t k = (uint32_t)(g & 3u);
    const uint32_t word = k == 0u ? w.w[0] : k == 1u ? w.w[1] : k == 2u ? w.w[2] : w.w[3];   // (selects: no run-time index into a private array)
    return (word >> (2u * (t & 15u))) & 3u;
}

}  // namespace mgym
