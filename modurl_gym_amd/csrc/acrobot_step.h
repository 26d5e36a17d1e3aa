// acrobot_step.h — Acrobot-v1 for ONE environment held in registers: the RK4 step, the reset draw and the on-device policy forms, exactly as
// include/mgym.h states them (MGYM_ACROBOT).  Not in the reference: gymnasium's Acrobot-v1 ("book" dynamics, m1 = m2 = l1 = 1, lc1 = lc2 = 0.5,
// I1 = I2 = 1, g = 9.8, dt = 0.2, no torque noise) with every operation an individually rounded f32 one — parity unpinned.  Plain host + device
// code like pendulum_step.h: the kernels of acrobot.hip and the host check tests/native/acrobot_check.cpp (g++ -ffp-contract=off) compile the SAME
// lines.
//
// What an environment is here: th1, th2, w1, w2 and (cos th1, sin th1, cos th2, sin th2) of those very angle words — the observation's first four
// components, kept beside the state under Pendulum's invariant (c == mg_cosf(th), s == mg_sinf(th) after every entry point that writes an angle),
// so that stage 1 of the integration and the termination test read stored words.  An environment-step then costs eight sincos pairs: two for each
// of the stages 2 - 4 and two for the new observation.  There is no data-dependent loop anywhere in the step: a non-finite state gives NaNs.
#pragma once
#include <math.h>
#include <stdint.h>
#include "mgym_math.h"
#include "time_limit.h"   // (also what gives a g++ build its empty __device__ / __forceinline__)
#include "philox.h"
#include "mlp_policy.h"

namespace mgym {

constexpr float kAbMaxVel1 = 12.566370614359172f, kAbMaxVel2 = 28.274333882308138f;   // V1 = (float)(4 pi), V2 = (float)(9 pi)
constexpr float kAbH = 0.1f, kAbDt = 0.2f;
constexpr float kAbPi = 3.14159274f, kAbTwoPi = 6.28318548f;   // PI_F, TWO_PI_F of include/mgym.h

// the compare form of the velocity clamps: a NaN passes through
MG_HD float ab_clamp(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// fmodf is exact by definition (the result is a representable float: no rounding), so the device library's and glibc's give the same word
MG_HD float ab_fmodf(float x, float y) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_fmodf(x, y);
#else
    return fmodf(x, y);
#endif
}

// cos and sin of one angle.  |th| < 120: mg_sincosf_u, bit-identical to mg_cosf / mg_sinf (glibc's) for every float and lock-step — a wave's arms point
// in every quadrant.  Beyond (RK4 stage angles of an extreme imported state): the out-of-line table reduction mg_sinf and mg_cosf themselves use, once
// per output — it returns its word by value, where the shared sincos form hands two back through memory, which would be the kernels' only scratch.
MG_HD void ab_sincos(float th, float& cs, float& sn) {
    if (abstop12(th) < abstop12(120.0f)) {
        mg_sincosf_u(th, &sn, &cs);
    } else {
        sn = mg_sincosf_large(th, 0);
        cs = mg_sincosf_large(th, 1);
    }
}

// what a lane keeps of one environment
struct AbEnv { float th1, th2, w1, w2, c1, s1, c2, s2; };

// (cos, sin) of both angles
MG_HD void acrobot_trig(AbEnv& e) {
    ab_sincos(e.th1, e.c1, e.s1);
    ab_sincos(e.th2, e.c2, e.s2);
}

// include/mgym.h, deriv(): the accelerations (dd1, dd2) from the trig words of the two angles, the velocities and the torque
MG_HD void acrobot_deriv(float s1, float c1, float s2, float c2, float w1, float w2, float tau, float& dd1, float& dd2) {
    const float s12 = s1 * c2 + c1 * s2;
    const float d1 = 3.5f + c2;
    const float d2 = 1.25f + 0.5f * c2;
    const float phi2 = 4.9f * s12;
    const float phi1 = (((-(0.5f * (w2 * w2)) * s2) - (w2 * w1) * s2) + 14.7f * s1) + phi2;
    dd2 = (((tau + (d2 / d1) * phi1) - (0.5f * (w1 * w1)) * s2) - phi2) / (1.25f - (d2 * d2) / d1);
    dd1 = -((d2 * dd2 + phi1) / d1);
}

// the loop-free wrap of an angle into [-pi, pi] (a NaN fails both comparisons and stays; an infinity gives fmodf's NaN)
MG_HD float acrobot_wrap(float x) {
    if (x > kAbPi || x < -kAbPi) {
        float r = ab_fmodf(x + kAbPi, kAbTwoPi);
        if (r < 0.0f) r += kAbTwoPi;
        x = r - kAbPi;
    }
    return x;
}

// One step (include/mgym.h, "step, action word a").  Returns false, with reward 0, done 0 and the environment untouched, for a > 2.
MG_HD bool acrobot_step_one(AbEnv& e, uint32_t action, float& reward, uint32_t& done) {
    if (action > 2u) { reward = 0.0f; done = 0u; return false; }
    const float tau = (float)action - 1.0f;
    const float dt6 = kAbDt / 6.0f;
    // k1 from the stored trig words (reducing the two angles again here instead gives the same words and was measured 9 - 11 % slower: DESIGN.md 5d)
    float a1, b1, a2, b2, a3, b3, a4, b4;   // (dd1, dd2) of the four stages
    acrobot_deriv(e.s1, e.c1, e.s2, e.c2, e.w1, e.w2, tau, a1, b1);
    AbEnv q;
    q.th1 = e.th1 + kAbH * e.w1; q.th2 = e.th2 + kAbH * e.w2; q.w1 = e.w1 + kAbH * a1; q.w2 = e.w2 + kAbH * b1;
    const float u2 = q.w1, v2 = q.w2;   // k2's first two components
    acrobot_trig(q);
    acrobot_deriv(q.s1, q.c1, q.s2, q.c2, q.w1, q.w2, tau, a2, b2);
    q.th1 = e.th1 + kAbH * u2; q.th2 = e.th2 + kAbH * v2; q.w1 = e.w1 + kAbH * a2; q.w2 = e.w2 + kAbH * b2;
    const float u3 = q.w1, v3 = q.w2;
    acrobot_trig(q);
    acrobot_deriv(q.s1, q.c1, q.s2, q.c2, q.w1, q.w2, tau, a3, b3);
    q.th1 = e.th1 + kAbDt * u3; q.th2 = e.th2 + kAbDt * v3; q.w1 = e.w1 + kAbDt * a3; q.w2 = e.w2 + kAbDt * b3;
    const float u4 = q.w1, v4 = q.w2;
    acrobot_trig(q);
    acrobot_deriv(q.s1, q.c1, q.s2, q.c2, q.w1, q.w2, tau, a4, b4);
    // y' = y + dt6 * (((k1 + 2 k2) + 2 k3) + k4)
    const float n_th1 = e.th1 + dt6 * (((e.w1 + 2.0f * u2) + 2.0f * u3) + u4);
    const float n_th2 = e.th2 + dt6 * (((e.w2 + 2.0f * v2) + 2.0f * v3) + v4);
    const float n_w1 = e.w1 + dt6 * (((a1 + 2.0f * a2) + 2.0f * a3) + a4);
    const float n_w2 = e.w2 + dt6 * (((b1 + 2.0f * b2) + 2.0f * b3) + b4);
    e.th1 = acrobot_wrap(n_th1);
    e.th2 = acrobot_wrap(n_th2);
    e.w1 = ab_clamp(n_w1, -kAbMaxVel1, kAbMaxVel1);
    e.w2 = ab_clamp(n_w2, -kAbMaxVel2, kAbMaxVel2);
    acrobot_trig(e);
    const bool term = (-e.c1 - (e.c1 * e.c2 - e.s1 * e.s2)) > 1.0f;
    done = term ? 1u : 0u;
    reward = term ? 0.0f : -1.0f;
    return true;
}

// A caller-visible step with the time limit: the step, then (TL) elapsed += 1 and truncated = elapsed >= limit.  As for MountainCar the count
// advances whether or not the action was valid.  Returns false for an invalid action.
template <bool TL>
MG_HD bool acrobot_env_step(uint32_t limit, AbEnv& e, uint32_t& elapsed, uint32_t action, float& reward, uint32_t& done, uint32_t& truncated) {
    const bool ok = acrobot_step_one(e, action, reward, done);
    truncated = 0u;
    if (TL) { elapsed = tl_advance(elapsed); truncated = tl_truncated(limit, elapsed); }
    return ok;
}

// Reset: four values ~ U[-0.1, 0.1), each sampled in f64 and rounded to f32 — the angles from the env's SLOT_RESET0 draw of this episode, the
// velocities from its SLOT_RESET1 draw; the caller then stores episode + 1 and elapsed = 0.
__device__ __forceinline__ void acrobot_reset_one(uint64_t seed, uint64_t env_id, uint32_t episode, AbEnv& e) {
    const Philox4 a = env_draw(seed, env_id, episode, SLOT_RESET0), b = env_draw(seed, env_id, episode, SLOT_RESET1);
    e.th1 = uniform_f64_to_f32(-0.1, 0.1, a.w[0], a.w[1]);
    e.th2 = uniform_f64_to_f32(-0.1, 0.1, a.w[2], a.w[3]);
    e.w1 = uniform_f64_to_f32(-0.1, 0.1, b.w[0], b.w[1]);
    e.w2 = uniform_f64_to_f32(-0.1, 0.1, b.w[2], b.w[3]);
    acrobot_trig(e);
}

// mgym_rollout_uniform, MountainCar's Discrete(3) draw: the four envs with global ids g .. g + 3 (g a multiple of 4) share one Philox stream keyed by
// the policy seed, counter (g lo, g hi, uniform call count, SLOT_POLICY + t / 2); step t takes half t % 2 of word k (low half first), h, and the
// action (3 h) >> 16.  A rollout evaluates the block on its even steps and keeps it for the odd one.
__device__ __forceinline__ Philox4 acrobot_uniform_block(uint64_t policy_seed, uint32_t call, uint64_t g, uint32_t t) {
    return philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), call, SLOT_POLICY + (t >> 1), (uint32_t)policy_seed, (uint32_t)(policy_seed >> 32));
}
MG_HD uint32_t acrobot_uniform_action(uint32_t w, uint32_t t) { return (((t & 1u) ? w >> 16 : w & 0xffffu) * 3u) >> 16; }

// mgym_rollout_linear: three rows of (6 weights, bias); s_j = ((((((w_j0 o0 + w_j1 o1) + w_j2 o2) + w_j3 o3) + w_j4 o4) + w_j5 o5) + b_j, the
// sequential strict argmax of the LunarLander form (the first of equal scores wins, a NaN never replaces an earlier score, a NaN s_0 gives 0)
struct AbLinearPolicy { float w[3][6], b[3]; };
MG_HD uint32_t acrobot_linear_action(const AbLinearPolicy& p, const float (&o)[6]) {
    float best = 0.0f;
    uint32_t a = 0u;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        float s = p.w[j][0] * o[0];
#pragma unroll
        for (int q = 1; q < 6; ++q) s = s + p.w[j][q] * o[q];
        s = s + p.b[j];
        if (j == 0) best = s;
        else if (s > best) { best = s; a = (uint32_t)j; }
    }
    return a;
}

// the observation an environment holds
MG_HD void acrobot_obs(const AbEnv& e, float (&o)[6]) { o[0] = e.c1; o[1] = e.s1; o[2] = e.c2; o[3] = e.s2; o[4] = e.w1; o[5] = e.w2; }

}  // namespace mgym
