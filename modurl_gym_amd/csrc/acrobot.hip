// acrobot.hip — Acrobot-v1 step()/reset() and the fused rollouts as struct-of-arrays gfx950 kernels.
//
// NOT in the reference: gymnasium's Acrobot-v1 ("book" dynamics, RK4, no torque noise) restated in f32 (include/mgym.h, MGYM_ACROBOT;
// acrobot_step.h holds the per-environment lines), parity unpinned.  Episodes end when the tip swings above the bar, or by
// mgym_config::max_episode_steps (time_limit.h).
//
// Data layout in HBM (engine-owned), nine columns n_pad words apart: cos1[n] sin1[n] cos2[n] sin2[n] w1[n] w2[n] f32 — the observation, six
// adjacent columns (mgym_observation is a view of them) — th1[n] th2[n] f32 (wrapped by the step, taken as they are by mgym_set_state),
// episode[n] u32 (touched only by reset); elapsed[n] u16 beside them.  One lane owns 4 consecutive environments (16-byte accesses).  Stage 1 of
// the integration reads the four stored trig words instead of reducing the angles again.
// Algorithmic bytes per env-step of mgym_step: 74 (the eight state columns 32 R + 32 W; action 4 R; reward 4 W; done 1 W; truncated 1 W), with a
// time limit + 2 R + 2 W = 78.  A rollout keeps the eight words and the count in registers over its K steps: 10 per env-step.
// This is the one classic family whose step is arithmetic, not traffic: four derivative evaluations with four IEEE divides each and eight f64
// sincos pairs per environment-step.
#include "classic_env.h"
#include "acrobot_step.h"

namespace mgym {

struct AcrobotDev {
    float* obs;          // column k at obs + k * n_pad: cos1 sin1 cos2 sin2 w1 w2 th1 th2
    uint64_t n_pad;
    uint32_t* episode;
    uint64_t n, seed, env_id_base;
    uint32_t* err;
    unsigned long long* done_count;  // kDoneShards partial counts of finished env-steps (mgym_episode_count)
    int auto_reset;
    uint16_t* elapsed;   // caller-visible steps since the env's last reset, saturating at 65535 (padded to n_pad like the state columns)
    uint32_t limit;      // max_episode_steps; 0: off
};

// an environment's eight words in column order, and back
__device__ __forceinline__ AbEnv ab_env(float c1, float s1, float c2, float s2, float w1, float w2, float th1, float th2) {
    AbEnv e; e.c1 = c1; e.s1 = s1; e.c2 = c2; e.s2 = s2; e.w1 = w1; e.w2 = w2; e.th1 = th1; e.th2 = th2;
    return e;
}
__device__ __forceinline__ float ab_word(const AbEnv& e, int col) {
    switch (col) {
    case 0: return e.c1; case 1: return e.s1; case 2: return e.c2; case 3: return e.s2;
    case 4: return e.w1; case 5: return e.w2; case 6: return e.th1; default: return e.th2;
    }
}
__device__ __forceinline__ float4 ab_col4(const AbEnv (&e)[4], int col) { return make_float4(ab_word(e[0], col), ab_word(e[1], col), ab_word(e[2], col), ab_word(e[3], col)); }

// one env of the engine's columns
__device__ __forceinline__ AbEnv ab_load1(const AcrobotDev& d, uint64_t i) {
    const float* p = d.obs + i;
    const uint64_t s = d.n_pad;
    return ab_env(p[0], p[s], p[2 * s], p[3 * s], p[4 * s], p[5 * s], p[6 * s], p[7 * s]);
}
__device__ __forceinline__ void ab_store1(const AcrobotDev& d, uint64_t i, const AbEnv& e) {
#pragma unroll
    for (int c = 0; c < 8; ++c) d.obs[(uint64_t)c * d.n_pad + i] = ab_word(e, c);
}
// a lane's four envs (i0 a multiple of 4): eight 16-byte accesses
__device__ __forceinline__ void ab_load4(const AcrobotDev& d, uint64_t i0, AbEnv (&e)[4]) {
    float4 v[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = *reinterpret_cast<const float4*>(d.obs + (uint64_t)c * d.n_pad + i0);
    e[0] = ab_env(v[0].x, v[1].x, v[2].x, v[3].x, v[4].x, v[5].x, v[6].x, v[7].x);
    e[1] = ab_env(v[0].y, v[1].y, v[2].y, v[3].y, v[4].y, v[5].y, v[6].y, v[7].y);
    e[2] = ab_env(v[0].z, v[1].z, v[2].z, v[3].z, v[4].z, v[5].z, v[6].z, v[7].z);
    e[3] = ab_env(v[0].w, v[1].w, v[2].w, v[3].w, v[4].w, v[5].w, v[6].w, v[7].w);
}
__device__ __forceinline__ void ab_store4(const AcrobotDev& d, uint64_t i0, const AbEnv (&e)[4]) {
#pragma unroll
    for (int c = 0; c < 8; ++c) nt_store4(d.obs + (uint64_t)c * d.n_pad + i0, ab_col4(e, c));
}
// the observation of a lane's four envs into a caller's [6][n] slab
__device__ __forceinline__ void ab_store_obs4(float* o, uint64_t n, const AbEnv (&e)[4]) {
#pragma unroll
    for (int c = 0; c < 6; ++c) nt_store4(o + (uint64_t)c * n, ab_col4(e, c));
}

// the fused reset of env i: the draws of its current episode, episode + 1 (the caller clears its count)
__device__ __forceinline__ void acrobot_reset_env(const AcrobotDev& d, uint64_t i, AbEnv& e) {
    const uint32_t ep = d.episode[i];
    acrobot_reset_one(d.seed, d.env_id_base + i, ep, e);
    d.episode[i] = ep + 1u;
}

// the observation words of a finished env, before its reset, into the channel of mgym_set_final_obs_out
__device__ __forceinline__ void acrobot_final_store(float* fin, uint64_t n, const AbEnv& e) { final_store<6>(fin, n, {e.c1, e.s1, e.c2, e.s2, e.w1, e.w2}); }

// The generic step kernel: any n, any alignment of the caller's buffers (VEC = 1), or 4 environments per lane with a ragged last group (VEC = 4).
// The loop over a lane's environments keeps one environment's integration live at a time (the sched_barrier between them): four in flight do not fit.
// Fin (here and in the kernels below): mgym_set_final_obs_out (soa4.h) — `fin` is the step's [6][n] slab, or the call's [K][6][n] in a rollout.
template <int VEC, bool TL, class... Fin>
__global__ void __launch_bounds__(kBlock)
acrobot_step_kernel(AcrobotDev d, const uint32_t* __restrict__ act, float* __restrict__ obs_out, float* __restrict__ rew, uint8_t* __restrict__ done_out,
                    uint8_t* __restrict__ trunc_out, Fin... fin) {
    const uint64_t groups = (d.n + VEC - 1) / VEC;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    bool bad = false;
    uint32_t finished = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
        const uint64_t i0 = g * VEC;
        AbEnv e[4];
        float r[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        uint32_t a[4] = {1u, 1u, 1u, 1u}, dn[4] = {0u, 0u, 0u, 0u};
        uint32_t el[4] = {0u, 0u, 0u, 0u}, tr[4] = {0u, 0u, 0u, 0u};   // (time limit only)
        const bool full = (VEC == 1) || (i0 + VEC <= d.n);
        if constexpr (TL) {
            if (VEC == 4) load_elapsed4(d.elapsed, i0, el);   // (the column is padded: a ragged last group may load it whole)
            else el[0] = d.elapsed[i0];
        }
        if (VEC == 4) {
            ab_load4(d, i0, e);   // (the columns are padded: a ragged last group may load them whole)
            if (full) {
                const uint4 va = *reinterpret_cast<const uint4*>(act + i0);
                a[0] = va.x; a[1] = va.y; a[2] = va.z; a[3] = va.w;
            } else {
#pragma unroll
                for (int k = 0; k < VEC; ++k)
                    if (i0 + k < d.n) a[k] = act[i0 + k];
            }
        } else {
            e[0] = ab_load1(d, i0);
            a[0] = act[i0];
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const bool in = i0 + k < d.n;
            if (!acrobot_env_step<TL>(d.limit, e[k], el[k], a[k], r[k], dn[k], tr[k])) bad = true;
            const uint32_t f = dn[k] | tr[k];
            finished += (f && in) ? 1u : 0u;
            if (d.auto_reset && f && in) {
                if constexpr (has_final<Fin...>) acrobot_final_store(final_ptr(fin...) + i0 + k, d.n, e[k]);
                acrobot_reset_env(d, i0 + k, e[k]); el[k] = 0u;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (VEC == 4 && full) {
            ab_store4(d, i0, e);
            if (obs_out) ab_store_obs4(obs_out + i0, d.n, e);
            if (rew) nt_store4(rew + i0, make_float4(r[0], r[1], r[2], r[3]));
            if (done_out) __builtin_nontemporal_store(pack_bytes4(dn), reinterpret_cast<uint32_t*>(done_out + i0));
            if (trunc_out) __builtin_nontemporal_store(pack_bytes4(tr), reinterpret_cast<uint32_t*>(trunc_out + i0));
            if constexpr (TL) store_elapsed4(d.elapsed, i0, el);
        } else {
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const uint64_t i = i0 + k;
                if (i < d.n) {
                    ab_store1(d, i, e[k]);
                    if (obs_out) {
#pragma unroll
                        for (int c = 0; c < 6; ++c) obs_out[(uint64_t)c * d.n + i] = ab_word(e[k], c);
                    }
                    if (rew) rew[i] = r[k];
                    if (done_out) done_out[i] = (uint8_t)dn[k];
                    if (trunc_out) trunc_out[i] = (uint8_t)tr[k];
                    if constexpr (TL) d.elapsed[i] = (uint16_t)el[k];
                }
            }
        }
    }
    flush_counts(d.done_count, d.err, finished, bad);
}

// The 16-byte path (caller buffers aligned, n % 4 == 0, n <= 2^26), the form of mountaincar_step4_kernel: one lane owns 4 consecutive
// environments; block-uniform passes; the engine columns through one buffer resource (descriptor and column / pass offsets in SGPRs, one constant
// VGPR lane offset; the farthest column starts 7 n_pad words in, and 28 n_pad + 4 n < 2^32 for n <= 2^26); the columns are padded to n_pad (a
// multiple of the block's 1024 envs), so every lane may load them — only in-range lanes store.  Every load of a pass is issued before the
// sched_barrier.  Finished envs are counted with __ballot + popcount; resets are rare (an episode lasts >= 60 steps) and stay in place.
// ONE: the single-pass form, one block per tile of 1024 environments (populations of at most the block cap's tiles) — no loop, no test on n before the
// loads, no read of the grid size; !ONE: the grid-stride form.  The arguments are plain scalars and pointers in the order the kernel first needs
// them; the leading 14 dwords (obs .. err) can be asked for as preloaded SGPRs (Makefile, PRELOAD).
template <bool RESET, bool TL, bool ONE, class... Fin>
__global__ void __launch_bounds__(kBlock)
acrobot_step4_kernel(float* obs_col, uint32_t n_pad, uint32_t n, const uint32_t* __restrict__ act, uint16_t* elapsed, uint64_t seed, uint64_t env_id_base,
                     uint32_t* err, unsigned long long* done_count, float* __restrict__ obs_out, float* __restrict__ rew, uint8_t* __restrict__ done_out,
                     uint8_t* __restrict__ trunc_out, uint32_t limit, Fin... fin) {
    constexpr uint32_t kPerBlock = (uint32_t)kBlock * 4;
    const uint32_t lane_env = threadIdx.x * 4u, off4 = lane_env * 4u;
    const uint32_t colb = n_pad * 4u;  // column stride in bytes
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(obs_col, 0, 0xffffffff, 0x00020000);
    const AcrobotDev d{obs_col, n_pad, reinterpret_cast<uint32_t*>(obs_col + 8 * (uint64_t)n_pad), n, seed, env_id_base, err, done_count, RESET ? 1 : 0, elapsed, limit};
    bool bad = false;
    uint32_t finished = 0;
    uint32_t base = blockIdx.x * kPerBlock;   // block-uniform
    do {
        const uint32_t sb = base * 4u;
        // every load of the pass first
        u32x4 v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = __builtin_amdgcn_raw_buffer_load_b128(rs, off4, sb + (uint32_t)c * colb, 0);
        uint32_t el[4] = {0u, 0u, 0u, 0u}, tr[4] = {0u, 0u, 0u, 0u};   // (time limit only)
        if constexpr (TL) load_elapsed4(elapsed, base + lane_env, el);   // (padded to n_pad like the state columns: every lane may load)
        const bool in = lane_env < n - base;
        uint4 va = make_uint4(1u, 1u, 1u, 1u);
        if (in) va = *at<uint4>(act + base, off4);
        __builtin_amdgcn_sched_barrier(0);
        AbEnv e[4] = {ab_env(as_f32(v[0].x), as_f32(v[1].x), as_f32(v[2].x), as_f32(v[3].x), as_f32(v[4].x), as_f32(v[5].x), as_f32(v[6].x), as_f32(v[7].x)),
                      ab_env(as_f32(v[0].y), as_f32(v[1].y), as_f32(v[2].y), as_f32(v[3].y), as_f32(v[4].y), as_f32(v[5].y), as_f32(v[6].y), as_f32(v[7].y)),
                      ab_env(as_f32(v[0].z), as_f32(v[1].z), as_f32(v[2].z), as_f32(v[3].z), as_f32(v[4].z), as_f32(v[5].z), as_f32(v[6].z), as_f32(v[7].z)),
                      ab_env(as_f32(v[0].w), as_f32(v[1].w), as_f32(v[2].w), as_f32(v[3].w), as_f32(v[4].w), as_f32(v[5].w), as_f32(v[6].w), as_f32(v[7].w))};
        const uint32_t a[4] = {va.x, va.y, va.z, va.w};
        float r[4];
        uint32_t dn[4], fn[4], any_fin = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!acrobot_env_step<TL>(limit, e[k], el[k], a[k], r[k], dn[k], tr[k])) bad = true;
            fn[k] = dn[k] | tr[k];
            any_fin |= fn[k];
            __builtin_amdgcn_sched_barrier(0);   // one environment's integration live at a time
        }
        const unsigned long long m = __ballot(in && any_fin);
        if (m) {  // rare: count and (RESET) restart the finished envs in place
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                finished += (uint32_t)__popcll(__ballot(in && fn[k]));
                if (RESET && in && fn[k]) {
                    if constexpr (has_final<Fin...>) acrobot_final_store(final_ptr(fin...) + base + lane_env + k, n, e[k]);
                    acrobot_reset_env(d, (uint64_t)base + lane_env + k, e[k]); el[k] = 0u;
                }
            }
        }
        if (in) {
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float4 w = ab_col4(e, c);
                __builtin_amdgcn_raw_buffer_store_b128(u32x4{as_u32(w.x), as_u32(w.y), as_u32(w.z), as_u32(w.w)}, rs, off4, sb + (uint32_t)c * colb, 2);
            }
            if (obs_out) ab_store_obs4(at<float>(obs_out + base, off4), n, e);
            if (rew) nt_store4(at<float>(rew + base, off4), make_float4(r[0], r[1], r[2], r[3]));
            if (done_out) __builtin_nontemporal_store(pack_bytes4(dn), reinterpret_cast<uint32_t*>(done_out + base + lane_env));
            if (trunc_out) __builtin_nontemporal_store(pack_bytes4(tr), reinterpret_cast<uint32_t*>(trunc_out + base + lane_env));
            if constexpr (TL) store_elapsed4(elapsed, base + lane_env, el);
        }
        if constexpr (ONE) break;
        base += gridDim.x * kPerBlock;   // (at most 2^23 envs a stride: no 32-bit wrap below n <= 2^26)
    } while (base < n);
    if ((threadIdx.x & 63) == 0 && finished)
        atomicAdd(done_count + ((blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) & (kDoneShards - 1)), (unsigned long long)finished);
    if (__any(bad)) {
        if ((threadIdx.x & 63) == 0) atomicOr(err, DEV_ERR_INVALID_ACTION);
    }
}

// Fused K-step rollout (mgym_rollout and the policy forms): 4 environments per lane — the eight words of each and the elapsed count — stay in
// registers for K steps; per step one 16-B action word in (TABLE) or out, reward / done / truncated (and optionally the observation) out.  Same
// per-env function and the same in-place auto-reset as the step kernels, hence bit-identical to K separate steps.
// The policies decide from the six observation words held before the step (acrobot_step.h); actions_out holds u32 words.
// (mgym_rollout_mlp2's sources take the address of the handle's pack and its widths at the head of the trailing pack: soa4.h)
template <int POLICY = ROLL_ACT_TABLE, bool TL = false, class... Fin>
__global__ void __launch_bounds__(kBlock)
acrobot_rollout_kernel(AcrobotDev d, const uint32_t* __restrict__ act, int K, float* __restrict__ obs_out, float* __restrict__ rew,
                       uint8_t* __restrict__ done_out, uint8_t* __restrict__ trunc_out, PolicyArg<POLICY, 6, 3, AbLinearPolicy> pol = {}, uint32_t* __restrict__ act_out = nullptr,
                       UniformDraw uni = {}, Fin... fin) {
    static_assert(roll_act_discrete_takes(POLICY), "Acrobot has discrete actions: no Gaussian draw");
    const uint64_t groups = d.n / 4;  // n % 4 == 0 is required by the host wrapper
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    bool bad = false;
    uint32_t finished = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
        const uint64_t i0 = g * 4;
        AbEnv e[4];
        ab_load4(d, i0, e);
        Philox4 bits{};
        uint32_t el[4] = {0u, 0u, 0u, 0u};   // (time limit only: the count lives in registers across the K steps)
        if constexpr (TL) load_elapsed4(d.elapsed, i0, el);
        for (int t = 0; t < K; ++t) {
            const uint64_t off = (uint64_t)t * d.n + i0;
            uint32_t a[4];
            if constexpr (POLICY == ROLL_ACT_UNIFORM) {
                if ((t & 1) == 0) bits = acrobot_uniform_block(uni.seed, uni.call, d.env_id_base + i0, (uint32_t)t);
#pragma unroll
                for (int k = 0; k < 4; ++k) a[k] = acrobot_uniform_action(bits.w[k], (uint32_t)t);
            } else if constexpr (roll_act_is_mlp(POLICY) || roll_act_is_mlp2(POLICY)) {
                // hidden-layer policy of either depth on the six observation words: the argmax, or (SAMPLE) the draw from the scores — one Philox evaluation per
                // lane per step, its four words for the lane's four envs (policy.h: net, activation and head)
                float o[4][6];
#pragma unroll
                for (int k = 0; k < 4; ++k) acrobot_obs(e[k], o[k]);
                Philox4 w;
                policy_draw<POLICY>(uni.seed, d.env_id_base + i0, uni.call, (uint32_t)t, w);
                policy_actions4<POLICY, 6, 3>(pol, w.w, 0.0f, o, a, fin...);
            } else if constexpr (POLICY == ROLL_ACT_LINEAR) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float o[6];
                    acrobot_obs(e[k], o);
                    a[k] = acrobot_linear_action(pol, o);
                }
            } else {
                const u32x4 va = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(act + off));
                a[0] = va.x; a[1] = va.y; a[2] = va.z; a[3] = va.w;
            }
            if constexpr (POLICY != ROLL_ACT_TABLE) {
                if (act_out) __builtin_nontemporal_store(u32x4{a[0], a[1], a[2], a[3]}, reinterpret_cast<u32x4*>(act_out + off));
            }
            float r[4];
            uint32_t dn[4], tr[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!acrobot_env_step<TL>(d.limit, e[k], el[k], a[k], r[k], dn[k], tr[k])) bad = true;
                const uint32_t f = dn[k] | tr[k];
                finished += f;
                if (d.auto_reset && f) {
                    if constexpr (has_final<Fin...>) acrobot_final_store(final_ptr(fin...) + (uint64_t)t * 6 * d.n + i0 + k, d.n, e[k]);
                    acrobot_reset_env(d, i0 + k, e[k]); el[k] = 0u;
                }
                __builtin_amdgcn_sched_barrier(0);   // one environment's integration live at a time
            }
            if (rew) nt_store4(rew + off, make_float4(r[0], r[1], r[2], r[3]));
            if (done_out) __builtin_nontemporal_store(pack_bytes4(dn), reinterpret_cast<uint32_t*>(done_out + off));
            if (trunc_out) __builtin_nontemporal_store(pack_bytes4(tr), reinterpret_cast<uint32_t*>(trunc_out + off));
            if (obs_out) ab_store_obs4(obs_out + (uint64_t)t * 6 * d.n + i0, d.n, e);
        }
        ab_store4(d, i0, e);
        if constexpr (TL) store_elapsed4(d.elapsed, i0, el);
    }
    flush_counts(d.done_count, d.err, finished, bad);
}

__global__ void __launch_bounds__(kBlock)
acrobot_reset_kernel(AcrobotDev d, const uint8_t* __restrict__ m0, const uint8_t* __restrict__ m1, int all, int masks_aligned, float* __restrict__ obs_out) {
    const uint64_t groups = (d.n + 3) / 4;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
        const uint64_t i0 = g * 4;
        const uint32_t m = reset_mask4(m0, m1, all, masks_aligned, i0, d.n);
        if (m == 0) continue;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint64_t i = i0 + k;
            if (i < d.n && ((m >> (8 * k)) & 0xffu)) {
                AbEnv e;
                acrobot_reset_env(d, i, e);
                ab_store1(d, i, e);
                d.elapsed[i] = 0;
                if (obs_out) {
#pragma unroll
                    for (int c = 0; c < 6; ++c) obs_out[(uint64_t)c * d.n + i] = ab_word(e, c);
                }
            }
        }
    }
}

// mgym_reset_deterministic: every state word 0 -> the observation (1, 0, 1, 0, 0, 0); the episode number stays
__global__ void acrobot_zero_kernel(AcrobotDev d, float* __restrict__ obs_out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.n) return;
    const AbEnv e = ab_env(1.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f);
    ab_store1(d, i, e);
    d.elapsed[i] = 0;
    if (obs_out) {
#pragma unroll
        for (int c = 0; c < 6; ++c) obs_out[(uint64_t)c * d.n + i] = ab_word(e, c);
    }
}

// state blob: th1, th2, w1, w2, episode
__global__ void acrobot_export_kernel(AcrobotDev d, uint32_t* __restrict__ blob) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.n) return;
    const AbEnv e = ab_load1(d, i);
    blob[i] = as_u32(e.th1);
    blob[d.n + i] = as_u32(e.th2);
    blob[2 * d.n + i] = as_u32(e.w1);
    blob[3 * d.n + i] = as_u32(e.w2);
    blob[4 * d.n + i] = d.episode[i];
}

__global__ void acrobot_import_kernel(AcrobotDev d, const uint32_t* __restrict__ blob) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.n) return;
    AbEnv e;
    e.th1 = as_f32(blob[i]); e.th2 = as_f32(blob[d.n + i]); e.w1 = as_f32(blob[2 * d.n + i]); e.w2 = as_f32(blob[3 * d.n + i]);   // as they are: no wrap, no clamp
    acrobot_trig(e);   // the stored trig words are those of the imported angle words
    ab_store1(d, i, e);
    d.episode[i] = blob[4 * d.n + i];
    d.elapsed[i] = 0;   // an imported state starts its count at 0 (mgym_set_elapsed_steps overrides)
}

struct AcrobotEnv final : ClassicEnv {
    AcrobotDev dev{};

    int init() override {
        obs_dim = 6;
        state_cols = 5;
        if (const int st = alloc(9)) return st;
        float* f = cols;
        MGYM_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(f), 0x3f800000, n_pad, stream));               // th1 = 0: cos = 1
        MGYM_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(f + 2 * n_pad), 0x3f800000, n_pad, stream));   // th2 = 0: cos = 1
        dev.obs = f; dev.n_pad = n_pad;
        dev.episode = reinterpret_cast<uint32_t*>(f + 8 * n_pad);
        fill_common(dev);
        step4_max = 1ull << 26;   // (acrobot_step4_kernel's 32-bit offsets reach 7 columns in)
        return MGYM_OK;
    }

    int reset(const uint8_t* m0, const uint8_t* m1, bool all, float* obs_out) override { return launch_reset(acrobot_reset_kernel, dev, m0, m1, all, obs_out); }
    int reset_deterministic(float* obs_out) override { return launch_per_env(acrobot_zero_kernel, dev, obs_out); }

    int step(const void* actions, float* obs_out, float* reward, uint8_t* done, uint8_t* trunc) override {
        const uint32_t* act = static_cast<const uint32_t*>(actions);
        return launch_step(act, obs_out, reward, done, trunc,
            [&](dim3 g, auto R, auto T, auto O, auto... fin) {
                hipLaunchKernelGGL((acrobot_step4_kernel<decltype(R)::value, decltype(T)::value, decltype(O)::value, decltype(fin)...>), g, dim3(kBlock), 0, stream, dev.obs, (uint32_t)n_pad, (uint32_t)n,
                                   act, dev.elapsed, dev.seed, dev.env_id_base, dev.err, dev.done_count, obs_out, reward, done, trunc, dev.limit, fin...);
            },
            [&](dim3 g, auto V, auto T, auto... fin) {
                hipLaunchKernelGGL((acrobot_step_kernel<decltype(V)::value ? 4 : 1, decltype(T)::value, decltype(fin)...>), g, dim3(kBlock), 0, stream, dev, act, obs_out, reward, done, trunc, fin...);
            });
    }

    // the one launch of the fused rollout kernel with the action source POLICY; `arg`: the linear words or the hidden-layer pack, `uni`: the uniform stream, or the
    // categorical draw's seed and call word; `net`: a two-hidden-layer source's Mlp2Net, the head of the kernel's trailing pack
    template <int POLICY, class... Net>
    void launch_rollout(const uint32_t* act, uint32_t* act_out, int K, float* obs_out, float* reward, uint8_t* done, uint8_t* trunc, const PolicyArg<POLICY, 6, 3, AbLinearPolicy>& arg, UniformDraw uni,
                        Net... net) {
        with_bools([&](auto T) {
            constexpr bool TL = decltype(T)::value;
            if (final_obs) hipLaunchKernelGGL((acrobot_rollout_kernel<POLICY, TL, Net..., float*>), dim3(grid_for(n / 4)), dim3(kBlock), 0, stream, dev, act, K, obs_out, reward, done, trunc, arg, act_out, uni, net..., final_obs);
            else hipLaunchKernelGGL((acrobot_rollout_kernel<POLICY, TL, Net...>), dim3(grid_for(n / 4)), dim3(kBlock), 0, stream, dev, act, K, obs_out, reward, done, trunc, arg, act_out, uni, net...);
        }, dev.limit != 0u);
    }

    void rollout_table(const uint32_t* act, int K, float* obs_out, float* reward, uint8_t* done, uint8_t* trunc) override {
        launch_rollout<ROLL_ACT_TABLE>(act, nullptr, K, obs_out, reward, done, trunc, AbLinearPolicy{}, UniformDraw{});
    }

    int rollout_policy(const PolicyCall& call, int K, void* actions_out, float* obs_out, float* reward, uint8_t* done, uint8_t* trunc) override {
        const char* refusal = roll_act_gauss(call.source) ? ": Acrobot has discrete actions: use mgym_rollout_mlp_sample" : nullptr;   // (the C ABI refuses it first)
        return rollout_policy_classic<6, 3, roll_act_discrete_takes>(call, K, actions_out, obs_out, reward, done, trunc, false, refusal,
            [](const float* w) {   // weights: 3 rows of (6 weights, bias)
                AbLinearPolicy lin{};
                for (int j = 0; j < 3; ++j) {
                    for (int q = 0; q < 6; ++q) lin.w[j][q] = w[7 * j + q];
                    lin.b[j] = w[7 * j + 6];
                }
                return lin;
            },
            [&](auto S, const auto& arg, auto... draw_net) { launch_rollout<decltype(S)::value>(nullptr, static_cast<uint32_t*>(actions_out), K, obs_out, reward, done, trunc, arg, draw_net...); });
    }

    int get_state(void* blob) override { return launch_per_env(acrobot_export_kernel, dev, static_cast<uint32_t*>(blob)); }
    int set_state(const void* blob) override { return launch_per_env(acrobot_import_kernel, dev, static_cast<const uint32_t*>(blob)); }
};

Env* make_acrobot() { return new AcrobotEnv(); }

}  // namespace mgym
