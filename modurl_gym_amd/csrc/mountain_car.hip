// mountain_car.hip — MountainCarV0 (discrete) and MountainCarContinuous-v0 step()/reset()
// as struct-of-arrays gfx950 kernels.
//
// MountainCarV0 replaces `impl Gym for MountainCarV0` (reference
// src/classic_control/mountain_car.rs: reset :279-291, step :293-330).
// MountainCarContinuous-v0 is NOT in the reference (BASELINE config 3 asks for it):
// gymnasium semantics, parity unpinned; it shares everything but the action decoding,
// goal position and reward.
//
// Data layout in HBM (engine-owned): position[n] velocity[n] f32 (the observation),
// episode[n] u32 (touched only by reset).  One lane owns 4 consecutive environments
// (16-byte accesses).  Algorithmic bytes per env-step: 26 (state 8 R + 8 W, action 4 R,
// reward 4 W, done 1 W, truncated 1 W).
// Episode time limit (mgym_config::max_episode_steps, not in the reference — time_limit.h): elapsed[n] u16, one lane's 4 environments in ONE
// 8-byte access, read and written by the time-limited instantiations only (TL = true: mgym_step 26 + 2 R + 2 W = 30 B per env-step; a rollout
// keeps the count in registers, one read and one write per launch).  A handle without a limit launches the TL = false instantiations, which
// are the kernels as they were: the count is then left alone (0 after a reset, not advanced).
#include "classic_env.h"
#include "mgym_math.h"
#include "mlp_policy.h"
#include "philox.h"
#include "time_limit.h"

namespace mgym {

struct MountainCarParams {
    float min_position, max_position, max_speed, goal_position, goal_velocity;
    float force, gravity;  // discrete: 0.001, 0.0025; continuous: power 0.0015 in `force`
};

// mountain_car.rs:35-40; the family (discrete / continuous) fixes everything but goal_velocity
__host__ __device__ constexpr MountainCarParams mc_params(bool continuous, float goal_velocity) {
    return MountainCarParams{-1.2f, 0.6f, 0.07f, continuous ? 0.45f : 0.5f, goal_velocity, continuous ? 0.0015f : 0.001f, 0.0025f};
}

struct MountainCarDev {
    float *pos, *vel;
    uint32_t* episode;
    uint64_t n, seed, env_id_base;
    uint32_t* err;
    unsigned long long* done_count;  // kDoneShards partial counts of finished env-steps (mgym_episode_count)
    MountainCarParams p;
    int auto_reset;
    uint16_t* elapsed;   // caller-visible steps since the env's last reset, saturating at 65535 (padded to n_pad like the state columns)
    uint32_t limit;      // max_episode_steps; 0: off
};

// f32::clamp: if self < min {min} else if self > max {max} else {self}
__device__ __forceinline__ float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// reset(): mountain_car.rs:279-291 — position ~ U[-0.6,-0.4) sampled f64 -> f32, velocity 0
__device__ __forceinline__ void mountaincar_reset_one(const MountainCarDev& d, uint64_t i, float& pos, float& vel) {
    uint32_t ep = d.episode[i];
    Philox4 a = env_draw(d.seed, d.env_id_base + i, ep, SLOT_RESET0);
    pos = uniform_f64_to_f32(-0.6, -0.4, a.w[0], a.w[1]);
    vel = 0.0f;
    d.episode[i] = ep + 1u;
}

template <bool CONT>
__device__ __forceinline__ void mountaincar_step_one(const MountainCarParams& p, float& position, float& velocity,
                                                     uint32_t action_bits, float& reward, uint32_t& done, bool& bad) {
    float push;  // the action-dependent velocity increment
    float a_f = 0.0f;
    if (CONT) {
        a_f = as_f32(action_bits);
        if (a_f != a_f) { bad = true; reward = 0.0f; done = 0u; return; }
        float force = clampf(a_f, -1.0f, 1.0f);
        push = force * p.force;
    } else {
        if (action_bits >= 3u) { bad = true; reward = 0.0f; done = 0u; return; }  // :294
        push = ((float)action_bits - 1.0f) * p.force;                               // :301
    }
    velocity += push + mg_cosf_u(3.0f * position) * (-p.gravity);                     // :301-302
    velocity = clampf(velocity, -p.max_speed, p.max_speed);                         // :304
    position += velocity;                                                           // :306
    position = clampf(position, p.min_position, p.max_position);                    // :308
    if (position == p.min_position && velocity < 0.0f) velocity = 0.0f;             // :311-313
    bool terminated = position >= p.goal_position && velocity >= p.goal_velocity;   // :318
    done = terminated ? 1u : 0u;
    if (CONT) {
        float r = 0.0f;
        if (terminated) r = 100.0f;
        r -= a_f * a_f * 0.1f;
        reward = r;
    } else {
        reward = -1.0f;  // :319
    }
}

// Fin (here and in the kernels below): mgym_set_final_obs_out (soa4.h) — `fin` is the step's [2][n] slab, or the call's [K][2][n] in a rollout.
template <int VEC, bool CONT, bool TL = false, class... Fin>
__global__ void __launch_bounds__(kBlock)
mountaincar_step_kernel(MountainCarDev d, const uint32_t* __restrict__ act, float* __restrict__ obs_out,
                        float* __restrict__ rew, uint8_t* __restrict__ done_out, uint8_t* __restrict__ trunc_out, Fin... fin_out) {
    const uint64_t groups = (d.n + VEC - 1) / VEC;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    bool bad = false;
    uint32_t finished = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
        const uint64_t i0 = g * VEC;
        float ps[VEC], vs[VEC], r[VEC];
        uint32_t a[VEC], dn[VEC];
        uint32_t el[4] = {0u, 0u, 0u, 0u}, tr[4] = {0u, 0u, 0u, 0u};   // (time limit only)
        const bool full = (VEC == 1) || (i0 + VEC <= d.n);
        if constexpr (TL) {
            if (VEC == 4) load_elapsed4(d.elapsed, i0, el);   // (the column is padded: a ragged last group may load it whole)
            else el[0] = d.elapsed[i0];
        }
        if (VEC == 4 && full) {
            float4 vp = *reinterpret_cast<const float4*>(d.pos + i0);
            float4 vv = *reinterpret_cast<const float4*>(d.vel + i0);
            uint4 va = *reinterpret_cast<const uint4*>(act + i0);
            ps[0] = vp.x; ps[1 % VEC] = vp.y; ps[2 % VEC] = vp.z; ps[3 % VEC] = vp.w;
            vs[0] = vv.x; vs[1 % VEC] = vv.y; vs[2 % VEC] = vv.z; vs[3 % VEC] = vv.w;
            a[0] = va.x; a[1 % VEC] = va.y; a[2 % VEC] = va.z; a[3 % VEC] = va.w;
        } else {
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                uint64_t i = i0 + k;
                bool in = i < d.n;
                ps[k] = in ? d.pos[i] : 0.0f;
                vs[k] = in ? d.vel[i] : 0.0f;
                a[k] = in ? act[i] : (CONT ? 0u : 1u);
            }
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            mountaincar_step_one<CONT>(d.p, ps[k], vs[k], a[k], r[k], dn[k], bad);
            uint32_t fin = dn[k];
            if constexpr (TL) { el[k] = tl_advance(el[k]); tr[k] = tl_truncated(d.limit, el[k]); fin |= tr[k]; }
            finished += (fin && (i0 + k < d.n)) ? 1u : 0u;
            if (d.auto_reset && fin && (i0 + k < d.n)) {
                if constexpr (has_final<Fin...>) final_store<2>(final_ptr(fin_out...) + i0 + k, d.n, {ps[k], vs[k]});
                mountaincar_reset_one(d, i0 + k, ps[k], vs[k]); if constexpr (TL) el[k] = 0u;
            }
        }
        if (VEC == 4 && full) {
            float4 op = make_float4(ps[0], ps[1 % VEC], ps[2 % VEC], ps[3 % VEC]);
            float4 ov = make_float4(vs[0], vs[1 % VEC], vs[2 % VEC], vs[3 % VEC]);
            // non-temporal output stores (measured on the CartPole kernel: ~5 % at 1 Mi envs)
            nt_store4(d.pos + i0, op);
            nt_store4(d.vel + i0, ov);
            if (obs_out) {
                nt_store4(obs_out + i0, op);
                nt_store4(obs_out + d.n + i0, ov);
            }
            if (rew) nt_store4(rew + i0, make_float4(r[0], r[1 % VEC], r[2 % VEC], r[3 % VEC]));
            if (done_out) {
                const uint32_t dn4[4] = {dn[0], dn[1 % VEC], dn[2 % VEC], dn[3 % VEC]};
                __builtin_nontemporal_store(pack_bytes4(dn4), reinterpret_cast<uint32_t*>(done_out + i0));
            }
            if (trunc_out) __builtin_nontemporal_store(pack_bytes4(tr), reinterpret_cast<uint32_t*>(trunc_out + i0));  // :328 truncated: false, always (TL: the time limit)
            if constexpr (TL) store_elapsed4(d.elapsed, i0, el);
        } else {
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                uint64_t i = i0 + k;
                if (i < d.n) {
                    d.pos[i] = ps[k]; d.vel[i] = vs[k];
                    if (obs_out) { obs_out[i] = ps[k]; obs_out[d.n + i] = vs[k]; }
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

// The 16-byte path (caller buffers aligned, n % 4 == 0): one lane owns 4 consecutive environments; block-uniform passes;
// engine columns through one buffer resource (descriptor and column / pass offsets in SGPRs, one constant VGPR lane
// offset: no per-lane address arithmetic; n <= 2^27 so every byte offset fits 32 bits); the columns are padded to n_pad
// (a multiple of the block's 1024 envs), so every lane may load them — only in-range lanes store.  The done mask is
// reduced with __ballot + popcount for mgym_episode_count; resets are rare here (episodes last >= 100 steps) and stay
// in place.
// ONE: the single-pass form — the host launched one block per tile of 1024 environments (every population of at most the block cap's tiles), so
// the instantiation has no loop, no test on n before its loads and no read of the grid size; !ONE: the grid-stride form of larger populations
// (no more blocks than tiles, so a block's first pass needs no test either).  The arguments are plain scalars and pointers in the order the
// kernel first needs them — what the loads need (pos, n_pad, n, actions, the elapsed column), then the rest; the leading 14 dwords (pos .. err)
// can be asked for as preloaded SGPRs (Makefile, PRELOAD).  MountainCarDev is rebuilt from them for mountaincar_step_one / mountaincar_reset_one: the
// columns lie n_pad words apart, and the physics constants depend on the family alone (mc_params), all but goal_velocity.
template <bool CONT, bool RESET, bool TL, bool ONE, class... Fin>
__global__ void __launch_bounds__(kBlock)
mountaincar_step4_kernel(float* pos, uint32_t n_pad, uint32_t n, const uint32_t* __restrict__ act, uint16_t* elapsed, uint64_t seed, uint64_t env_id_base,
                         uint32_t* err, unsigned long long* done_count, float* __restrict__ obs_out, float* __restrict__ rew, uint8_t* __restrict__ done_out,
                         uint8_t* __restrict__ trunc_out, uint32_t limit, float goal_velocity, Fin... fin_out) {
    constexpr uint32_t kPerBlock = (uint32_t)kBlock * 4;
    const uint32_t lane_env = threadIdx.x * 4u, off4 = lane_env * 4u;
    const uint32_t colb = n_pad * 4u;  // column stride in bytes
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(pos, 0, 0xffffffff, 0x00020000);
    const MountainCarDev d{pos, pos + n_pad, reinterpret_cast<uint32_t*>(pos + 2 * (uint64_t)n_pad), n, seed, env_id_base, err, done_count,
                           mc_params(CONT, goal_velocity), RESET ? 1 : 0, elapsed, limit};
    bool bad = false;
    uint32_t finished = 0;
    uint32_t base = blockIdx.x * kPerBlock;   // block-uniform
    do {
        const uint32_t sb = base * 4u;
        // every load of the pass first
        const u32x4 vp = __builtin_amdgcn_raw_buffer_load_b128(rs, off4, sb, 0);
        const u32x4 vv = __builtin_amdgcn_raw_buffer_load_b128(rs, off4, sb + colb, 0);
        uint32_t el[4] = {0u, 0u, 0u, 0u}, tr[4] = {0u, 0u, 0u, 0u}, fin[4];   // (el / tr: time limit only)
        if constexpr (TL) load_elapsed4(d.elapsed, base + lane_env, el);            // (padded to n_pad like the state columns: every lane may load)
        const bool in = lane_env < n - base;
        uint4 va = CONT ? make_uint4(0u, 0u, 0u, 0u) : make_uint4(1u, 1u, 1u, 1u);
        if (in) va = *at<uint4>(act + base, off4);
        __builtin_amdgcn_sched_barrier(0);
        float ps[4] = {as_f32(vp.x), as_f32(vp.y), as_f32(vp.z), as_f32(vp.w)}, vs[4] = {as_f32(vv.x), as_f32(vv.y), as_f32(vv.z), as_f32(vv.w)}, r[4];
        uint32_t a[4] = {va.x, va.y, va.z, va.w}, dn[4];
        uint32_t any_done = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            mountaincar_step_one<CONT>(d.p, ps[k], vs[k], a[k], r[k], dn[k], bad);
            fin[k] = dn[k];
            if constexpr (TL) { el[k] = tl_advance(el[k]); tr[k] = tl_truncated(d.limit, el[k]); fin[k] |= tr[k]; }
            any_done |= fin[k];
        }
        const unsigned long long m = __ballot(in && any_done);
        if (m) {  // rare: count and (RESET) restart the finished envs in place
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                finished += (uint32_t)__popcll(__ballot(in && fin[k]));
                if (RESET && in && fin[k]) {
                    if constexpr (has_final<Fin...>) final_store<2>(final_ptr(fin_out...) + base + lane_env + k, n, {ps[k], vs[k]});
                    mountaincar_reset_one(d, (uint64_t)base + lane_env + k, ps[k], vs[k]); if constexpr (TL) el[k] = 0u;
                }
            }
        }
        if (in) {
            __builtin_amdgcn_raw_buffer_store_b128(u32x4{as_u32(ps[0]), as_u32(ps[1]), as_u32(ps[2]), as_u32(ps[3])}, rs, off4, sb, 2);
            __builtin_amdgcn_raw_buffer_store_b128(u32x4{as_u32(vs[0]), as_u32(vs[1]), as_u32(vs[2]), as_u32(vs[3])}, rs, off4, sb + colb, 2);
            if (obs_out) {
                float* o = at<float>(obs_out + base, off4);
                nt_store4(o, make_float4(ps[0], ps[1], ps[2], ps[3]));
                nt_store4(o + d.n, make_float4(vs[0], vs[1], vs[2], vs[3]));
            }
            if (rew) nt_store4(at<float>(rew + base, off4), make_float4(r[0], r[1], r[2], r[3]));
            if (done_out) __builtin_nontemporal_store(pack_bytes4(dn), reinterpret_cast<uint32_t*>(done_out + base + lane_env));
            if (trunc_out) __builtin_nontemporal_store(pack_bytes4(tr), reinterpret_cast<uint32_t*>(trunc_out + base + lane_env));  // :328 truncated: false, always (TL: the time limit)
            if constexpr (TL) store_elapsed4(d.elapsed, base + lane_env, el);
        }
        if constexpr (ONE) break;
        base += gridDim.x * kPerBlock;   // (at most 2^23 envs a stride: no 32-bit wrap below n <= 2^27)
    } while (base < n);
    if ((threadIdx.x & 63) == 0 && finished)
        atomicAdd(d.done_count + ((blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) & (kDoneShards - 1)), (unsigned long long)finished);
    if (__any(bad)) {
        if ((threadIdx.x & 63) == 0) atomicOr(d.err, DEV_ERR_INVALID_ACTION);
    }
}

// Fused K-step rollout (mgym_rollout): 4 environments per lane stay in registers for K steps; per step one 16-B
// action word in, reward / done / truncated (and optionally the observation) out.  Same per-env function and the
// same in-place auto-reset as mountaincar_step_kernel<4, CONT>, hence bit-identical to K separate steps.
// mgym_rollout_linear: the action comes from the observation the env holds before the step instead of a table.  Discrete(3): the index of the largest of
// the three scores s_j = (w[j][0] * position + w[j][1] * velocity) + b[j] (the first of equal ones); Box(-1, 1): the one score itself as the force (the
// step clamps it like any action).  f32, in that order, nothing fused.
struct McLinearPolicy { float w[3][2], b[3]; };
// mgym_rollout_uniform (UniformDraw, policy.h): the lane's four envs (global ids g .. g + 3, g a multiple of 4) share one Philox stream keyed by the policy seed, counter =
// (g, number of earlier mgym_rollout_uniform calls on this handle, SLOT_POLICY + block).  Discrete(3): step t takes, for env g + k, half (t % 2) of word k
// of block t / 2 (low half first), h, and the action (3 h) >> 16 — each action within 2^-16 of 1/3.  Box(-1, 1): word k of block t, top 24 bits u:
// the force u 2^-23 - 1, uniform over the multiples of 2^-23 in [-1, 1).
// mgym_rollout_mlp: the weight pack of mlp_policy.h (A = 3 scores, or the one force of MountainCarContinuous) takes the place of the linear words in the
// kernel's arguments; the other policies' instantiations keep the arguments they had
// (PolicyArg, policy.h; mgym_rollout_mlp2's sources take the address of the handle's pack, its widths and sigma at the head of the trailing pack: soa4.h)
// mgym_rollout_mlp_gauss (MountainCarContinuous only): sigma, the policy seed and the call word travel beside the pack, in the place of the uniform stream (DrawArg)
template <bool CONT, int POLICY = ROLL_ACT_TABLE, bool TL = false, class... Fin>
__global__ void __launch_bounds__(kBlock)
mountaincar_rollout_kernel(MountainCarDev d, const uint32_t* __restrict__ act, int K, float* __restrict__ obs_out, float* __restrict__ rew,
                           uint8_t* __restrict__ done_out, uint8_t* __restrict__ trunc_out, PolicyArg<POLICY, 2, CONT ? 1 : 3, McLinearPolicy> lin = {}, uint32_t* __restrict__ act_out = nullptr,
                           DrawArg<POLICY> uni = {}, Fin... fin_out) {
    constexpr bool LINEAR = POLICY == ROLL_ACT_LINEAR;
    const uint64_t groups = d.n / 4;  // n % 4 == 0 is required by the host wrapper
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    bool bad = false;
    uint32_t finished = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
        const uint64_t i0 = g * 4;
        float4 vp = *reinterpret_cast<const float4*>(d.pos + i0), vv = *reinterpret_cast<const float4*>(d.vel + i0);
        float ps[4] = {vp.x, vp.y, vp.z, vp.w}, vs[4] = {vv.x, vv.y, vv.z, vv.w};
        Philox4 bits{};
        uint32_t el[4] = {0u, 0u, 0u, 0u};   // (time limit only: the count lives in registers across the K steps)
        if constexpr (TL) load_elapsed4(d.elapsed, i0, el);
        for (int t = 0; t < K; ++t) {
            const uint64_t off = (uint64_t)t * d.n + i0;
            uint32_t a[4], dn[4];
            if constexpr (POLICY == ROLL_ACT_UNIFORM) {
                const uint64_t gid = d.env_id_base + i0;
                if (CONT || (t & 1) == 0)
                    bits = philox4x32_10((uint32_t)gid, (uint32_t)(gid >> 32), uni.call, SLOT_POLICY + (uint32_t)(CONT ? t : t >> 1), (uint32_t)uni.seed, (uint32_t)(uni.seed >> 32));
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if constexpr (CONT) a[k] = __float_as_uint((float)(bits.w[k] >> 8) * 1.1920928955078125e-07f - 1.0f);
                    else a[k] = ((((t & 1) ? bits.w[k] >> 16 : bits.w[k] & 0xffffu)) * 3u) >> 16;
                }
            } else if constexpr (roll_act_is_mlp(POLICY) || roll_act_is_mlp2(POLICY)) {
                // hidden-layer policy of either depth on (position, velocity) of the lane's four envs before the step (policy.h: net, activation, head and draw)
                static_assert(CONT ? roll_act_box_takes(POLICY) : roll_act_discrete_takes(POLICY), "the heads a family has");
                const float o[4][2] = {{ps[0], vs[0]}, {ps[1], vs[1]}, {ps[2], vs[2]}, {ps[3], vs[3]}};
                Philox4 w;
                policy_draw<POLICY>(uni.seed, d.env_id_base + i0, uni.call, (uint32_t)t, w);
                policy_actions4<POLICY, 2, CONT ? 1 : 3>(lin, w.w, draw_sigma(uni), o, a, fin_out...);
            } else if constexpr (LINEAR) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float s0 = (lin.w[0][0] * ps[k] + lin.w[0][1] * vs[k]) + lin.b[0];
                    if constexpr (CONT) a[k] = __float_as_uint(s0);
                    else {
                        const float s1 = (lin.w[1][0] * ps[k] + lin.w[1][1] * vs[k]) + lin.b[1], s2 = (lin.w[2][0] * ps[k] + lin.w[2][1] * vs[k]) + lin.b[2];
                        uint32_t best = s1 > s0 ? 1u : 0u;
                        const float sb = s1 > s0 ? s1 : s0;
                        a[k] = s2 > sb ? 2u : best;
                    }
                }
            } else {
                u32x4 va = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(act + off));
                a[0] = va.x; a[1] = va.y; a[2] = va.z; a[3] = va.w;
            }
            if constexpr (POLICY != ROLL_ACT_TABLE) {
                if (act_out) __builtin_nontemporal_store(u32x4{a[0], a[1], a[2], a[3]}, reinterpret_cast<u32x4*>(act_out + off));
            }
            float r[4];
            uint32_t tr[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                mountaincar_step_one<CONT>(d.p, ps[k], vs[k], a[k], r[k], dn[k], bad);
                uint32_t fin = dn[k];
                if constexpr (TL) { el[k] = tl_advance(el[k]); tr[k] = tl_truncated(d.limit, el[k]); fin |= tr[k]; }
                finished += fin;
                if (d.auto_reset && fin) {
                    if constexpr (has_final<Fin...>) final_store<2>(final_ptr(fin_out...) + (uint64_t)t * 2 * d.n + i0 + k, d.n, {ps[k], vs[k]});
                    mountaincar_reset_one(d, i0 + k, ps[k], vs[k]); if constexpr (TL) el[k] = 0u;
                }
            }
            if (rew) nt_store4(rew + off, make_float4(r[0], r[1], r[2], r[3]));
            if (done_out) __builtin_nontemporal_store(pack_bytes4(dn), reinterpret_cast<uint32_t*>(done_out + off));
            if (trunc_out) __builtin_nontemporal_store(pack_bytes4(tr), reinterpret_cast<uint32_t*>(trunc_out + off));
            if (obs_out) {
                float* o = obs_out + (uint64_t)t * 2 * d.n + i0;
                nt_store4(o, make_float4(ps[0], ps[1], ps[2], ps[3]));
                nt_store4(o + d.n, make_float4(vs[0], vs[1], vs[2], vs[3]));
            }
        }
        nt_store4(d.pos + i0, make_float4(ps[0], ps[1], ps[2], ps[3]));
        nt_store4(d.vel + i0, make_float4(vs[0], vs[1], vs[2], vs[3]));
        if constexpr (TL) store_elapsed4(d.elapsed, i0, el);
    }
    flush_counts(d.done_count, d.err, finished, bad);
}

__global__ void __launch_bounds__(kBlock)
mountaincar_reset_kernel(MountainCarDev d, const uint8_t* __restrict__ m0, const uint8_t* __restrict__ m1, int all,
                         int masks_aligned, float* __restrict__ obs_out) {
    const uint64_t groups = (d.n + 3) / 4;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
        const uint64_t i0 = g * 4;
        const uint32_t m = reset_mask4(m0, m1, all, masks_aligned, i0, d.n);
        if (m == 0) continue;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint64_t i = i0 + k;
            if (i < d.n && ((m >> (8 * k)) & 0xffu)) {
                float p, v;
                mountaincar_reset_one(d, i, p, v);
                d.pos[i] = p; d.vel[i] = v;
                d.elapsed[i] = 0;
                if (obs_out) { obs_out[i] = p; obs_out[d.n + i] = v; }
            }
        }
    }
}

__global__ void mountaincar_export_kernel(MountainCarDev d, uint32_t* __restrict__ blob) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.n) return;
    blob[i] = as_u32(d.pos[i]);
    blob[d.n + i] = as_u32(d.vel[i]);
    blob[2 * d.n + i] = d.episode[i];
}

__global__ void mountaincar_import_kernel(MountainCarDev d, const uint32_t* __restrict__ blob) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.n) return;
    d.pos[i] = as_f32(blob[i]);
    d.vel[i] = as_f32(blob[d.n + i]);
    d.episode[i] = blob[2 * d.n + i];
    d.elapsed[i] = 0;   // the blob stays 3 columns: an imported state starts its count at 0 (mgym_set_elapsed_steps overrides)
}

struct MountainCarEnv final : ClassicEnv {
    bool continuous;
    MountainCarDev dev{};

    explicit MountainCarEnv(bool c) : continuous(c) {}

    int init() override {
        obs_dim = 2;
        state_cols = 3;
        if (const int st = alloc(3)) return st;  // mountain_car.rs:51 zeros
        dev.pos = cols; dev.vel = cols + n_pad;
        dev.episode = reinterpret_cast<uint32_t*>(cols + 2 * n_pad);
        fill_common(dev);
        dev.p = mc_params(continuous, cfg.goal_velocity);
        return MGYM_OK;
    }

    int reset(const uint8_t* m0, const uint8_t* m1, bool all, float* obs_out) override { return launch_reset(mountaincar_reset_kernel, dev, m0, m1, all, obs_out); }

    int reset_deterministic(float* obs_out) override {  // mountain_car.rs:403-408: state = zeros (no reset())
        if (n == 0) return MGYM_OK;
        MGYM_HIP(hipMemsetAsync(dev.pos, 0, 2 * n_pad * sizeof(float), stream));
        MGYM_HIP(hipMemsetAsync(dev.elapsed, 0, n_pad * sizeof(uint16_t), stream));
        if (obs_out) MGYM_HIP(hipMemsetAsync(obs_out, 0, 2 * n * sizeof(float), stream));
        return MGYM_OK;
    }

    int step(const void* actions, float* obs_out, float* reward, uint8_t* done, uint8_t* trunc) override {
        const uint32_t* act = static_cast<const uint32_t*>(actions);
        int st = MGYM_OK;
        with_bools([&](auto C) {
            constexpr bool CONT = decltype(C)::value;
            st = launch_step(act, obs_out, reward, done, trunc,
                [&](dim3 g, auto R, auto T, auto O, auto... fin) {
                    hipLaunchKernelGGL((mountaincar_step4_kernel<CONT, decltype(R)::value, decltype(T)::value, decltype(O)::value, decltype(fin)...>), g, dim3(kBlock), 0, stream, dev.pos, (uint32_t)n_pad,
                                       (uint32_t)n, act, dev.elapsed, dev.seed, dev.env_id_base, dev.err, dev.done_count, obs_out, reward, done, trunc, dev.limit, dev.p.goal_velocity, fin...);
                },
                [&](dim3 g, auto V, auto T, auto... fin) {
                    hipLaunchKernelGGL((mountaincar_step_kernel<decltype(V)::value ? 4 : 1, CONT, decltype(T)::value, decltype(fin)...>), g, dim3(kBlock), 0, stream, dev, act, obs_out, reward, done, trunc, fin...);
                });
        }, continuous);
        return st;
    }

    // the one launch of the fused rollout kernel with the action source POLICY; `arg`: the linear weights or the hidden-layer pack, `uni`: the uniform stream, or the
    // Gaussian draw's sigma, seed and call word; `net`: a two-hidden-layer source's Mlp2Net, the head of the kernel's trailing pack
    template <bool CONT, int POLICY, class... Net>
    void launch_rollout(const uint32_t* act, uint32_t* act_out, int K, float* obs_out, float* reward, uint8_t* done, uint8_t* trunc, const PolicyArg<POLICY, 2, CONT ? 1 : 3, McLinearPolicy>& arg,
                        DrawArg<POLICY> uni, Net... net) {
        with_bools([&](auto T) {
            constexpr bool TL = decltype(T)::value;
            if (final_obs) hipLaunchKernelGGL((mountaincar_rollout_kernel<CONT, POLICY, TL, Net..., float*>), dim3(grid_for(n / 4)), dim3(kBlock), 0, stream, dev, act, K, obs_out, reward, done, trunc, arg, act_out, uni, net..., final_obs);
            else hipLaunchKernelGGL((mountaincar_rollout_kernel<CONT, POLICY, TL, Net...>), dim3(grid_for(n / 4)), dim3(kBlock), 0, stream, dev, act, K, obs_out, reward, done, trunc, arg, act_out, uni, net...);
        }, dev.limit != 0u);
    }

    void rollout_table(const uint32_t* act, int K, float* obs_out, float* reward, uint8_t* done, uint8_t* trunc) override {
        with_bools([&](auto C) { launch_rollout<decltype(C)::value, ROLL_ACT_TABLE>(act, nullptr, K, obs_out, reward, done, trunc, McLinearPolicy{}, UniformDraw{}); }, continuous);
    }

    // Discrete(3) takes the categorical draws and A = 3 scores, Box(-1, 1) the Gaussian draws and the one force (the C ABI refuses the other's entry points and heads)
    template <bool CONT>
    int rollout_policy_of(const PolicyCall& call, int K, void* actions_out, float* obs_out, float* reward, uint8_t* done, uint8_t* trunc) {
        return rollout_policy_classic<2, CONT ? 1 : 3, CONT ? roll_act_box_takes : roll_act_discrete_takes>(call, K, actions_out, obs_out, reward, done, trunc, false, nullptr,
            [](const float* w) {   // weights: `rows` rows of (w_position, w_velocity, bias)
                McLinearPolicy lin{};
                constexpr int rows = CONT ? 1 : 3;
                for (int j = 0; j < rows; ++j) { lin.w[j][0] = w[3 * j + 0]; lin.w[j][1] = w[3 * j + 1]; lin.b[j] = w[3 * j + 2]; }
                return lin;
            },
            [&](auto S, const auto& arg, auto... draw_net) { launch_rollout<CONT, decltype(S)::value>(nullptr, static_cast<uint32_t*>(actions_out), K, obs_out, reward, done, trunc, arg, draw_net...); });
    }
    int rollout_policy(const PolicyCall& call, int K, void* actions_out, float* obs_out, float* reward, uint8_t* done, uint8_t* trunc) override {
        return continuous ? rollout_policy_of<true>(call, K, actions_out, obs_out, reward, done, trunc) : rollout_policy_of<false>(call, K, actions_out, obs_out, reward, done, trunc);
    }

    int get_state(void* blob) override { return launch_per_env(mountaincar_export_kernel, dev, static_cast<uint32_t*>(blob)); }
    int set_state(const void* blob) override { return launch_per_env(mountaincar_import_kernel, dev, static_cast<const uint32_t*>(blob)); }
};

Env* make_mountaincar(bool continuous) { return new MountainCarEnv(continuous); }

}  // namespace mgym
