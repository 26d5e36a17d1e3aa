// pendulum.hip — Pendulum-v1 step()/reset() and the fused rollouts as struct-of-arrays gfx950 kernels.
//
// NOT in the reference: gymnasium's Pendulum-v1 restated in f32 (include/mgym.h, MGYM_PENDULUM; pendulum_step.h holds the per-environment lines),
// parity unpinned.  No termination: an episode ends by mgym_config::max_episode_steps alone (time_limit.h).
//
// Data layout in HBM (engine-owned), five columns n_pad words apart: cos[n] sin[n] thdot[n] f32 — the observation, three adjacent columns
// (mgym_observation is a view of them) — th[n] f32 (not wrapped), episode[n] u32 (touched only by reset); elapsed[n] u16 beside them.  One lane
// owns 4 consecutive environments (16-byte accesses).  The step reads the stored sin word as sinf(th) instead of reducing th a second time.
// Algorithmic bytes per env-step of mgym_step: 38 (th, thdot, sin 12 R; cos, sin, thdot, th 16 W; action 4 R; reward 4 W; done 1 W; truncated
// 1 W), with a time limit + 2 R + 2 W = 42.  A rollout keeps th, thdot, cos, sin and the count in registers over its K steps: 10 per env-step.
#include "classic_env.h"
#include "pendulum_step.h"

namespace mgym {

struct PendulumDev {
    float *cs, *sn, *thdot, *th;   // cs + k * n_pad
    uint32_t* episode;
    uint64_t n, seed, env_id_base;
    uint32_t* err;
    unsigned long long* done_count;  // kDoneShards partial counts of finished env-steps (mgym_episode_count)
    float c_g;                       // 1.5f * gravity
    int auto_reset;
    uint16_t* elapsed;   // caller-visible steps since the env's last reset, saturating at 65535 (padded to n_pad like the state columns)
    uint32_t limit;      // max_episode_steps; 0: off
};

// the fused reset of env i: the draw of its current episode, episode + 1 (the caller clears its count)
__device__ __forceinline__ void pendulum_reset_env(const PendulumDev& d, uint64_t i, float& th, float& thdot, float& cs, float& sn) {
    const uint32_t ep = d.episode[i];
    pendulum_reset_one(d.seed, d.env_id_base + i, ep, th, thdot, cs, sn);
    d.episode[i] = ep + 1u;
}

// The generic step kernel: any n, any alignment of the caller's buffers (VEC = 1), or 4 environments per lane with a ragged last group (VEC = 4)
// Fin (here and in the kernels below): mgym_set_final_obs_out (soa4.h) — `fin` is the step's [3][n] slab, or the call's [K][3][n] in a rollout.
template <int VEC, bool TL, class... Fin>
__global__ void __launch_bounds__(kBlock)
pendulum_step_kernel(PendulumDev d, const uint32_t* __restrict__ act, float* __restrict__ obs_out, float* __restrict__ rew, uint8_t* __restrict__ done_out,
                     uint8_t* __restrict__ trunc_out, Fin... fin) {
    const uint64_t groups = (d.n + VEC - 1) / VEC;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    bool bad = false;
    uint32_t finished = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
        const uint64_t i0 = g * VEC;
        float th[VEC], td[VEC], cs[VEC], sn[VEC], r[VEC];
        uint32_t a[VEC];
        uint32_t el[4] = {0u, 0u, 0u, 0u}, tr[4] = {0u, 0u, 0u, 0u};   // (time limit only)
        const bool full = (VEC == 1) || (i0 + VEC <= d.n);
        if constexpr (TL) {
            if (VEC == 4) load_elapsed4(d.elapsed, i0, el);   // (the column is padded: a ragged last group may load it whole)
            else el[0] = d.elapsed[i0];
        }
        if (VEC == 4 && full) {
            const float4 v0 = *reinterpret_cast<const float4*>(d.th + i0), v1 = *reinterpret_cast<const float4*>(d.thdot + i0);
            const float4 v2 = *reinterpret_cast<const float4*>(d.sn + i0);
            const uint4 va = *reinterpret_cast<const uint4*>(act + i0);
            th[0] = v0.x; th[1 % VEC] = v0.y; th[2 % VEC] = v0.z; th[3 % VEC] = v0.w;
            td[0] = v1.x; td[1 % VEC] = v1.y; td[2 % VEC] = v1.z; td[3 % VEC] = v1.w;
            sn[0] = v2.x; sn[1 % VEC] = v2.y; sn[2 % VEC] = v2.z; sn[3 % VEC] = v2.w;
            a[0] = va.x; a[1 % VEC] = va.y; a[2 % VEC] = va.z; a[3 % VEC] = va.w;
        } else {
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const uint64_t i = i0 + k;
                const bool in = i < d.n;
                th[k] = in ? d.th[i] : 0.0f;
                td[k] = in ? d.thdot[i] : 0.0f;
                sn[k] = in ? d.sn[i] : 0.0f;
                a[k] = in ? act[i] : 0u;
            }
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            cs[k] = 1.0f;   // (written by every valid step; read back only where the action was a NaN)
            const bool in = i0 + k < d.n;
            const bool ok = pendulum_env_step<TL>(d.c_g, d.limit, th[k], td[k], cs[k], sn[k], el[k], a[k], r[k], tr[k]);
            if (!ok) { bad = true; if (in) cs[k] = d.cs[i0 + k]; }
            finished += (tr[k] && in) ? 1u : 0u;
            if (d.auto_reset && tr[k] && in) {
                if constexpr (has_final<Fin...>) final_store<3>(final_ptr(fin...) + i0 + k, d.n, {cs[k], sn[k], td[k]});
                pendulum_reset_env(d, i0 + k, th[k], td[k], cs[k], sn[k]); el[k] = 0u;
            }
        }
        if (VEC == 4 && full) {
            const float4 oc = make_float4(cs[0], cs[1 % VEC], cs[2 % VEC], cs[3 % VEC]), os = make_float4(sn[0], sn[1 % VEC], sn[2 % VEC], sn[3 % VEC]);
            const float4 od = make_float4(td[0], td[1 % VEC], td[2 % VEC], td[3 % VEC]);
            nt_store4(d.cs + i0, oc);
            nt_store4(d.sn + i0, os);
            nt_store4(d.thdot + i0, od);
            nt_store4(d.th + i0, make_float4(th[0], th[1 % VEC], th[2 % VEC], th[3 % VEC]));
            if (obs_out) {
                nt_store4(obs_out + i0, oc);
                nt_store4(obs_out + d.n + i0, os);
                nt_store4(obs_out + 2 * d.n + i0, od);
            }
            if (rew) nt_store4(rew + i0, make_float4(r[0], r[1 % VEC], r[2 % VEC], r[3 % VEC]));
            if (done_out) __builtin_nontemporal_store(0u, reinterpret_cast<uint32_t*>(done_out + i0));   // done = 0, always
            if (trunc_out) __builtin_nontemporal_store(pack_bytes4(tr), reinterpret_cast<uint32_t*>(trunc_out + i0));
            if constexpr (TL) store_elapsed4(d.elapsed, i0, el);
        } else {
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const uint64_t i = i0 + k;
                if (i < d.n) {
                    d.cs[i] = cs[k]; d.sn[i] = sn[k]; d.thdot[i] = td[k]; d.th[i] = th[k];
                    if (obs_out) { obs_out[i] = cs[k]; obs_out[d.n + i] = sn[k]; obs_out[2 * d.n + i] = td[k]; }
                    if (rew) rew[i] = r[k];
                    if (done_out) done_out[i] = 0;
                    if (trunc_out) trunc_out[i] = (uint8_t)tr[k];
                    if constexpr (TL) d.elapsed[i] = (uint16_t)el[k];
                }
            }
        }
    }
    flush_counts(d.done_count, d.err, finished, bad);
}

// The 16-byte path (caller buffers aligned, n % 4 == 0, n <= 2^27), the form of mountaincar_step4_kernel: one lane owns 4 consecutive
// environments; block-uniform passes; the engine columns through one buffer resource (descriptor and column / pass offsets in SGPRs, one constant
// VGPR lane offset; the farthest column read or written this way starts 3 n_pad words in, and 16 n_pad + 4 n < 2^32); the columns are padded to
// n_pad (a multiple of the block's 1024 envs), so every lane may load them — only in-range lanes store.  Every load of a pass is issued before the
// sched_barrier.  Finished envs (truncated ones: there is no other end) are counted with __ballot + popcount; resets are rare and stay in place.
// ONE: the single-pass form, one block per tile of 1024 environments (populations of at most the block cap's tiles) — no loop, no test on n before the
// loads, no read of the grid size; !ONE: the grid-stride form.  The arguments are plain scalars and pointers in the order the kernel first needs
// them; the leading 14 dwords (cs .. err) can be asked for as preloaded SGPRs (Makefile, PRELOAD).
template <bool RESET, bool TL, bool ONE, class... Fin>
__global__ void __launch_bounds__(kBlock)
pendulum_step4_kernel(float* cs_col, uint32_t n_pad, uint32_t n, const uint32_t* __restrict__ act, uint16_t* elapsed, uint64_t seed, uint64_t env_id_base,
                      uint32_t* err, unsigned long long* done_count, float* __restrict__ obs_out, float* __restrict__ rew, uint8_t* __restrict__ done_out,
                      uint8_t* __restrict__ trunc_out, uint32_t limit, float c_g, Fin... fin) {
    constexpr uint32_t kPerBlock = (uint32_t)kBlock * 4;
    const uint32_t lane_env = threadIdx.x * 4u, off4 = lane_env * 4u;
    const uint32_t colb = n_pad * 4u;  // column stride in bytes
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(cs_col, 0, 0xffffffff, 0x00020000);
    const PendulumDev d{cs_col, cs_col + n_pad, cs_col + 2 * (uint64_t)n_pad, cs_col + 3 * (uint64_t)n_pad, reinterpret_cast<uint32_t*>(cs_col + 4 * (uint64_t)n_pad),
                        n, seed, env_id_base, err, done_count, c_g, RESET ? 1 : 0, elapsed, limit};
    bool bad = false;
    uint32_t finished = 0;
    uint32_t base = blockIdx.x * kPerBlock;   // block-uniform
    do {
        const uint32_t sb = base * 4u;
        // every load of the pass first
        const u32x4 vs = __builtin_amdgcn_raw_buffer_load_b128(rs, off4, sb + colb, 0);
        const u32x4 vd = __builtin_amdgcn_raw_buffer_load_b128(rs, off4, sb + 2u * colb, 0);
        const u32x4 vt = __builtin_amdgcn_raw_buffer_load_b128(rs, off4, sb + 3u * colb, 0);
        uint32_t el[4] = {0u, 0u, 0u, 0u}, tr[4] = {0u, 0u, 0u, 0u};   // (time limit only)
        if constexpr (TL) load_elapsed4(elapsed, base + lane_env, el);   // (padded to n_pad like the state columns: every lane may load)
        const bool in = lane_env < n - base;
        uint4 va = make_uint4(0u, 0u, 0u, 0u);
        if (in) va = *at<uint4>(act + base, off4);
        __builtin_amdgcn_sched_barrier(0);
        float sn[4] = {as_f32(vs.x), as_f32(vs.y), as_f32(vs.z), as_f32(vs.w)}, td[4] = {as_f32(vd.x), as_f32(vd.y), as_f32(vd.z), as_f32(vd.w)};
        float th[4] = {as_f32(vt.x), as_f32(vt.y), as_f32(vt.z), as_f32(vt.w)}, cs[4] = {1.0f, 1.0f, 1.0f, 1.0f}, r[4];
        const uint32_t a[4] = {va.x, va.y, va.z, va.w};
        uint32_t any_fin = 0, nan_mask = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!pendulum_env_step<TL>(c_g, limit, th[k], td[k], cs[k], sn[k], el[k], a[k], r[k], tr[k])) nan_mask |= 1u << k;
            any_fin |= tr[k];
        }
        if (nan_mask) {   // rare (an error): the env keeps its state, so its cos word is read back
            bad = true;
            const u32x4 vc = __builtin_amdgcn_raw_buffer_load_b128(rs, off4, sb, 0);
            const float c0[4] = {as_f32(vc.x), as_f32(vc.y), as_f32(vc.z), as_f32(vc.w)};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (nan_mask & (1u << k)) cs[k] = c0[k];
        }
        if constexpr (TL) {
            const unsigned long long m = __ballot(in && any_fin);
            if (m) {  // rare: count and (RESET) restart the finished envs in place
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    finished += (uint32_t)__popcll(__ballot(in && tr[k]));
                    if (RESET && in && tr[k]) {
                        if constexpr (has_final<Fin...>) final_store<3>(final_ptr(fin...) + base + lane_env + k, n, {cs[k], sn[k], td[k]});
                        pendulum_reset_env(d, (uint64_t)base + lane_env + k, th[k], td[k], cs[k], sn[k]); el[k] = 0u;
                    }
                }
            }
        }
        if (in) {
            const u32x4 oc{as_u32(cs[0]), as_u32(cs[1]), as_u32(cs[2]), as_u32(cs[3])}, os{as_u32(sn[0]), as_u32(sn[1]), as_u32(sn[2]), as_u32(sn[3])};
            const u32x4 od{as_u32(td[0]), as_u32(td[1]), as_u32(td[2]), as_u32(td[3])};
            __builtin_amdgcn_raw_buffer_store_b128(oc, rs, off4, sb, 2);
            __builtin_amdgcn_raw_buffer_store_b128(os, rs, off4, sb + colb, 2);
            __builtin_amdgcn_raw_buffer_store_b128(od, rs, off4, sb + 2u * colb, 2);
            __builtin_amdgcn_raw_buffer_store_b128(u32x4{as_u32(th[0]), as_u32(th[1]), as_u32(th[2]), as_u32(th[3])}, rs, off4, sb + 3u * colb, 2);
            if (obs_out) {
                float* o = at<float>(obs_out + base, off4);
                nt_store4(o, make_float4(cs[0], cs[1], cs[2], cs[3]));
                nt_store4(o + n, make_float4(sn[0], sn[1], sn[2], sn[3]));
                nt_store4(o + 2 * (uint64_t)n, make_float4(td[0], td[1], td[2], td[3]));
            }
            if (rew) nt_store4(at<float>(rew + base, off4), make_float4(r[0], r[1], r[2], r[3]));
            if (done_out) __builtin_nontemporal_store(0u, reinterpret_cast<uint32_t*>(done_out + base + lane_env));   // done = 0, always
            if (trunc_out) __builtin_nontemporal_store(pack_bytes4(tr), reinterpret_cast<uint32_t*>(trunc_out + base + lane_env));
            if constexpr (TL) store_elapsed4(elapsed, base + lane_env, el);
        }
        if constexpr (ONE) break;
        base += gridDim.x * kPerBlock;   // (at most 2^23 envs a stride: no 32-bit wrap below n <= 2^27)
    } while (base < n);
    if ((threadIdx.x & 63) == 0 && finished)
        atomicAdd(done_count + ((blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) & (kDoneShards - 1)), (unsigned long long)finished);
    if (__any(bad)) {
        if ((threadIdx.x & 63) == 0) atomicOr(err, DEV_ERR_INVALID_ACTION);
    }
}

// Fused K-step rollout (mgym_rollout and the policy forms): 4 environments per lane — th, thdot, cos, sin and the elapsed count — stay in registers
// for K steps; per step one 16-B action word in (TABLE) or out, reward / done / truncated (and optionally the observation) out.  Same per-env
// function and the same in-place auto-reset as the step kernels, hence bit-identical to K separate steps.  One sincos per environment-step.
// The policies decide from (cos, sin, thdot) held before the step (pendulum_step.h); actions_out holds f32 words.
// (mgym_rollout_mlp2's sources take the address of the handle's pack, its widths and sigma at the head of the trailing pack: soa4.h)
// mgym_rollout_mlp_gauss: sigma, the policy seed and the call word travel beside the pack, in the place of the uniform stream (PolicyArg, DrawArg: policy.h)
template <int POLICY = ROLL_ACT_TABLE, bool TL = false, class... Fin>
__global__ void __launch_bounds__(kBlock)
pendulum_rollout_kernel(PendulumDev d, const uint32_t* __restrict__ act, int K, float* __restrict__ obs_out, float* __restrict__ rew,
                        uint8_t* __restrict__ done_out, uint8_t* __restrict__ trunc_out, PolicyArg<POLICY, 3, 1, PdLinearPolicy> pol = {}, uint32_t* __restrict__ act_out = nullptr,
                        DrawArg<POLICY> uni = {}, Fin... fin) {
    static_assert(roll_act_box_takes(POLICY), "Pendulum has no categorical draw");
    const uint64_t groups = d.n / 4;  // n % 4 == 0 is required by the host wrapper
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    bool bad = false;
    uint32_t finished = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
        const uint64_t i0 = g * 4;
        const float4 v0 = *reinterpret_cast<const float4*>(d.th + i0), v1 = *reinterpret_cast<const float4*>(d.thdot + i0);
        const float4 v2 = *reinterpret_cast<const float4*>(d.cs + i0), v3 = *reinterpret_cast<const float4*>(d.sn + i0);
        float th[4] = {v0.x, v0.y, v0.z, v0.w}, td[4] = {v1.x, v1.y, v1.z, v1.w}, cs[4] = {v2.x, v2.y, v2.z, v2.w}, sn[4] = {v3.x, v3.y, v3.z, v3.w};
        uint32_t el[4] = {0u, 0u, 0u, 0u};   // (time limit only: the count lives in registers across the K steps)
        if constexpr (TL) load_elapsed4(d.elapsed, i0, el);
        for (int t = 0; t < K; ++t) {
            const uint64_t off = (uint64_t)t * d.n + i0;
            uint32_t a[4];
            if constexpr (POLICY == ROLL_ACT_UNIFORM) {
                pendulum_uniform_actions(uni.seed, uni.call, d.env_id_base + i0, (uint32_t)t, a);
            } else if constexpr (roll_act_gauss(POLICY)) {
                // mgym_rollout_mlp_gauss: written out beside the branch below, through the forwarding function it always had (no other form kept its code)
                const float o[4][3] = {{cs[0], sn[0], td[0]}, {cs[1], sn[1], td[1]}, {cs[2], sn[2], td[2]}, {cs[3], sn[3], td[3]}};
                pendulum_gauss_actions<roll_act_hidden_act(POLICY)>(pol, o, uni.seed, uni.call, d.env_id_base + i0, (uint32_t)t, uni.sigma, a);
            } else if constexpr (roll_act_is_mlp(POLICY) || roll_act_is_mlp2(POLICY)) {
                // hidden-layer policy of either depth on (cos, sin, thdot): the one score is the torque, or (the two-layer GAUSS head) the mean of the draw around it —
                // one Philox evaluation per lane per step, its two word pairs for the lane's two env pairs (policy.h: net, activation and head; the step clamps the torque)
                const float o[4][3] = {{cs[0], sn[0], td[0]}, {cs[1], sn[1], td[1]}, {cs[2], sn[2], td[2]}, {cs[3], sn[3], td[3]}};
                Philox4 w;
                policy_draw<POLICY>(uni.seed, d.env_id_base + i0, uni.call, (uint32_t)t, w);
                policy_actions4<POLICY, 3, 1>(pol, w.w, draw_sigma(uni), o, a, fin...);
            } else if constexpr (POLICY == ROLL_ACT_LINEAR) {
#pragma unroll
                for (int k = 0; k < 4; ++k) a[k] = pendulum_linear_action(pol, cs[k], sn[k], td[k]);
            } else {
                const u32x4 va = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(act + off));
                a[0] = va.x; a[1] = va.y; a[2] = va.z; a[3] = va.w;
            }
            if constexpr (POLICY != ROLL_ACT_TABLE) {
                if (act_out) __builtin_nontemporal_store(u32x4{a[0], a[1], a[2], a[3]}, reinterpret_cast<u32x4*>(act_out + off));
            }
            float r[4];
            uint32_t tr[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!pendulum_env_step<TL>(d.c_g, d.limit, th[k], td[k], cs[k], sn[k], el[k], a[k], r[k], tr[k])) bad = true;   // (cs is live here: a NaN action leaves it)
                finished += tr[k];
                if (d.auto_reset && tr[k]) {
                    if constexpr (has_final<Fin...>) final_store<3>(final_ptr(fin...) + (uint64_t)t * 3 * d.n + i0 + k, d.n, {cs[k], sn[k], td[k]});
                    pendulum_reset_env(d, i0 + k, th[k], td[k], cs[k], sn[k]); el[k] = 0u;
                }
            }
            if (rew) nt_store4(rew + off, make_float4(r[0], r[1], r[2], r[3]));
            if (done_out) __builtin_nontemporal_store(0u, reinterpret_cast<uint32_t*>(done_out + off));   // done = 0, always
            if (trunc_out) __builtin_nontemporal_store(pack_bytes4(tr), reinterpret_cast<uint32_t*>(trunc_out + off));
            if (obs_out) {
                float* o = obs_out + (uint64_t)t * 3 * d.n + i0;
                nt_store4(o, make_float4(cs[0], cs[1], cs[2], cs[3]));
                nt_store4(o + d.n, make_float4(sn[0], sn[1], sn[2], sn[3]));
                nt_store4(o + 2 * d.n, make_float4(td[0], td[1], td[2], td[3]));
            }
        }
        nt_store4(d.cs + i0, make_float4(cs[0], cs[1], cs[2], cs[3]));
        nt_store4(d.sn + i0, make_float4(sn[0], sn[1], sn[2], sn[3]));
        nt_store4(d.thdot + i0, make_float4(td[0], td[1], td[2], td[3]));
        nt_store4(d.th + i0, make_float4(th[0], th[1], th[2], th[3]));
        if constexpr (TL) store_elapsed4(d.elapsed, i0, el);
    }
    flush_counts(d.done_count, d.err, finished, bad);
}

__global__ void __launch_bounds__(kBlock)
pendulum_reset_kernel(PendulumDev d, const uint8_t* __restrict__ m0, const uint8_t* __restrict__ m1, int all, int masks_aligned, float* __restrict__ obs_out) {
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
                float th, td, cs, sn;
                pendulum_reset_env(d, i, th, td, cs, sn);
                d.cs[i] = cs; d.sn[i] = sn; d.thdot[i] = td; d.th[i] = th;
                d.elapsed[i] = 0;
                if (obs_out) { obs_out[i] = cs; obs_out[d.n + i] = sn; obs_out[2 * d.n + i] = td; }
            }
        }
    }
}

// mgym_reset_deterministic: th = 0, thdot = 0 -> the observation (1, 0, 0); the episode number stays
__global__ void pendulum_zero_kernel(PendulumDev d, float* __restrict__ obs_out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.n) return;
    d.cs[i] = 1.0f; d.sn[i] = 0.0f; d.thdot[i] = 0.0f; d.th[i] = 0.0f;
    d.elapsed[i] = 0;
    if (obs_out) { obs_out[i] = 1.0f; obs_out[d.n + i] = 0.0f; obs_out[2 * d.n + i] = 0.0f; }
}

// state blob: th, thdot, episode
__global__ void pendulum_export_kernel(PendulumDev d, uint32_t* __restrict__ blob) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.n) return;
    blob[i] = as_u32(d.th[i]);
    blob[d.n + i] = as_u32(d.thdot[i]);
    blob[2 * d.n + i] = d.episode[i];
}

__global__ void pendulum_import_kernel(PendulumDev d, const uint32_t* __restrict__ blob) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.n) return;
    const float th = as_f32(blob[i]);
    float cs, sn;
    pendulum_sincos(th, cs, sn);   // the stored cos and sin are those of the imported th word
    d.th[i] = th; d.cs[i] = cs; d.sn[i] = sn;
    d.thdot[i] = as_f32(blob[d.n + i]);
    d.episode[i] = blob[2 * d.n + i];
    d.elapsed[i] = 0;   // the blob stays 3 columns: an imported state starts its count at 0 (mgym_set_elapsed_steps overrides)
}

struct PendulumEnv final : ClassicEnv {
    PendulumDev dev{};

    int init() override {
        obs_dim = 3;
        state_cols = 3;
        if (const int st = alloc(5)) return st;
        float* f = cols;
        MGYM_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(f), 0x3f800000, n_pad, stream));   // th = 0: cos = 1
        dev.cs = f; dev.sn = f + n_pad; dev.thdot = f + 2 * n_pad; dev.th = f + 3 * n_pad;
        dev.episode = reinterpret_cast<uint32_t*>(f + 4 * n_pad);
        fill_common(dev);
        dev.c_g = pendulum_c_g(cfg.gravity);
        return MGYM_OK;
    }

    int reset(const uint8_t* m0, const uint8_t* m1, bool all, float* obs_out) override { return launch_reset(pendulum_reset_kernel, dev, m0, m1, all, obs_out); }
    int reset_deterministic(float* obs_out) override { return launch_per_env(pendulum_zero_kernel, dev, obs_out); }

    int step(const void* actions, float* obs_out, float* reward, uint8_t* done, uint8_t* trunc) override {
        const uint32_t* act = static_cast<const uint32_t*>(actions);
        // (the final-observation forms exist with a time limit only: final_live())
        return launch_step(act, obs_out, reward, done, trunc,
            [&](dim3 g, auto R, auto T, auto O, auto... fin) {
                if constexpr (decltype(T)::value || sizeof...(fin) == 0)
                    hipLaunchKernelGGL((pendulum_step4_kernel<decltype(R)::value, decltype(T)::value, decltype(O)::value, decltype(fin)...>), g, dim3(kBlock), 0, stream, dev.cs, (uint32_t)n_pad,
                                       (uint32_t)n, act, dev.elapsed, dev.seed, dev.env_id_base, dev.err, dev.done_count, obs_out, reward, done, trunc, dev.limit, dev.c_g, fin...);
            },
            [&](dim3 g, auto V, auto T, auto... fin) {
                if constexpr (decltype(T)::value || sizeof...(fin) == 0)
                    hipLaunchKernelGGL((pendulum_step_kernel<decltype(V)::value ? 4 : 1, decltype(T)::value, decltype(fin)...>), g, dim3(kBlock), 0, stream, dev, act, obs_out, reward, done, trunc, fin...);
            });
    }

    // the one launch of the fused rollout kernel with the action source POLICY; `arg`: the linear words or the hidden-layer pack, `uni`: the uniform stream, or the
    // Gaussian draw's sigma, seed and call word; `net`: a two-hidden-layer source's Mlp2Net, the head of the kernel's trailing pack
    template <int POLICY, class... Net>
    void launch_rollout(const uint32_t* act, uint32_t* act_out, int K, float* obs_out, float* reward, uint8_t* done, uint8_t* trunc, const PolicyArg<POLICY, 3, 1, PdLinearPolicy>& arg,
                        DrawArg<POLICY> uni, Net... net) {
        with_bools([&](auto T, auto F) {
            constexpr bool TL = decltype(T)::value;
            if constexpr (!decltype(F)::value) hipLaunchKernelGGL((pendulum_rollout_kernel<POLICY, TL, Net...>), dim3(grid_for(n / 4)), dim3(kBlock), 0, stream, dev, act, K, obs_out, reward, done, trunc, arg, act_out, uni, net...);
            else if constexpr (TL) hipLaunchKernelGGL((pendulum_rollout_kernel<POLICY, true, Net..., float*>), dim3(grid_for(n / 4)), dim3(kBlock), 0, stream, dev, act, K, obs_out, reward, done, trunc, arg, act_out, uni, net..., final_obs);
        }, dev.limit != 0u, final_live());
    }

    // without a time limit no Pendulum episode ever ends
    bool final_live() const override { return final_obs != nullptr && dev.limit != 0u; }

    void rollout_table(const uint32_t* act, int K, float* obs_out, float* reward, uint8_t* done, uint8_t* trunc) override {
        launch_rollout<ROLL_ACT_TABLE>(act, nullptr, K, obs_out, reward, done, trunc, PdLinearPolicy{}, UniformDraw{});
    }

    int rollout_policy(const PolicyCall& call, int K, void* actions_out, float* obs_out, float* reward, uint8_t* done, uint8_t* trunc) override {
        const char* refusal = roll_act_samples(call.source) ? ": Pendulum has no discrete actions to draw from" : nullptr;   // (the C ABI refuses it first)
        return rollout_policy_classic<3, 1, roll_act_box_takes>(call, K, actions_out, obs_out, reward, done, trunc, false, refusal,
            [](const float* w) { return PdLinearPolicy{{w[0], w[1], w[2]}, w[3]}; },
            [&](auto S, const auto& arg, auto... draw_net) { launch_rollout<decltype(S)::value>(nullptr, static_cast<uint32_t*>(actions_out), K, obs_out, reward, done, trunc, arg, draw_net...); });
    }

    int get_state(void* blob) override { return launch_per_env(pendulum_export_kernel, dev, static_cast<uint32_t*>(blob)); }
    int set_state(const void* blob) override { return launch_per_env(pendulum_import_kernel, dev, static_cast<const uint32_t*>(blob)); }
};

Env* make_pendulum() { return new PendulumEnv(); }

}  // namespace mgym
