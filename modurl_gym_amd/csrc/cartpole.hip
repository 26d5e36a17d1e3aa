// cartpole.hip — CartPoleV1 step()/reset() as struct-of-arrays gfx950 kernels.
//
// Replaces the bodies of `impl Gym for CartPoleV1` (reference src/classic_control/cartpole.rs:
// reset :238-249, step :251-348) for n_envs independent environments.
//
// Data layout in HBM (engine-owned, one allocation, column stride n_pad words):
//   x[n] x_dot[n] theta[n] theta_dot[n]   f32   — the state, which IS the observation (:301)
//   ctr[n]                                u32   — steps_since_reset | steps_beyond_terminated | episode
//                                                 (bit layout in cartpole_step.h)
// One lane owns 4 consecutive environments: every column is read and written with one
// 16-byte access per lane (1 KiB per wave instruction, fully coalesced).  The engine's columns are
// addressed through ONE buffer resource — descriptor and column / pass offsets in SGPRs, one constant
// VGPR lane offset, no per-lane address arithmetic; the physics constants (cartpole.rs:45-56: none is a
// builder argument) are compile-time constants; outputs leave with non-temporal stores.
// No MFMA: the physics is element-wise, and the one contraction (the hidden layer of mgym_rollout_mlp) was measured faster as packed VALU FMAs.
//
// Algorithmic HBM bytes per env-step (obs_out == NULL, zero-copy observation): 50
//   state 16 R + 16 W, action 4 R, reward 4 W, done 1 W, truncated 1 W, ctr 4 R + 4 W.
// There is no other per-env word: the episode counter that keys the reset draws rides in `ctr`.
//
// Arithmetic: cartpole_step.h.  A wave whose 256 environments all pass cartpole_fast_ok() (theta on the
// small-argument path, bounded theta_dot, valid action: every live environment) runs the branch-free fast
// form, proven bit-identical to the reference form; any other wave runs the reference form for that pass.
//
// Done-mask handling (fused auto-reset, MGYM_FLAG_AUTO_RESET): finished environments are rare per ENV
// (~4.5 % per step under a random policy) but nearly every WAVE holds one, so resetting in place would make
// every wave pay Philox4x32-10 (quarter-rate integer multiplies) four times over.  Instead each wave
// compacts its finished envs with __ballot + popcount prefix sums into a wave-private LDS list (no block
// barrier, no atomics), the wave's first lanes draw all new states in ONE pass (two lanes per env, one Philox
// evaluation each), owners read theirs back.  The step kernel stores reward, done and truncated before that pass.
// The same ballots feed the per-handle finished-episode counter (mgym_episode_count).
#include "common.h"
#include "cartpole_step.h"
#include "mlp_policy.h"
#include "philox.h"
#include "soa4.h"

namespace mgym {

struct CartPoleDev {
    float* base;        // columns x, x_dot, theta, theta_dot, ctr at base + k * n_pad (one pointer: SGPR budget)
    uint64_t n_pad;
    uint64_t n;
    uint64_t seed, env_id_base;
    uint32_t* err;
    unsigned long long* done_count;  // kDoneShards partial counts (finished env-steps)
    __host__ __device__ float* x() const { return base; }
    __host__ __device__ float* xd() const { return base + n_pad; }
    __host__ __device__ float* th() const { return base + 2 * n_pad; }
    __host__ __device__ float* thd() const { return base + 3 * n_pad; }
    __host__ __device__ uint32_t* ctr() const { return reinterpret_cast<uint32_t*>(base + 4 * n_pad); }
};

constexpr int kNtAux = 2;   // cache-policy bits of a buffer store, 2 = nt.  Every output leaves with non-temporal stores: 10.9 us vs 11.4 us at 1 Mi envs (round 1)
constexpr int kWaves = kBlock / 64;

struct CartPoleLane {
    float x, xd, th, thd;
    uint32_t ctr;
};

// reset(): cartpole.rs:238-249 — state ~ U[-0.05, 0.05)^4 sampled in f64 then cast,
// steps_since_reset = 0, steps_beyond_terminated = None.  `episode` = Philox counter word 2.
// Half h of the new state (h = 0: x, x_dot from SLOT_RESET0; h = 1: theta, theta_dot from SLOT_RESET1) is one
// Philox evaluation: the halves are independent, so two lanes can draw one env's state.
__device__ __forceinline__ void cartpole_draw_half(uint64_t seed, uint64_t gid, uint32_t episode, uint32_t h, float out[2]) {
    Philox4 a = env_draw(seed, gid, episode, SLOT_RESET0 + h);
    out[0] = uniform_f64_to_f32(-0.05, 0.05, a.w[0], a.w[1]);
    out[1] = uniform_f64_to_f32(-0.05, 0.05, a.w[2], a.w[3]);
}
__device__ __forceinline__ void cartpole_draw(uint64_t seed, uint64_t gid, uint32_t episode, float out[4]) {
    cartpole_draw_half(seed, gid, episode, 0u, out);
    cartpole_draw_half(seed, gid, episode, 1u, out + 2);
}

// non-temporal store of one word: a lane's four done / truncated bytes
__device__ __forceinline__ void st1u(uint32_t* p, uint32_t a) { __builtin_nontemporal_store(a, p); }

// Wave-private scratch of the done-mask compaction: one wave's finished envs (at most 64 * VEC)
template <int VEC>
struct WaveResetScratch {
    uint32_t ent[64 * VEC];     // (episode << 12) | local env id within the wave's 64*VEC envs
    float fresh[64 * VEC][4];   // new states by list slot
};

// A wave pass is two calls, and every lane of the wave makes both (wave collectives):
//   cartpole_wave_advance  steps the VEC environments of every lane (fast form when the whole wave qualifies);
//                          reward / done / truncated are final after it (the step kernel stores them before the reset)
//   cartpole_wave_reset    counts the finished envs and — RESET — replaces them by fresh episodes in place
template <int VEC, bool EULER, bool SB>
__device__ __forceinline__ void cartpole_wave_advance(CartPoleLane (&s)[VEC], const uint32_t (&a)[VEC], const bool (&valid)[VEC],
                                                      float (&r)[VEC], uint32_t (&dn)[VEC], uint32_t (&tr)[VEC], bool& bad) {
    constexpr CartPoleParams P = cartpole_params(EULER ? 1 : 0, SB ? 1 : 0);
    bool ok = true;
#pragma unroll
    for (int k = 0; k < VEC; ++k) ok = ok & cartpole_fast_ok(s[k].th, s[k].thd, a[k]);  // bitwise: no short-circuit branches
    if (__all(ok)) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) cartpole_step_fast<EULER, SB>(P, s[k].x, s[k].xd, s[k].th, s[k].thd, s[k].ctr, a[k], r[k], dn[k], tr[k]);
    } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k)
            if (!cartpole_step_ref(P, s[k].x, s[k].xd, s[k].th, s[k].thd, s[k].ctr, a[k], r[k], dn[k], tr[k]) && valid[k]) bad = true;
    }
}

// `wave_first` = index of the wave's first environment.  Returns the number of finished envs in this wave pass.
// The draw pass gives each listed env two lanes, one per Philox evaluation (cartpole_draw_half): lane j draws half
// j & 1 of list entry j >> 1, so one pass serves up to 32 finished envs (a wave holds ~11.5 per step at 1 Mi envs
// under a random policy) and half as many Philox rounds sit in the pass as with one lane per env.
template <int VEC, bool RESET>
__device__ __forceinline__ uint32_t cartpole_wave_reset(const CartPoleDev& d, CartPoleLane (&s)[VEC], const bool (&valid)[VEC],
                                                        const uint32_t (&dn)[VEC], const uint32_t (&tr)[VEC], uint64_t wave_first,
                                                        WaveResetScratch<VEC>& lds) {
    // done-mask reduction: ballots + popcounts give every finished env its slot in the wave's list
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t slot[VEC];
    uint32_t total = 0;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const bool fin = valid[k] && (dn[k] | tr[k]);
        const unsigned long long m = __ballot(fin);
        slot[k] = fin ? total + (uint32_t)__popcll(m & below) : 0xffffffffu;
        total += (uint32_t)__popcll(m);
    }
    if (RESET && total) {
#pragma unroll
        for (int k = 0; k < VEC; ++k)
            if (slot[k] != 0xffffffffu) lds.ent[slot[k]] = (s[k].ctr & (kCpEpMask << kCpEpShift)) | (uint32_t)(lane * VEC + k);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (uint32_t j = (uint32_t)lane; j < 2u * total; j += 64u) {  // one pass unless > 32 envs of the wave finished at once
            const uint32_t e = lds.ent[j >> 1], h = j & 1u;
            float f[2];
            cartpole_draw_half(d.seed, d.env_id_base + wave_first + (e & 0xfffu), e >> kCpEpShift, h, f);
            *reinterpret_cast<float2*>(&lds.fresh[j >> 1][2u * h]) = make_float2(f[0], f[1]);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            if (slot[k] != 0xffffffffu) {
                s[k].x = lds.fresh[slot[k]][0]; s[k].xd = lds.fresh[slot[k]][1];
                s[k].th = lds.fresh[slot[k]][2]; s[k].thd = lds.fresh[slot[k]][3];
                s[k].ctr = cp_ctr_after_reset(s[k].ctr);
            }
        }
        __builtin_amdgcn_wave_barrier();  // the list is reused by the wave's next pass
    }
    return total;
}

// Every thread of the block calls this once, at the end of the kernel.
template <int WAVES>
__device__ __forceinline__ void cartpole_flush_counts(const CartPoleDev& d, uint32_t finished, bool bad) {
    // the block's waves add their counts in LDS, then one fire-and-forget atomic per block, spread over kDoneShards
    // addresses.  The shards share 16 cache lines and memory-side atomics on one line serialise: one atomic per wave
    // (4096 per launch at 1 Mi envs) left a 0.44 us tail on the launch, measured against a build without the count.
    __shared__ uint32_t wave_fin[WAVES];
    if (WAVES > 1) {
        if ((threadIdx.x & 63) == 0) wave_fin[threadIdx.x >> 6] = finished;
        __syncthreads();
        finished = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) finished += wave_fin[w];
    }
    if (threadIdx.x == 0 && finished)
        atomicAdd(d.done_count + (blockIdx.x & (kDoneShards - 1)), (unsigned long long)finished);
    if (__any(bad)) {
        if ((threadIdx.x & 63) == 0) atomicOr(d.err, DEV_ERR_INVALID_ACTION);
    }
}

// VEC: envs per lane (4 = 16-byte accesses; 1 = fallback for misaligned caller buffers).
// RESET: MGYM_FLAG_AUTO_RESET.
// ONE: the single-pass form — the host launched exactly one block per tile of BLK * VEC environments (every population of at most the block cap's
// tiles: 8 Mi envs at 256 threads), so the instantiation has no loop, no test on n before its loads and no read of the grid size.  !ONE: the
// grid-stride form of larger populations; the host launches no more blocks than tiles, so a block's first pass needs no test either.
// The arguments are plain scalars and pointers in the order the kernel first needs them — what the state loads need (base, n_pad), then n and
// the actions, then the rest — and CartPoleDev is rebuilt from them for the per-wave functions: the leading 14 dwords (base .. done_count)
// can be asked for as preloaded SGPRs (Makefile, PRELOAD); without that one scalar load and one wait stand before the loads.
// Fin: mgym_set_final_obs_out (soa4.h) — `fin` is the step's [4][n] slab; a finished env's four words leave with reward / done / truncated, ahead of the reset pass.
template <int VEC, bool EULER, bool SB, bool RESET, int BLK, bool ONE, class... Fin>
__global__ void __launch_bounds__(BLK)
cartpole_step_kernel(float* col0, uint32_t n_pad, uint32_t n, const uint32_t* __restrict__ act, uint64_t seed, uint64_t env_id_base, uint32_t* err,
                     unsigned long long* done_count, float* __restrict__ obs_out, float* __restrict__ rew, uint8_t* __restrict__ done_out,
                     uint8_t* __restrict__ trunc_out, Fin... fin) {
    __shared__ WaveResetScratch<VEC> lds_[RESET ? BLK / 64 : 1];
    constexpr uint32_t kPerBlock = (uint32_t)BLK * VEC;
    const uint32_t lane_env = threadIdx.x * VEC;     // first env of this lane within the block's slice
    const uint32_t off4 = lane_env * 4u;             // its byte offset in a 4-byte column
    const uint32_t colb = n_pad * 4u;                // engine column stride in bytes
    // raw buffer resource over the engine's allocation (stride 0, no bounds clamp, 32-bit data format: gfx9 word 3 = 0x00020000)
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(col0, 0, 0xffffffff, 0x00020000);
    const CartPoleDev d{col0, n_pad, n, seed, env_id_base, err, done_count};
    bool bad = false;
    uint32_t finished = 0;
    uint32_t base = blockIdx.x * kPerBlock;          // wave-uniform; n <= 2^27: env indices and byte offsets fit 32 bits
    do {
        const uint32_t sb = base * 4u;               // byte offset of this pass in a column
        CartPoleLane s[VEC];
        uint32_t a[VEC];
        bool valid[VEC];
        float r[VEC];
        uint32_t dn[VEC], tr[VEC];
        bool in;  // the host launches VEC = 4 only when n % 4 == 0: a lane is wholly in or out
        float* const bx = col0 + base;
        const uint64_t col = n_pad;
        if constexpr (VEC == 4) {
            // Engine columns: buffer loads — resource descriptor and column/pass offsets in SGPRs, one constant VGPR lane
            // offset, no per-lane address arithmetic.  The columns are padded to n_pad (a multiple of the block's 1024
            // envs), so every lane of the block may load (padding holds zeros and is never stored back).
            // Every load of the pass is issued here, before anything that feeds no address.
            const u32x4 vth = __builtin_amdgcn_raw_buffer_load_b128(rs, off4, sb + 2u * colb, 0);
            const u32x4 vthd = __builtin_amdgcn_raw_buffer_load_b128(rs, off4, sb + 3u * colb, 0);
            const u32x4 vx = __builtin_amdgcn_raw_buffer_load_b128(rs, off4, sb, 0);
            const u32x4 vxd = __builtin_amdgcn_raw_buffer_load_b128(rs, off4, sb + colb, 0);
            const u32x4 vc = __builtin_amdgcn_raw_buffer_load_b128(rs, off4, sb + 4u * colb, 0);
            in = lane_env < n - base;
            uint4 va = make_uint4(0u, 0u, 0u, 0u);
            if (in) va = *at<uint4>(act + base, off4);  // caller buffer: n words exactly
            __builtin_amdgcn_sched_barrier(0);
            s[0] = {as_f32(vx.x), as_f32(vxd.x), as_f32(vth.x), as_f32(vthd.x), vc.x};
            s[1] = {as_f32(vx.y), as_f32(vxd.y), as_f32(vth.y), as_f32(vthd.y), vc.y};
            s[2] = {as_f32(vx.z), as_f32(vxd.z), as_f32(vth.z), as_f32(vthd.z), vc.z};
            s[3] = {as_f32(vx.w), as_f32(vxd.w), as_f32(vth.w), as_f32(vthd.w), vc.w};
            a[0] = va.x; a[1] = va.y; a[2] = va.z; a[3] = va.w;
        } else {
            in = lane_env < n - base;
            s[0] = {0.f, 0.f, 0.f, 0.f, 0u};
            a[0] = 0u;
            if (in) {
                s[0] = {*at<float>(bx, off4), *at<float>(bx + col, off4), *at<float>(bx + 2 * col, off4), *at<float>(bx + 3 * col, off4),
                        *at<uint32_t>(bx + 4 * col, off4)};
                a[0] = *at<uint32_t>(act + base, off4);
            }
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) valid[k] = in;
        WaveResetScratch<VEC>& lds = lds_[RESET ? (threadIdx.x >> 6) : 0];
        cartpole_wave_advance<VEC, EULER, SB>(s, a, valid, r, dn, tr, bad);
        // reward / done / truncated do not depend on the reset: issued here, their write-out drains while the reset
        // pass runs (the LDS fences of cartpole_wave_reset keep the compiler from sinking them past it)
        if (in) {
            if constexpr (VEC == 4) {
                if (rew) nt_store4(at<float>(rew + base, off4), make_float4(r[0], r[1], r[2], r[3]));
                if (done_out) st1u(at<uint32_t>(done_out + base, lane_env), pack_bytes4(dn));
                if (trunc_out) st1u(at<uint32_t>(trunc_out + base, lane_env), pack_bytes4(tr));
            } else {
                if (rew) *at<float>(rew + base, off4) = r[0];
                if (done_out) *at<uint8_t>(done_out + base, lane_env) = (uint8_t)dn[0];
                if (trunc_out) *at<uint8_t>(trunc_out + base, lane_env) = (uint8_t)tr[0];
            }
            if constexpr (has_final<Fin...>) {
#pragma unroll
                for (int k = 0; k < VEC; ++k)
                    if (dn[k] | tr[k]) final_store<4>(at<float>(final_ptr(fin...) + base, off4) + k, n, {s[k].x, s[k].xd, s[k].th, s[k].thd});
            }
        }
        const uint64_t wave_first = base + (uint64_t)(threadIdx.x & ~63) * VEC;
        finished += cartpole_wave_reset<VEC, RESET>(d, s, valid, dn, tr, wave_first, lds);

        if (in) {
            if constexpr (VEC == 4) {
                __builtin_amdgcn_raw_buffer_store_b128(u32x4{as_u32(s[0].x), as_u32(s[1].x), as_u32(s[2].x), as_u32(s[3].x)}, rs, off4, sb, kNtAux);
                __builtin_amdgcn_raw_buffer_store_b128(u32x4{as_u32(s[0].xd), as_u32(s[1].xd), as_u32(s[2].xd), as_u32(s[3].xd)}, rs, off4, sb + colb, kNtAux);
                __builtin_amdgcn_raw_buffer_store_b128(u32x4{as_u32(s[0].th), as_u32(s[1].th), as_u32(s[2].th), as_u32(s[3].th)}, rs, off4, sb + 2u * colb, kNtAux);
                __builtin_amdgcn_raw_buffer_store_b128(u32x4{as_u32(s[0].thd), as_u32(s[1].thd), as_u32(s[2].thd), as_u32(s[3].thd)}, rs, off4, sb + 3u * colb, kNtAux);
                __builtin_amdgcn_raw_buffer_store_b128(u32x4{s[0].ctr, s[1].ctr, s[2].ctr, s[3].ctr}, rs, off4, sb + 4u * colb, kNtAux);
                if (obs_out) {
                    float* const bo = obs_out + base;
                    *at<float4>(bo, off4) = make_float4(s[0].x, s[1].x, s[2].x, s[3].x);
                    *at<float4>(bo + d.n, off4) = make_float4(s[0].xd, s[1].xd, s[2].xd, s[3].xd);
                    *at<float4>(bo + 2 * d.n, off4) = make_float4(s[0].th, s[1].th, s[2].th, s[3].th);
                    *at<float4>(bo + 3 * d.n, off4) = make_float4(s[0].thd, s[1].thd, s[2].thd, s[3].thd);
                }
            } else {
                *at<float>(bx, off4) = s[0].x; *at<float>(bx + col, off4) = s[0].xd; *at<float>(bx + 2 * col, off4) = s[0].th;
                *at<float>(bx + 3 * col, off4) = s[0].thd; *at<uint32_t>(bx + 4 * col, off4) = s[0].ctr;
                if (obs_out) {
                    float* const bo = obs_out + base;
                    *at<float>(bo, off4) = s[0].x; *at<float>(bo + d.n, off4) = s[0].xd;
                    *at<float>(bo + 2 * d.n, off4) = s[0].th; *at<float>(bo + 3 * d.n, off4) = s[0].thd;
                }
            }
        }
        if constexpr (ONE) break;
        base += gridDim.x * kPerBlock;   // (at most 2^23 envs a stride: no 32-bit wrap below n <= 2^27)
    } while (base < n);
    cartpole_flush_counts<BLK / 64>(d, finished, bad);
}

// policy of a fused rollout: actions from the caller's [K][n] table, or drawn / decided on the device (the action sources of policy.h)
struct LinearPolicy { float w[4], b; };   // action = ((w0 x + w1 x_dot) + w2 theta) + w3 theta_dot + b > 0 (mgym_rollout_linear)
// mgym_rollout_mlp: the weight pack of mlp_policy.h, MlpPack<4, 2>, takes the place of the five linear words in the kernel's arguments (PolicyArg, policy.h:
// 1 804 bytes by value; the other policies' instantiations keep the arguments they had)
// (mgym_rollout_mlp2's sources take the address of the handle's pack and its widths at the head of the trailing pack: soa4.h)

// Fused K-step rollout (mgym_rollout / mgym_rollout_uniform): one lane keeps its 4 environments in registers for
// K steps; per step it reads one 16-B action word (or takes the next bit of its Philox policy stream) and writes
// reward / done / truncated (and the observation / the drawn actions if asked).  Identical to K launches of
// cartpole_step_kernel by construction: same per-wave function.
// Fin: the call's [K][4][n] final observations — stored before the reset pass, which replaces the registers (the other outputs of a step leave after it)
template <bool EULER, bool SB, bool RESET, int POLICY, class... Fin>
__global__ void __launch_bounds__(kBlock)
cartpole_rollout_kernel(CartPoleDev d, const uint32_t* __restrict__ act, uint32_t* __restrict__ act_out, uint64_t policy_seed, uint32_t policy_call, PolicyArg<POLICY, 4, 2, LinearPolicy> lin,
                        int K, float* __restrict__ obs_out, float* __restrict__ rew, uint8_t* __restrict__ done_out, uint8_t* __restrict__ trunc_out, Fin... fin) {
    __shared__ WaveResetScratch<4> lds_[RESET ? kWaves : 1];
    constexpr uint64_t kPerBlock = (uint64_t)kBlock * 4;
    bool bad = false;
    uint32_t finished = 0;
    WaveResetScratch<4>& lds = lds_[RESET ? (threadIdx.x >> 6) : 0];
    // per-step buffers through buffer resources: descriptor + (step, pass) offset in SGPRs, one constant VGPR lane offset.
    // The host wrapper guarantees K * n * 4 < 2^32 (fused_rollout_args_ok: every byte offset into a [K][n] word buffer fits 32 bits) and n % 4 == 0.
    const uint32_t lane_env = threadIdx.x * 4u, off4 = lane_env * 4u;
    const uint32_t colb = (uint32_t)d.n_pad * 4u, nb4 = (uint32_t)d.n * 4u;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(d.base, 0, 0xffffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(POLICY == ROLL_ACT_TABLE ? act : act_out), 0, 0xffffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(rew, 0, 0xffffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(done_out, 0, 0xffffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rt = __builtin_amdgcn_make_buffer_rsrc(trunc_out, 0, 0xffffffff, 0x00020000);
    for (uint64_t base = (uint64_t)blockIdx.x * kPerBlock; base < d.n; base += (uint64_t)gridDim.x * kPerBlock) {
        const uint64_t i0 = base + (uint64_t)threadIdx.x * 4;
        const uint64_t left = d.n - base;
        const bool in = lane_env < (left < kPerBlock ? (uint32_t)left : (uint32_t)kPerBlock);
        const uint32_t sb = (uint32_t)base * 4u;
        CartPoleLane s[4];
        bool valid[4] = {in, in, in, in};
        {   // engine columns are padded to the block's span: every lane may load; only in-range lanes store
            const u32x4 vx = __builtin_amdgcn_raw_buffer_load_b128(rs, off4, sb, 0), vxd = __builtin_amdgcn_raw_buffer_load_b128(rs, off4, sb + colb, 0);
            const u32x4 vth = __builtin_amdgcn_raw_buffer_load_b128(rs, off4, sb + 2u * colb, 0), vthd = __builtin_amdgcn_raw_buffer_load_b128(rs, off4, sb + 3u * colb, 0);
            const u32x4 vc = __builtin_amdgcn_raw_buffer_load_b128(rs, off4, sb + 4u * colb, 0);
            s[0] = {as_f32(vx.x), as_f32(vxd.x), as_f32(vth.x), as_f32(vthd.x), vc.x}; s[1] = {as_f32(vx.y), as_f32(vxd.y), as_f32(vth.y), as_f32(vthd.y), vc.y};
            s[2] = {as_f32(vx.z), as_f32(vxd.z), as_f32(vth.z), as_f32(vthd.z), vc.z}; s[3] = {as_f32(vx.w), as_f32(vxd.w), as_f32(vth.w), as_f32(vthd.w), vc.w};
        }
        const uint64_t wave_first = base + (uint64_t)(threadIdx.x & ~63) * 4;
        Philox4 bits{};  // POLICY == ROLL_ACT_UNIFORM: 128 policy bits = 32 steps of this lane's 4 envs
        uint32_t so = sb;  // byte offset of (step t, this pass) in a [K][n] word buffer; byte buffers use so / 4
        for (int t = 0; t < K; ++t, so += nb4) {
            uint32_t a[4] = {0u, 0u, 0u, 0u}, dn[4], tr[4];
            float r[4];
            if constexpr (POLICY == ROLL_ACT_TABLE) {
                if (in) { const u32x4 va = __builtin_amdgcn_raw_buffer_load_b128(ra, off4, so, 2); a[0] = va.x; a[1] = va.y; a[2] = va.z; a[3] = va.w; }
            } else if constexpr (roll_act_is_mlp(POLICY) || roll_act_is_mlp2(POLICY)) {
                // hidden-layer policy of either depth on the observations the lane's four envs hold before the step (policy.h: net, activation and head; the
                // heads that draw take one Philox evaluation per lane per step, its four words for the lane's four envs — policy_call: the caller's call word)
                static_assert(roll_act_discrete_takes(POLICY), "CartPole has discrete actions: no Gaussian draw");
                const float o[4][4] = {{s[0].x, s[0].xd, s[0].th, s[0].thd}, {s[1].x, s[1].xd, s[1].th, s[1].thd}, {s[2].x, s[2].xd, s[2].th, s[2].thd}, {s[3].x, s[3].xd, s[3].th, s[3].thd}};
                if constexpr (roll_act_is_mlp2(POLICY)) {
                    // (written out a second time for one dead initialiser: the two-layer kernels always zeroed their words first, the one-layer ones never did,
                    // and either set allocates its registers otherwise with the other's declaration — DESIGN.md)
                    Philox4 w{};
                    policy_draw<POLICY>(policy_seed, d.env_id_base + i0, policy_call, (uint32_t)t, w);
                    policy_actions4<POLICY, 4, 2>(lin, w.w, 0.0f, o, a, fin...);
                } else {
                    Philox4 w;
                    policy_draw<POLICY>(policy_seed, d.env_id_base + i0, policy_call, (uint32_t)t, w);
                    policy_actions4<POLICY, 4, 2>(lin, w.w, 0.0f, o, a, fin...);
                }
            } else if constexpr (POLICY == ROLL_ACT_LINEAR) {
                // linear policy on the observation the env holds before the step, in the documented order (the file is compiled with -ffp-contract=off)
#pragma unroll
                for (int k = 0; k < 4; ++k) a[k] = ((((lin.w[0] * s[k].x + lin.w[1] * s[k].xd) + lin.w[2] * s[k].th) + lin.w[3] * s[k].thd) + lin.b > 0.0f) ? 1u : 0u;
            } else {
                // uniform random policy: env i takes bit (t % 32) of word (i % 4) of Philox(policy_seed; lane's first
                // global env id, policy_call, SLOT_POLICY + t / 32) — one Philox evaluation per lane per 32 steps
                if ((t & 31) == 0) bits = env_draw(policy_seed, d.env_id_base + i0, policy_call, SLOT_POLICY + (uint32_t)(t >> 5));
#pragma unroll
                for (int k = 0; k < 4; ++k) a[k] = (bits.w[k] >> (t & 31)) & 1u;
            }
            if constexpr (POLICY != ROLL_ACT_TABLE) {
                if (in && act_out) __builtin_amdgcn_raw_buffer_store_b128(u32x4{a[0], a[1], a[2], a[3]}, ra, off4, so, 2);
            }
            cartpole_wave_advance<4, EULER, SB>(s, a, valid, r, dn, tr, bad);
            if constexpr (has_final<Fin...>) {
                if (in) {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (dn[k] | tr[k]) final_store<4>(final_ptr(fin...) + (uint64_t)t * 4 * d.n + i0 + k, d.n, {s[k].x, s[k].xd, s[k].th, s[k].thd});
                }
            }
            // stored after the reset pass: storing reward / done / truncated before it (as cartpole_step_kernel does)
            // made the linear-policy rollout, whose waves rarely reset, 4 % slower
            finished += cartpole_wave_reset<4, RESET>(d, s, valid, dn, tr, wave_first, lds);
            if (in) {
                if (rew) __builtin_amdgcn_raw_buffer_store_b128(u32x4{as_u32(r[0]), as_u32(r[1]), as_u32(r[2]), as_u32(r[3])}, rr, off4, so, 2);
                if (done_out) __builtin_amdgcn_raw_buffer_store_b32(pack_bytes4(dn), rd, lane_env, so >> 2, 2);
                if (trunc_out) __builtin_amdgcn_raw_buffer_store_b32(pack_bytes4(tr), rt, lane_env, so >> 2, 2);
                if (obs_out) {
                    float* o = obs_out + (uint64_t)t * 4 * d.n + i0;
                    nt_store4(o, make_float4(s[0].x, s[1].x, s[2].x, s[3].x)); nt_store4(o + d.n, make_float4(s[0].xd, s[1].xd, s[2].xd, s[3].xd));
                    nt_store4(o + 2 * d.n, make_float4(s[0].th, s[1].th, s[2].th, s[3].th)); nt_store4(o + 3 * d.n, make_float4(s[0].thd, s[1].thd, s[2].thd, s[3].thd));
                }
            }
        }
        if (in) {
            __builtin_amdgcn_raw_buffer_store_b128(u32x4{as_u32(s[0].x), as_u32(s[1].x), as_u32(s[2].x), as_u32(s[3].x)}, rs, off4, sb, kNtAux);
            __builtin_amdgcn_raw_buffer_store_b128(u32x4{as_u32(s[0].xd), as_u32(s[1].xd), as_u32(s[2].xd), as_u32(s[3].xd)}, rs, off4, sb + colb, kNtAux);
            __builtin_amdgcn_raw_buffer_store_b128(u32x4{as_u32(s[0].th), as_u32(s[1].th), as_u32(s[2].th), as_u32(s[3].th)}, rs, off4, sb + 2u * colb, kNtAux);
            __builtin_amdgcn_raw_buffer_store_b128(u32x4{as_u32(s[0].thd), as_u32(s[1].thd), as_u32(s[2].thd), as_u32(s[3].thd)}, rs, off4, sb + 3u * colb, kNtAux);
            __builtin_amdgcn_raw_buffer_store_b128(u32x4{s[0].ctr, s[1].ctr, s[2].ctr, s[3].ctr}, rs, off4, sb + 4u * colb, kNtAux);
        }
    }
    cartpole_flush_counts<kWaves>(d, finished, bad);
}

// Masked reset.  One lane looks at 4 consecutive mask bytes of each mask with a single dword
// load (2 B/env of traffic); masked envs are compacted through LDS, so one pass of the block's first lanes
// evaluates Philox for all of them instead of every wave paying for its one or two masked lanes.
// `all` skips masks and compaction.
__global__ void __launch_bounds__(kBlock)
cartpole_reset_kernel(CartPoleDev d, const uint8_t* __restrict__ m0, const uint8_t* __restrict__ m1, int all,
                      int masks_aligned, float* __restrict__ obs_out) {
    __shared__ uint32_t count;
    __shared__ uint16_t idx[kBlock * 4];
    constexpr uint64_t kPerBlock = (uint64_t)kBlock * 4;
    for (uint64_t base = (uint64_t)blockIdx.x * kPerBlock; base < d.n; base += (uint64_t)gridDim.x * kPerBlock) {
        const uint64_t i0 = base + (uint64_t)threadIdx.x * 4;
        uint32_t m = 0;
        if (i0 < d.n) {
            if (all) {
                m = 0x01010101u;
            } else if (masks_aligned && i0 + 4 <= d.n) {
                if (m0) m |= *reinterpret_cast<const uint32_t*>(m0 + i0);
                if (m1) m |= *reinterpret_cast<const uint32_t*>(m1 + i0);
            } else {
                for (int k = 0; k < 4 && i0 + k < d.n; ++k) {
                    uint32_t b = 0;
                    if (m0) b |= m0[i0 + k];
                    if (m1) b |= m1[i0 + k];
                    m |= (b ? 1u : 0u) << (8 * k);
                }
            }
        }
        uint32_t cnt;
        if (all) {
            cnt = (uint32_t)((d.n - base) < kPerBlock ? (d.n - base) : kPerBlock);
        } else {
            if (threadIdx.x == 0) count = 0;
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (i0 + k < d.n && ((m >> (8 * k)) & 0xffu)) idx[atomicAdd(&count, 1u)] = (uint16_t)(threadIdx.x * 4 + k);
            __syncthreads();
            cnt = count;
        }
        for (uint32_t j = threadIdx.x; j < cnt; j += kBlock) {
            const uint64_t i = base + (all ? j : (uint32_t)idx[j]);
            const uint32_t c = d.ctr()[i];
            float f[4];
            cartpole_draw(d.seed, d.env_id_base + i, c >> kCpEpShift, f);
            d.x()[i] = f[0]; d.xd()[i] = f[1]; d.th()[i] = f[2]; d.thd()[i] = f[3]; d.ctr()[i] = cp_ctr_after_reset(c);
            if (obs_out) {
                obs_out[i] = f[0]; obs_out[d.n + i] = f[1]; obs_out[2 * d.n + i] = f[2]; obs_out[3 * d.n + i] = f[3];
            }
        }
        if (!all) __syncthreads();  // idx/count are reused by the next iteration
    }
}

// blob <-> engine columns (steps / sbt / episode are separate blob columns; saturations as in cartpole_step.h)
__global__ void cartpole_export_kernel(CartPoleDev d, uint32_t* __restrict__ blob) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.n) return;
    blob[0 * d.n + i] = as_u32(d.x()[i]);
    blob[1 * d.n + i] = as_u32(d.xd()[i]);
    blob[2 * d.n + i] = as_u32(d.th()[i]);
    blob[3 * d.n + i] = as_u32(d.thd()[i]);
    uint32_t c = d.ctr()[i];
    blob[4 * d.n + i] = c & kCpStepsMask;
    blob[5 * d.n + i] = (uint32_t)((int32_t)((c >> kCpSbtShift) & kCpSbtMask) - 1);  // -1 = None
    blob[6 * d.n + i] = c >> kCpEpShift;
}

__global__ void cartpole_import_kernel(CartPoleDev d, const uint32_t* __restrict__ blob) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.n) return;
    d.x()[i] = as_f32(blob[0 * d.n + i]);
    d.xd()[i] = as_f32(blob[1 * d.n + i]);
    d.th()[i] = as_f32(blob[2 * d.n + i]);
    d.thd()[i] = as_f32(blob[3 * d.n + i]);
    int32_t sbt = (int32_t)blob[5 * d.n + i];
    d.ctr()[i] = cp_ctr_pack(blob[4 * d.n + i], sbt < 0 ? 0u : (uint32_t)sbt + 1u, blob[6 * d.n + i]);
}

struct CartPoleEnv final : Env {
    void* base = nullptr;
    CartPoleDev dev{};
    bool auto_reset = false;
    int step_block = getenv("MGYM_CARTPOLE_BLOCK") ? atoi(getenv("MGYM_CARTPOLE_BLOCK")) : kBlock;  // threads per block of the step kernel (tuning knob)
    int max_blocks = classic_max_blocks(kMaxBlocks);   // block cap of the step kernel, in kBlock-sized blocks (MGYM_CLASSIC_MAX_BLOCKS lowers it)

    ~CartPoleEnv() override {
        if (base) (void)hipFree(base);
    }

    int init() override {
        obs_dim = 4;
        state_cols = 7;
        if (n > (1ull << 27)) {  // the step kernel addresses the five columns with 32-bit byte offsets from one buffer resource
            set_last_error("mgym_create: a CartPole handle holds at most 134 217 728 environments (shard larger populations over handles)");
            return MGYM_ERR_BAD_ARG;
        }
        MGYM_HIP(hipMalloc(&base, 5 * n_pad * sizeof(float)));
        MGYM_HIP(hipMemsetAsync(base, 0, 5 * n_pad * sizeof(float), stream));
        dev.base = static_cast<float*>(base);
        dev.n_pad = n_pad;
        dev.n = n;
        dev.seed = cfg.seed;
        dev.env_id_base = cfg.env_id_base;
        dev.err = d_err;
        dev.done_count = d_done;
        auto_reset = (cfg.flags & MGYM_FLAG_AUTO_RESET) != 0;
        // cartpole.rs:81: steps_beyond_terminated = Some(0) at construction
        if (n) MGYM_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(dev.ctr()), cp_ctr_pack(0u, 1u, 0u), n, stream));
        return MGYM_OK;
    }

    int reset(const uint8_t* m0, const uint8_t* m1, bool all, float* obs_out) override { return launch_reset(cartpole_reset_kernel, dev, m0, m1, all, obs_out); }

    int reset_deterministic(float* obs_out) override {  // cartpole.rs:437-442: self.reset()? then state = zeros
        int st = reset(nullptr, nullptr, true, nullptr);
        if (st != MGYM_OK || n == 0) return st;
        MGYM_HIP(hipMemsetAsync(dev.x(), 0, 4 * n_pad * sizeof(float), stream));
        if (obs_out) MGYM_HIP(hipMemsetAsync(obs_out, 0, 4 * n * sizeof(float), stream));
        return MGYM_OK;
    }

    template <int VEC, bool RESET, int BLK, class... Fin>
    void launch_step_blk(const uint32_t* act, float* obs_out, float* reward, uint8_t* done, uint8_t* trunc, Fin... fin) {
        const uint64_t nb = (n + (uint64_t)BLK * VEC - 1) / ((uint64_t)BLK * VEC);   // tiles (n > 0)
        const uint64_t cap = (uint64_t)max_blocks * kBlock / BLK;   // same thread count as the kBlock-sized cap
        const bool one = nb <= cap;                                 // one block per tile: the single-pass form
        dim3 g((unsigned)(one ? nb : cap)), b(BLK);
        with_bools([&](auto E, auto S, auto O) {
            hipLaunchKernelGGL((cartpole_step_kernel<VEC, decltype(E)::value, decltype(S)::value, RESET, BLK, decltype(O)::value, Fin...>), g, b, 0, stream, dev.base,
                               (uint32_t)dev.n_pad, (uint32_t)dev.n, act, dev.seed, dev.env_id_base, dev.err, dev.done_count, obs_out, reward, done, trunc, fin...);
        }, cfg.is_euler, cfg.sutton_barto_reward, one);
    }
    template <int VEC, bool RESET>
    void launch_step(const uint32_t* act, float* obs_out, float* reward, uint8_t* done, uint8_t* trunc) {
        if constexpr (RESET) {
            if (final_obs) { launch_step_blk<VEC, true, kBlock>(act, obs_out, reward, done, trunc, final_obs); return; }   // (mgym_set_final_obs_out; the block-size knob is not offered there)
        }
        if (VEC == 4 && step_block == 64) launch_step_blk<VEC, RESET, 64>(act, obs_out, reward, done, trunc);
        else if (VEC == 4 && step_block == 128) launch_step_blk<VEC, RESET, 128>(act, obs_out, reward, done, trunc);
        else launch_step_blk<VEC, RESET, kBlock>(act, obs_out, reward, done, trunc);
    }

    int step(const void* actions, float* obs_out, float* reward, uint8_t* done, uint8_t* trunc) override {
        if (n == 0) return MGYM_OK;
        const uint32_t* act = static_cast<const uint32_t*>(actions);
        const bool vec_ok = fused_rollout_args_ok(nullptr, n, 0, false, act, obs_out, reward, done, trunc);   // else one environment per lane
        with_bools([&](auto V, auto R) { launch_step<decltype(V)::value ? 4 : 1, decltype(R)::value>(act, obs_out, reward, done, trunc); }, vec_ok, auto_reset);
        MGYM_HIP(hipGetLastError());
        return MGYM_OK;
    }

    // the one launch of the fused rollout kernel with the action source POLICY; `lin`: the linear words or the hidden-layer pack, `uni`: the policy seed and call
    // word of a drawing source; `net`: a two-hidden-layer source's Mlp2Net, the head of the kernel's trailing pack
    template <int POLICY, class... Net>
    void launch_rollout(const uint32_t* act, uint32_t* act_out, int K, float* obs_out, float* reward, uint8_t* done, uint8_t* trunc, const PolicyArg<POLICY, 4, 2, LinearPolicy>& lin, UniformDraw uni,
                        Net... net) {
        const dim3 g(grid_for(n / 4)), b(kBlock);
        if (final_obs) {   // (an auto-reset handle: mgym_set_final_obs_out)
            with_bools([&](auto E, auto S) {
                hipLaunchKernelGGL((cartpole_rollout_kernel<decltype(E)::value, decltype(S)::value, true, POLICY, Net..., float*>), g, b, 0, stream, dev, act, act_out, uni.seed, uni.call, lin, K,
                                   obs_out, reward, done, trunc, net..., final_obs);
            }, cfg.is_euler, cfg.sutton_barto_reward);
            return;
        }
        with_bools([&](auto E, auto S, auto R) {
            hipLaunchKernelGGL((cartpole_rollout_kernel<decltype(E)::value, decltype(S)::value, decltype(R)::value, POLICY, Net...>), g, b, 0, stream, dev, act, act_out, uni.seed, uni.call, lin, K,
                               obs_out, reward, done, trunc, net...);
        }, cfg.is_euler, cfg.sutton_barto_reward, auto_reset);
    }

    int rollout(const void* actions, int K, float* obs_out, float* reward, uint8_t* done, uint8_t* trunc) override {
        if (n == 0 || K == 0) return MGYM_OK;
        const uint32_t* act = static_cast<const uint32_t*>(actions);
        if (!fused_rollout_args_ok(nullptr, n, K, true, act, obs_out, reward, done, trunc)) return Env::rollout(actions, K, obs_out, reward, done, trunc);  // K plain steps
        launch_rollout<ROLL_ACT_TABLE>(act, nullptr, K, obs_out, reward, done, trunc, LinearPolicy{}, UniformDraw{});
        MGYM_HIP(hipGetLastError());
        return MGYM_OK;
    }

    int rollout_policy(const PolicyCall& call, int K, void* actions_out, float* obs_out, float* reward, uint8_t* done, uint8_t* trunc) override {
        return rollout_policy_classic<4, 2, roll_act_discrete_takes>(call, K, actions_out, obs_out, reward, done, trunc, true, nullptr,
            [](const float* w) { return LinearPolicy{{w[0], w[1], w[2], w[3]}, w[4]}; },
            [&](auto S, const auto& arg, auto... draw_net) { launch_rollout<decltype(S)::value>(nullptr, static_cast<uint32_t*>(actions_out), K, obs_out, reward, done, trunc, arg, draw_net...); });
    }

    int observation(const float** obs, uint64_t* col_stride) override {
        *obs = dev.x();
        *col_stride = n_pad;
        return MGYM_OK;
    }

    int get_state(void* blob) override { return launch_per_env(cartpole_export_kernel, dev, static_cast<uint32_t*>(blob)); }
    int set_state(const void* blob) override { return launch_per_env(cartpole_import_kernel, dev, static_cast<const uint32_t*>(blob)); }
};

Env* make_cartpole() { return new CartPoleEnv(); }

}  // namespace mgym
