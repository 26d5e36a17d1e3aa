// soa4.h — device helpers of the struct-of-arrays kernels in which one lane owns 4 consecutive environments (cartpole.hip, mountain_car.hip,
// pendulum.hip, acrobot.hip): every column is read and written with one 16-byte access per lane, the 4 done bytes with one word.  The elapsed
// counters, the wave's count flush and the reset mask gather below are those of the last three (CartPole keeps its own: DESIGN.md §4).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "common.h"

namespace mgym {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint16_t u16x4 __attribute__((ext_vector_type(4)));

// 16-byte access at (uniform base pointer) + (32-bit per-lane byte offset): lowers to global_load/store with the
// base in SGPRs and the lane offset in one VGPR (no 64-bit per-lane address arithmetic, which was ~90 VALU
// instructions per wave pass when every column address was formed per lane)
template <typename T> __device__ __forceinline__ const T* at(const void* base, uint32_t byte_off) {
    return reinterpret_cast<const T*>(static_cast<const char*>(base) + byte_off);
}
template <typename T> __device__ __forceinline__ T* at(void* base, uint32_t byte_off) {
    return reinterpret_cast<T*>(static_cast<char*>(base) + byte_off);
}

// Non-temporal 16-byte store of a lane's four floats.  Outputs are written once and not read again by the
// kernel: non-temporal stores took the CartPole step from 11.4 us to 10.9 us at 1 Mi envs (round 1).
__device__ __forceinline__ void nt_store4(float* p, float4 v) {
    f32x4 w = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(w, reinterpret_cast<f32x4*>(p));
}

// Block cap of the classic step kernels, in kBlock-sized blocks: `compiled` (kMaxBlocks), or MGYM_CLASSIC_MAX_BLOCKS when that is lower (tuning
// knob, read when a handle is created).  A population of no more tiles than the cap is stepped in the single-pass form (one block per tile), a
// larger one in the grid-stride form: the knob brings the grid-stride form within reach of a few thousand environments.
inline int classic_max_blocks(int compiled) {
    const char* s = getenv("MGYM_CLASSIC_MAX_BLOCKS");
    const int v = s ? atoi(s) : compiled;
    return v < 1 ? 1 : (v > compiled ? compiled : v);
}

// a lane's four flags (0 / 1 each) as the four bytes of one word, environment k in byte k
__device__ __forceinline__ uint32_t pack_bytes4(const uint32_t (&b)[4]) { return b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24); }

// a lane's four elapsed counters (u16 each): one 8-byte access (i0 a multiple of 4)
__device__ __forceinline__ void load_elapsed4(const uint16_t* elapsed, uint64_t i0, uint32_t (&el)[4]) {
    const u16x4 v = *reinterpret_cast<const u16x4*>(elapsed + i0);
    el[0] = v.x; el[1] = v.y; el[2] = v.z; el[3] = v.w;
}
__device__ __forceinline__ void store_elapsed4(uint16_t* elapsed, uint64_t i0, const uint32_t (&el)[4]) {
    __builtin_nontemporal_store(u16x4{(uint16_t)el[0], (uint16_t)el[1], (uint16_t)el[2], (uint16_t)el[3]}, reinterpret_cast<u16x4*>(elapsed + i0));
}

// per-lane counts of finished envs summed over the wave, one fire-and-forget atomic per wave; the sticky invalid-action bit.  (The step4 kernels
// count with __ballot and keep their tail written out: a helper shared with this one moved instructions in them.)
__device__ __forceinline__ void flush_counts(unsigned long long* done_count, uint32_t* err, uint32_t finished, bool bad) {
    for (int o = 32; o > 0; o >>= 1) finished += __shfl_down(finished, o);
    if ((threadIdx.x & 63) == 0 && finished)
        atomicAdd(done_count + ((blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) & (kDoneShards - 1)), (unsigned long long)finished);
    if (__any(bad)) {
        if ((threadIdx.x & 63) == 0) atomicOr(err, DEV_ERR_INVALID_ACTION);
    }
}

// mgym_reset / mgym_reset_done: the mask word of the lane's four envs i0 .. i0 + 3, env k in byte k (nonzero: reset it) — every env (`all`), or the
// OR of the caller's byte masks m0 and m1 (either may be null): one word each where both are 4-byte aligned and the group is whole, bytes otherwise
__device__ __forceinline__ uint32_t reset_mask4(const uint8_t* m0, const uint8_t* m1, int all, int masks_aligned, uint64_t i0, uint64_t n) {
    uint32_t m = 0;
    if (all) {
        m = 0x01010101u;
    } else if (masks_aligned && i0 + 4 <= n) {
        if (m0) m |= *reinterpret_cast<const uint32_t*>(m0 + i0);
        if (m1) m |= *reinterpret_cast<const uint32_t*>(m1 + i0);
    } else {
        for (int k = 0; k < 4 && i0 + k < n; ++k) {
            uint32_t b = 0;
            if (m0) b |= m0[i0 + k];
            if (m1) b |= m1[i0 + k];
            m |= (b ? 1u : 0u) << (8 * k);
        }
    }
    return m;
}

// mgym_set_final_obs_out.  The stepping kernels end their template parameters with `class... Fin` and their arguments with `Fin... fin`: the pack is
// empty (the kernel as it always was: same arguments, same code) or one float* (the channel's instantiation, launched only while a pointer is set).
// The rollout kernels of the two-hidden-layer sources (mgym_rollout_mlp2) take their Mlp2Net at the head of the same pack, before the channel's pointer:
// what a newer source adds to the argument list travels there, so every instantiation from before it keeps its arguments, its code and its name
// (policy.h's mlp2_net_of reads it).
template <class... Fin> constexpr bool has_final = (std::is_same_v<Fin, float*> || ...);
__device__ __forceinline__ float* final_ptr() { return nullptr; }
__device__ __forceinline__ float* final_ptr(float* p) { return p; }
template <int D, int A> __device__ __forceinline__ float* final_ptr(const Mlp2Net<D, A>&) { return nullptr; }
template <int D, int A> __device__ __forceinline__ float* final_ptr(const Mlp2Net<D, A>&, float* p) { return p; }
// the D observation words of one finished environment, column k at fin + k * n — sparse 4-byte stores by the owning lane,
// made after the physics and before the fused reset replaces the registers.  `fin` points at the step's [D][n] slab, at the env's column.
// Plain stores, not non-temporal ones like the dense outputs: measured at 1 Mi CartPole envs, the K = 16 uniform rollout with the channel set costs
// +28 % with plain stores against +145 % with non-temporal ones (mgym_step: the same either way) — DESIGN.md §5b-2.
template <int D>
__device__ __forceinline__ void final_store(float* fin, uint64_t n, const float (&o)[D]) {
#pragma unroll
    for (int k = 0; k < D; ++k) fin[(uint64_t)k * n] = o[k];
}

}  // namespace mgym
