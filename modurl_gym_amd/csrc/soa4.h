// soa4.h — device helpers of the struct-of-arrays kernels in which one lane owns 4 consecutive environments (cartpole.hip, mountain_car.hip):
// every column is read and written with one 16-byte access per lane, the 4 done bytes with one word.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

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

// mgym_set_final_obs_out.  The stepping kernels end their template parameters with `class... Fin` and their arguments with `Fin... fin`: the pack is
// empty (the kernel as it always was: same arguments, same code) or one float* (the channel's instantiation, launched only while a pointer is set).
template <class... Fin> constexpr bool has_final = sizeof...(Fin) == 1;
__device__ __forceinline__ float* final_ptr() { return nullptr; }
__device__ __forceinline__ float* final_ptr(float* p) { return p; }
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
