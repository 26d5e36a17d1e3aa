// ll_roll.hip — the persistent launch of mgym_rollout for LunarLanderV3 (ll_roll.h) as a translation unit of its own, with the host entry
// points lunar_lander.hip calls.  Replaces K consecutive calls of `impl Gym for LunarLanderV3`::step (reference src/box_2d/lunar_lander.rs:919-1167).
#include "ll_roll.h"

namespace mgym {

int ll_rollout_blocks_per_cu(int* per_cu) {
    MGYM_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, ll_rollout_kernel<32>, 64, 0));
    return MGYM_OK;
}
void ll_rollout_ring_init(hipStream_t s, const RollQ& q) { hipLaunchKernelGGL(ll_rollout_ring_init_kernel, dim3(256), dim3(256), 0, s, q); }
void ll_rollout_begin(hipStream_t s, const RollQ& q, uint32_t n) { hipLaunchKernelGGL(ll_rollout_begin_kernel, dim3(1), dim3(64), 0, s, q, n); }
void ll_rollout_launch(hipStream_t s, unsigned grid, const LLDev& d, const LLIo& io, const RollQ& q) {
    hipLaunchKernelGGL(ll_rollout_kernel<32>, dim3(grid), dim3(64), 0, s, d, io, q);
}
// mgym_rollout_linear / mgym_rollout_uniform / mgym_rollout_mlp: the same launch with the action source `policy` (ll_roll_types.h), never with helper waves.
// *per_cu: resident blocks of the linear and uniform forms; *mlp_per_cu: of the hidden-layer forms, which get a grid of their own so that their register
// and scratch needs never change the grid of the other two.
int ll_rollout_policy_blocks_per_cu(int* per_cu, int* mlp_per_cu) {
    int a = 0, b = 0, c = 0, e = 0;
    MGYM_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, ll_rollout_kernel<32, ROLL_ACT_LINEAR, RollPolicy>, 64, 0));
    MGYM_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, ll_rollout_kernel<32, ROLL_ACT_UNIFORM, RollPolicy>, 64, 0));
    MGYM_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&c, ll_rollout_kernel<32, ROLL_ACT_MLP_RELU, RollPolicy>, 64, 0));
    MGYM_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&e, ll_rollout_kernel<32, ROLL_ACT_MLP_TANH, RollPolicy>, 64, 0));
    *per_cu = a < b ? a : b;
    *mlp_per_cu = c < e ? c : e;
    return MGYM_OK;
}
// every instantiation's by-value arguments fit the 4 KiB kernel-argument segment the launch can rely on (the hidden-layer pack is NOT among them)
static_assert(sizeof(LLDev) + sizeof(LLIo) + sizeof(RollQ) + sizeof(RollPolicy) <= 4096, "ll_rollout_kernel: by-value kernel arguments above 4096 bytes");
void ll_rollout_policy_launch(hipStream_t s, unsigned grid, const LLDev& d, const LLIo& io, const RollQ& q, const RollPolicy& pol, int policy) {
    with_policy_source([&](auto S) {   // the four sources the persistent launch carries: no other is instantiated, and none reaches this call
        constexpr int SRC = decltype(S)::value;
        if constexpr (SRC == ROLL_ACT_LINEAR || SRC == ROLL_ACT_UNIFORM || SRC == ROLL_ACT_MLP_RELU || SRC == ROLL_ACT_MLP_TANH)
            hipLaunchKernelGGL((ll_rollout_kernel<32, SRC, RollPolicy>), dim3(grid), dim3(64), 0, s, d, io, q, pol);
    }, policy);
}
// the handle's weight pack, stored on the stream ahead of the launch that reads it: the caller's array is read during the call only (it travels in this
// kernel's arguments), and consecutive calls on one stream each find their own weights
__global__ void __launch_bounds__(256) ll_rollout_mlp_pack_kernel(LLMlpPack pack, uint32_t* __restrict__ dst) {
    static_assert(sizeof(LLMlpPack) % 4 == 0, "copied word by word");
    const uint32_t* const src = reinterpret_cast<const uint32_t*>(&pack);
    for (uint32_t w = threadIdx.x; w < (uint32_t)(sizeof(LLMlpPack) / 4); w += blockDim.x) dst[w] = src[w];
}
void ll_rollout_mlp_pack_store(hipStream_t s, const LLMlpPack& pack, LLMlpPack* dst) {
    hipLaunchKernelGGL(ll_rollout_mlp_pack_kernel, dim3(1), dim3(256), 0, s, pack, reinterpret_cast<uint32_t*>(dst));
}
void ll_rollout_helper_launch(hipStream_t s, unsigned grid, const LLDev& d, const LLIo& io, const RollQ& q) {
    hipLaunchKernelGGL(ll_rollout_free_kernel<32>, dim3(grid), dim3(64), 0, s, d, io, q);
}

}  // namespace mgym
