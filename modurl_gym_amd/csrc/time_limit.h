// time_limit.h — the episode time limit (mgym_config::max_episode_steps): count, compare, saturate.
//
// Not in the reference: its MountainCarV0 and LunarLanderV3 never truncate (mountain_car.rs:324-329, lunar_lander.rs:1165); this is
// gymnasium's TimeLimit rule — after a step has produced its observation, reward and `done` exactly as without a limit,
// elapsed += 1 and truncated = elapsed >= limit; `done` is not changed, so both flags can be set on one step.
// Plain C++ like ll_env.h, so the kernels (mountain_car.hip, lunar_lander.hip, ll_roll.h) and the host check
// tests/native/time_limit_check.cpp compile the SAME lines.
#pragma once
#include <stdint.h>

#ifndef __HIPCC__
#ifndef __device__
#define __device__
#endif
#ifndef __forceinline__
#define __forceinline__ inline
#endif
#endif

namespace mgym {

constexpr uint32_t kMaxEpisodeSteps = 65535u;   // the largest limit mgym_create accepts: MountainCar keeps `elapsed` in 16 bits per env

// MountainCar's counter after one more caller-visible step: saturates at 65535, never wraps (an environment stepped past its limit
// without a reset keeps reporting truncated = 1)
__device__ __forceinline__ uint32_t tl_advance(uint32_t elapsed) { return elapsed < kMaxEpisodeSteps ? elapsed + 1u : kMaxEpisodeSteps; }

// truncated, from the count INCLUDING the step just taken (limit 0: off).  >=, not ==: past the limit the flag stays up
__device__ __forceinline__ uint32_t tl_truncated(uint32_t limit, uint32_t elapsed) { return (limit != 0u && elapsed >= limit) ? 1u : 0u; }

// mgym_set_elapsed_steps on a 16-bit counter: larger values are clamped
__device__ __forceinline__ uint32_t tl_clamp(uint32_t elapsed) { return elapsed < kMaxEpisodeSteps ? elapsed : kMaxEpisodeSteps; }

// LunarLander counts in EnvRegs::step (ll_env.h), which is 1 after reset() — its implicit step(0), lunar_lander.rs:911-916, is not a
// caller-visible step — and has already been advanced by ll_post_step when the flags are written: elapsed = step - 1
__device__ __forceinline__ uint32_t tl_ll_elapsed(uint32_t step_after) { return step_after != 0u ? step_after - 1u : 0u; }
__device__ __forceinline__ uint32_t tl_ll_truncated(uint32_t limit, uint32_t step_after) { return tl_truncated(limit, tl_ll_elapsed(step_after)); }

}  // namespace mgym
