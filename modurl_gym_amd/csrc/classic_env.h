// classic_env.h — the host side MountainCar, Pendulum and Acrobot share (mountain_car.hip, pendulum.hip, acrobot.hip): the engine's columns and
// elapsed counts, the launch geometry of their kernels, and the entry points that do not depend on a family's Dev struct or kernels.
#pragma once
#include "common.h"
#include "soa4.h"

namespace mgym {

struct ClassicEnv : Env {
    float* cols = nullptr;       // the family's f32 / u32 columns, n_pad words apart; the observation's come first (mgym_observation is a view of them)
    uint16_t* el_col = nullptr;  // elapsed[n_pad]
    int max_blocks = classic_max_blocks(kMaxBlocks);  // block cap of the 16-byte step kernel (MGYM_CLASSIC_MAX_BLOCKS lowers it)

    ~ClassicEnv() override;
    int alloc(int ncols);   // (init) `ncols` columns and the elapsed counts, zeroed on the stream
    // (init) the fields every family's Dev struct holds under the same names
    template <class Dev>
    void fill_common(Dev& d) const {
        d.n = n; d.seed = cfg.seed; d.env_id_base = cfg.env_id_base; d.err = d_err; d.done_count = d_done;
        d.auto_reset = (cfg.flags & MGYM_FLAG_AUTO_RESET) ? 1 : 0;
        d.elapsed = el_col; d.limit = cfg.max_episode_steps;
    }
    int elapsed(uint32_t* out, const uint32_t* in) override;
    int observation(const float** obs, uint64_t* col_stride) override { *obs = cols; *col_stride = n_pad; return MGYM_OK; }

    // mgym_rollout: the family's fused kernel where the call allows it (rollout_table launches it with ROLL_ACT_TABLE), K plain steps otherwise
    int rollout(const void* actions, int K, float* obs_out, float* reward, uint8_t* done, uint8_t* trunc) override {
        if (n == 0 || K == 0) return MGYM_OK;
        if (!fused_rollout_args_ok(nullptr, n, K, false, actions, obs_out, reward, done, trunc)) return Env::rollout(actions, K, obs_out, reward, done, trunc);
        rollout_table(static_cast<const uint32_t*>(actions), K, obs_out, reward, done, trunc);
        MGYM_HIP(hipGetLastError());
        return MGYM_OK;
    }
    virtual void rollout_table(const uint32_t* act, int K, float* obs_out, float* reward, uint8_t* done, uint8_t* trunc) = 0;

    // one thread per environment: export, import, zero
    template <class Kernel, class... Args>
    int launch_per_env(Kernel kernel, Args... args) {
        if (n == 0) return MGYM_OK;
        hipLaunchKernelGGL(kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, args...);
        MGYM_HIP(hipGetLastError());
        return MGYM_OK;
    }
    // a family's reset kernel (Dev, m0, m1, all, masks_aligned, obs_out), one lane per group of 4 environments
    template <class Kernel, class Dev>
    int launch_reset(Kernel kernel, const Dev& dev, const uint8_t* m0, const uint8_t* m1, bool all, float* obs_out) {
        if (n == 0) return MGYM_OK;
        hipLaunchKernelGGL(kernel, dim3(grid_for((n + 3) / 4)), dim3(kBlock), 0, stream, dev, m0, m1, all ? 1 : 0, aligned(m0, 4) && aligned(m1, 4) ? 1 : 0, obs_out);
        MGYM_HIP(hipGetLastError());
        return MGYM_OK;
    }

    // the caller's buffers allow 16-byte accesses (the VEC = 4 kernels; with n % 4 == 0 and n within the family's bound, the step4 kernel)
    bool vec_ok(const void* act, const float* obs_out, const float* reward, const uint8_t* done, const uint8_t* trunc) const {
        return aligned(act, 16) && aligned(reward, 16) && aligned(done, 4) && aligned(trunc, 4) && (obs_out == nullptr || (aligned(obs_out, 16) && n % 4 == 0));
    }
    // the step4 kernel's grid: one block per tile of 4 * kBlock environments — the single-pass form (returns true) — while the block cap allows,
    // max_blocks blocks in the grid-stride form beyond
    bool step4_grid(dim3& g) const {
        const uint64_t nb = (n + 4 * kBlock - 1) / (4 * kBlock);
        const bool one = nb <= (uint64_t)max_blocks;
        g = dim3((unsigned)(one ? nb : (uint64_t)max_blocks));
        return one;
    }
};

}  // namespace mgym
