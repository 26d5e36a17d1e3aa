// classic_env.h — the host side MountainCar, Pendulum and Acrobot share (mountain_car.hip, pendulum.hip, acrobot.hip): the engine's columns and
// elapsed counts, the one step launch (launch_step: kernel, grid and form; a family names its two kernels), and the entry points that do not depend on
// a family's Dev struct or kernels.
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
    uint64_t step4_max = 1ull << 27;   // the largest population the family's step4 kernel addresses (Acrobot: 2^26)
    // the channel of mgym_set_final_obs_out has something to deliver (only auto-reset handles hold a pointer)
    virtual bool final_live() const { return final_obs != nullptr; }

    // step() of the three families: the choice of kernel and grid, and the run-time bools as std::bool_constant arguments of the family's two launches.
    // `step4(grid, RESET, TL, ONE, fin...)` names its structured 16-byte kernel, `step1(grid, VEC4, TL, fin...)` its generic one; fin... is final_obs
    // where the channel is live (then RESET is on: only auto-reset handles hold a pointer) and nothing otherwise.
    template <class Step4, class Step1>
    int launch_step(const void* act, const float* obs_out, const float* reward, const uint8_t* done, const uint8_t* trunc, Step4&& step4, Step1&& step1) {
        if (n == 0) return MGYM_OK;
        const bool vec = vec_ok(act, obs_out, reward, done, trunc), tl = cfg.max_episode_steps != 0u, fin = final_live();
        const dim3 gv(grid_for((n + 3) / 4)), gs(grid_for(n));
        if (vec && n % 4 == 0 && n <= step4_max) {  // the structured 16-byte kernel
            dim3 g;
            const bool one = step4_grid(g);
            if (fin) with_bools([&](auto T, auto O) { step4(g, std::true_type{}, T, O, final_obs); }, tl, one);
            else with_bools([&](auto R, auto T, auto O) { step4(g, R, T, O); }, (cfg.flags & MGYM_FLAG_AUTO_RESET) != 0, tl, one);
        } else if (fin) {
            with_bools([&](auto T, auto V) { step1(decltype(V)::value ? gv : gs, V, T, final_obs); }, tl, vec);
        } else {
            with_bools([&](auto T, auto V) { step1(decltype(V)::value ? gv : gs, V, T); }, tl, vec);
        }
        MGYM_HIP(hipGetLastError());
        return MGYM_OK;
    }
};

}  // namespace mgym
