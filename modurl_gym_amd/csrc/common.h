// common.h — engine-internal declarations shared by the kernels' host wrappers and the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <type_traits>
#include "../../include/mgym.h"
#include "policy.h"

namespace mgym {

void set_last_error(const std::string& msg);
int hip_fail(hipError_t e, const char* what, const char* file, int line);

#define MGYM_HIP(expr)                                                        \
    do {                                                                      \
        hipError_t _e = (expr);                                               \
        if (_e != hipSuccess) return ::mgym::hip_fail(_e, #expr, __FILE__, __LINE__); \
    } while (0)

constexpr int kBlock = 256;          // 4 waves of 64
constexpr int kDoneShards = 256;     // per-handle finished-episode counter: partial sums, one fire-and-forget atomic per wave
constexpr int kMaxBlocks = 8192;     // grid-stride beyond this (measured best of 2048/4096/8192/uncapped at 32 Mi envs)

inline uint64_t round_up(uint64_t v, uint64_t m) { return (v + m - 1) / m * m; }
inline bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
inline int grid_for(uint64_t work_items) {
    uint64_t b = (work_items + kBlock - 1) / kBlock;
    if (b < 1) b = 1;
    if (b > (uint64_t)kMaxBlocks) b = kMaxBlocks;
    return (int)b;
}

// The one way from run-time bools to template arguments: with_bools(f, b0, b1, ..) calls the generic lambda f with one std::bool_constant
// per bool, f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ..) — every combination is instantiated, the matching one runs.
template <class F>
void with_bools(F&& f) { f(); }
template <class F, class... Rest>
void with_bools(F&& f, bool b, Rest... rest) {
    if (b) with_bools([&](auto... c) { f(std::true_type{}, c...); }, rest...);
    else with_bools([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

// What the fused rollout kernels of the classic families (one lane owns 4 consecutive environments, 16-byte accesses) ask of a call.
// `bound32`: the kernel addresses [K][n] word buffers with 32-bit byte offsets (CartPole).  `api`: the entry point named in the error
// message, or null for a caller that falls back to K plain steps instead of failing (mgym_rollout).
inline bool fused_rollout_args_ok(const char* api, uint64_t n, int K, bool bound32, const void* actions, const float* obs, const float* reward,
                                  const uint8_t* done, const uint8_t* trunc) {
    const bool ok = n % 4 == 0 && aligned(actions, 16) && aligned(reward, 16) && aligned(done, 4) && aligned(trunc, 4) && aligned(obs, 16) &&
                    (!bound32 || (uint64_t)K * n * 4 < (1ull << 32));
    if (!ok && api)
        set_last_error(std::string(api) + (bound32 ? ": n_envs must be a multiple of 4, the buffers 16-byte aligned, and K * n_envs below 2^30"
                                                   : ": n_envs must be a multiple of 4 and the buffers 16-byte aligned"));
    return ok;
}

// device-side sticky status bits (OR-ed into Env::d_err)
enum : uint32_t { DEV_ERR_INVALID_ACTION = 1u, DEV_ERR_NOT_RESET = 2u, DEV_ERR_CONTACT_OVERFLOW = 4u, DEV_ERR_SOLVER_OVERFLOW = 8u, DEV_ERR_INTERNAL = 16u };

// Base of every environment family: one device, one stream, engine-owned SoA state.
struct Env {
    mgym_config cfg{};
    int kind = 0;
    int obs_dim = 0;
    int state_cols = 0;
    uint64_t n = 0;      // environments
    uint64_t n_pad = 0;  // column stride (multiple of 1024 words: every column 4 KiB aligned)
    hipStream_t stream = nullptr;
    bool own_stream = false;
    uint32_t* d_err = nullptr;   // sticky device status word
    uint32_t* h_err = nullptr;   // pinned mirror
    unsigned long long* d_done = nullptr;  // kDoneShards partial counts of finished env-steps (done | truncated)
    unsigned long long* h_done = nullptr;  // pinned mirror
    hipEvent_t ev0 = nullptr, ev1 = nullptr;

    virtual ~Env() {}
    virtual int init() = 0;
    virtual int reset(const uint8_t* m0, const uint8_t* m1, bool all, float* obs_out) = 0;
    virtual int step(const void* actions, float* obs_out, float* reward, uint8_t* done, uint8_t* trunc) = 0;
    // step k of a K-step call: step() under the step's own action column, into slab k of each [K][..] output that is not null
    int step_k(int k, const void* actions_k, float* obs_out, float* reward, uint8_t* done, uint8_t* trunc) {
        return step(actions_k, obs_out ? obs_out + (size_t)k * obs_dim * n : nullptr, reward ? reward + (size_t)k * n : nullptr,
                    done ? done + (size_t)k * n : nullptr, trunc ? trunc + (size_t)k * n : nullptr);
    }
    // K fused steps; default: K launches of step() with strided per-step buffers
    virtual int rollout(const void* actions, int K, float* obs_out, float* reward, uint8_t* done, uint8_t* trunc) {
        float* const fin0 = final_obs;   // step k of the call writes its finished envs' observations to slab k (mgym_set_final_obs_out)
        int st = MGYM_OK;
        for (int k = 0; k < K && st == MGYM_OK; ++k) {
            if (fin0) final_obs = fin0 + (size_t)k * obs_dim * n;
            st = step_k(k, static_cast<const char*>(actions) + (size_t)k * n * 4, obs_out, reward, done, trunc);
        }
        final_obs = fin0;
        return st;
    }
    // mgym_set_final_obs_out: [final_cap][obs_dim][n] floats of the caller's, or null (the channel is off); only auto-reset handles of the classic families hold one
    float* final_obs = nullptr;
    int32_t final_cap = 0;
    // K fused steps under an on-device policy (mgym_rollout_uniform / _linear / _mlp): the action source, its weights or seed in `call`
    virtual int rollout_policy(const PolicyCall& call, int K, void* actions_out, float* obs_out, float* reward, uint8_t* done, uint8_t* trunc) = 0;
    // mgym_rollout_mlp2: the handle's weight pack in device memory (kMlp2PackMax floats, allocated at mgym_create).  mlp2_store lays the call's policy out
    // as mlp2_policy.h states and stores it on the stream ahead of the call's launches, by kernels that take the pack in slices as arguments: the caller's
    // array is read during the call only, a captured graph carries the weights, and consecutive calls on one stream each find their own.
    float* mlp2_dev = nullptr;
    int mlp2_store(const PolicyCall& call, int D, int A);
    // mgym_value_mlp: a second pack of the same size for a two-hidden-layer critic, so that an actor's and a critic's weights never share a buffer (a captured
    // graph that holds a mgym_rollout_mlp2 and a mgym_value_mlp replays each with its own); mlp2_store_to is the store of both
    float* value_dev = nullptr;
    // mgym_logprob_mlp: a third pack, for the same reason — the call re-evaluates an actor, usually the one a mgym_rollout_mlp2 on the same stream or in the same
    // graph drew with, but it may be another (the learner's current weights against the behaviour policy's), and neither call may find the other's words
    float* logp_dev = nullptr;
    // mgym_ppo_grad_mlp2 / mgym_value_grad_mlp2: a fourth and a fifth pack, the actor's and the critic's under their gradient calls, for the same reason
    float* ppo_grad_dev = nullptr;
    float* value_grad_dev = nullptr;
    int mlp2_store_to(float* dst, const float* weights, int D, int A, int H1, int H2);
    template <int D, int A>
    Mlp2Net<D, A> mlp2_net(const PolicyCall& call) const { return Mlp2Net<D, A>{mlp2_dev, call.hidden, call.hidden2, call.sigma}; }
    uint32_t uniform_calls = 0;  // mgym_rollout_uniform calls that launched so far (Philox counter word of the policy stream)
    // rollout_policy of the classic families (observation width D, A scores; `bound32`: fused_rollout_args_ok), whose fused kernels differ in name and config
    // only.  The family hands in what it owns.  TAKES: the sources it has kernels for; none is instantiated for another, and a call with one launches
    // nothing (the C ABI refuses it first).  `refusal`: the tail of the message where the family refuses the call itself, else null.  `linear`: its
    // linear-policy struct from call.weights.  `launch(S, arg, draw, net...)`: its one launch template with the source S, the policy argument (the linear
    // struct, value-initialised where the source reads none, or the hidden-layer pack), the draw (zeros where the source draws nothing), and for
    // a two-hidden-layer source its Mlp2Net, the head of the kernel's trailing pack (the weights are on the stream by then).
    template <int D, int A, bool (*TAKES)(int), class Linear, class Launch>
    int rollout_policy_classic(const PolicyCall& call, int K, void* actions_out, float* obs_out, float* reward, uint8_t* done, uint8_t* trunc, bool bound32,
                               const char* refusal, Linear&& linear, Launch&& launch) {
        if (n == 0 || K == 0) return MGYM_OK;
        if (refusal) { set_last_error(std::string(call.api) + refusal); return MGYM_ERR_BAD_ARG; }
        if (!fused_rollout_args_ok(call.api, n, K, bound32, actions_out, obs_out, reward, done, trunc)) return MGYM_ERR_BAD_ARG;
        if (roll_act_is_mlp2(call.source)) { if (const int st = mlp2_store(call, D, A)) return st; }
        with_policy_source([&](auto S) {
            constexpr int SRC = decltype(S)::value;
            if constexpr (!TAKES(SRC)) return;
            else if constexpr (roll_act_is_mlp2(SRC)) launch(S, decltype(linear(call.weights)){}, UniformDraw{call.seed, call.call}, mlp2_net<D, A>(call));
            else if constexpr (SRC == ROLL_ACT_UNIFORM) launch(S, decltype(linear(call.weights)){}, UniformDraw{call.seed, uniform_calls++});
            else if constexpr (SRC == ROLL_ACT_LINEAR) launch(S, linear(call.weights), UniformDraw{});
            else {   // the hidden-layer sources
                MlpPack<D, A> pack;
                mlp_pack<D, A>(call.weights, call.hidden, pack);
                if constexpr (roll_act_gauss(SRC)) launch(S, pack, GaussDraw{call.seed, call.call, call.sigma});
                else if constexpr (roll_act_samples(SRC)) launch(S, pack, UniformDraw{call.seed, call.call});
                else launch(S, pack, UniformDraw{});
            }
        }, call.source);
        MGYM_HIP(hipGetLastError());
        return MGYM_OK;
    }
    // one thread per environment: export, import, zero
    template <class Kernel, class... Args>
    int launch_per_env(Kernel kernel, Args... args) {
        if (n == 0) return MGYM_OK;
        hipLaunchKernelGGL(kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, args...);
        MGYM_HIP(hipGetLastError());
        return MGYM_OK;
    }
    // a classic family's reset kernel (Dev, m0, m1, all, masks_aligned, obs_out), one lane per group of 4 environments
    template <class Kernel, class Dev>
    int launch_reset(Kernel kernel, const Dev& dev, const uint8_t* m0, const uint8_t* m1, bool all, float* obs_out) {
        if (n == 0) return MGYM_OK;
        hipLaunchKernelGGL(kernel, dim3(grid_for((n + 3) / 4)), dim3(kBlock), 0, stream, dev, m0, m1, all ? 1 : 0, aligned(m0, 4) && aligned(m1, 4) ? 1 : 0, obs_out);
        MGYM_HIP(hipGetLastError());
        return MGYM_OK;
    }
    virtual int observation(const float** obs, uint64_t* col_stride) = 0;
    virtual int get_state(void* blob) = 0;
    virtual int set_state(const void* blob) = 0;
    // Testable::reset_deterministic of the reference's test modules (cartpole.rs:437-442, mountain_car.rs:403-408,
    // lunar_lander.rs:1249-1442)
    virtual int reset_deterministic(float* obs_out) = 0;
    // helper streams forked from `stream` must have rejoined it before a stream capture ends (mgym_graph_end)
    virtual int join_helpers() { return MGYM_OK; }
    // mgym_get_info: family-specific "key=value" lines appended to `out` (may launch probe kernels and synchronise)
    virtual int info(std::string&) { return MGYM_OK; }
    uint64_t config_epoch = 0;   // moves whenever something changes that captured launches have frozen into their arguments (abi.hip GraphBox)
    std::string hwq_env;   // GPU_MAX_HW_QUEUES as the environment held it at mgym_create ("unset" if absent)
    // mgym_get_elapsed_steps (out) / mgym_set_elapsed_steps (in): exactly one is non-null, a device array of n uint32; CartPole's counter is blob column 4
    virtual int elapsed(uint32_t*, const uint32_t*) { set_last_error("elapsed steps: MountainCar, Pendulum, Acrobot and LunarLander only (CartPole's counter is state blob column 4)"); return MGYM_ERR_BAD_ARG; }
    virtual int set_dispersion(const float*) { set_last_error("dispersion override: LunarLander only"); return MGYM_ERR_BAD_ARG; }
};

Env* make_cartpole();
Env* make_mountaincar(bool continuous);
Env* make_lunarlander();
Env* make_pendulum();
Env* make_acrobot();

}  // namespace mgym
