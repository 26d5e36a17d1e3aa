// mgym.hpp — C++ host-side mirror of the reference's environment interface, over the C ABI (mgym.h).
//
// The reference (ModuRL/ModuRL_Gym) is a Rust crate; its toolchain is absent from the build image, so
// the host side above the C ABI is C++ (the reference is compiled code).  Names, argument meaning and
// error behaviour follow the reference's `impl Gym for ...` blocks:
//     CartPoleV1::builder().sutton_barto_reward(b).is_euler(b).build()     cartpole.rs:34-44
//     MountainCarV0::builder().goal_velocity(v).build()                   mountain_car.rs:25-34
//     LunarLanderV3::builder().gravity(g).enable_wind(b).wind_power(p)
//                             .turbulence_power(p).seed(s).build()        lunar_lander.rs:278-291
//     reset() -> state;  step(action) -> StepInfo{state, reward, done, truncated}
// Where the reference panics (assert!), these throw: std::invalid_argument for an invalid action
// (cartpole.rs:252, mountain_car.rs:294) and bad gravity (lunar_lander.rs:292-296), std::logic_error
// for step-before-reset (lunar_lander.rs:920).  `VecGym` is the batched superset (device pointers).
// Header-only; link with libmgym.so.
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "mgym.h"

namespace mgym_host {

struct StepInfo {  // modurl::gym::StepInfo
    std::vector<float> state;
    float reward;
    bool done;
    bool truncated;
};

inline void check(int st) {
    if (st == MGYM_OK) return;
    std::string msg = mgym_last_error();
    switch (st) {
    case MGYM_ERR_INVALID_ACTION: throw std::invalid_argument("invalid action: " + msg);
    case MGYM_ERR_BAD_CONFIG: throw std::invalid_argument(msg);
    case MGYM_ERR_NOT_RESET: throw std::logic_error(msg);
    default: throw std::runtime_error("mgym status " + std::to_string(st) + ": " + msg);
    }
}

// n_envs environments of one family on one GPU; buffers are device pointers owned by the caller.  The episode time limit is
// cfg.max_episode_steps (0 = off, the reference's behaviour; CartPole keeps the reference's 500) — see mgym.h.
class VecGym {
  public:
    explicit VecGym(const mgym_config& cfg) : cfg_(cfg) {
        check(mgym_create(&cfg_, &env_));
        mgym_spec s;
        check(mgym_get_spec(cfg_.kind, &s));
        obs_dim_ = s.obs_dim;
    }
    ~VecGym() { mgym_destroy(env_); }
    VecGym(const VecGym&) = delete;
    VecGym& operator=(const VecGym&) = delete;

    void reset(const uint8_t* mask = nullptr, float* obs_out = nullptr) { check(mgym_reset(env_, mask, obs_out)); }
    void reset_done(const uint8_t* done, const uint8_t* trunc, float* obs_out = nullptr) { check(mgym_reset_done(env_, done, trunc, obs_out)); }
    void step(const void* actions, float* obs_out, float* reward, uint8_t* done, uint8_t* trunc) {
        check(mgym_step(env_, actions, obs_out, reward, done, trunc));
    }
    void sync() { check(mgym_sync(env_)); }
    // K fused steps under the on-device uniform random policy (CartPole); actions_out may be null
    void rollout_linear(const float* policy, int K, void* actions_out, float* obs, float* reward, uint8_t* done, uint8_t* trunc) {
        check(mgym_rollout_linear(env_, policy, K, actions_out, obs, reward, done, trunc));
    }
    // K fused steps under the on-device one-hidden-layer policy: policy = W1[H][D], b1[H], W2[A][H], b2[A] (host floats), activation MGYM_ACT_RELU / MGYM_ACT_TANH / MGYM_ACT_TANH_FAST (the cheap, word-defined tanh)
    // (LunarLander: K x (policy kernel, step) by default; inside its persistent rollout launch with MGYM_LL_ROLLOUT_MLP=1; the same words)
    void rollout_mlp(const float* policy, int hidden, int activation, int K, void* actions_out, float* obs, float* reward, uint8_t* done, uint8_t* trunc) {
        check(mgym_rollout_mlp(env_, policy, hidden, activation, K, actions_out, obs, reward, done, trunc));
    }
    // the same with the action drawn from the softmax of the scores (mgym_rollout_mlp_sample): a pure function of (policy_seed, policy_call, global env id,
    // step) and the scores; pass a new policy_call for each call that is to draw afresh.  Discrete families only; LunarLander always K x (policy kernel, step)
    void rollout_mlp_sample(const float* policy, int hidden, int activation, uint64_t policy_seed, uint32_t policy_call, int K, void* actions_out, float* obs, float* reward,
                            uint8_t* done, uint8_t* trunc) {
        check(mgym_rollout_mlp_sample(env_, policy, hidden, activation, policy_seed, policy_call, K, actions_out, obs, reward, done, trunc));
    }
    // MountainCarContinuous and Pendulum: the action drawn from a Gaussian around the score, a = mu + sigma * z (mgym_rollout_mlp_gauss): sigma finite and >= 0, z a
    // pure function of (policy_seed, policy_call, global env id, step); actions_out receives the f32 words before the step's clamp
    void rollout_mlp_gauss(const float* policy, int hidden, int activation, float sigma, uint64_t policy_seed, uint32_t policy_call, int K, void* actions_out, float* obs,
                           float* reward, uint8_t* done, uint8_t* trunc) {
        check(mgym_rollout_mlp_gauss(env_, policy, hidden, activation, sigma, policy_seed, policy_call, K, actions_out, obs, reward, done, trunc));
    }
    // two hidden layers, Linear(D, H1) - act - Linear(H1, H2) - act - Linear(H2, A) (mgym_rollout_mlp2): policy = W1[H1][D], b1[H1], W2[H2][H1], b2[H2], W3[A][H2],
    // b3[A] host floats; activation MGYM_ACT_RELU or MGYM_ACT_TANH_FAST; head MGYM_HEAD_GREEDY, MGYM_HEAD_SAMPLE (discrete families) or MGYM_HEAD_GAUSS
    // (MountainCarContinuous, Pendulum); sigma, policy_seed and policy_call are ignored by the heads that do not use them
    void rollout_mlp2(const float* policy, int hidden1, int hidden2, int activation, int head, float sigma, uint64_t policy_seed, uint32_t policy_call, int K,
                      void* actions_out, float* obs, float* reward, uint8_t* done, uint8_t* trunc) {
        check(mgym_rollout_mlp2(env_, policy, hidden1, hidden2, activation, head, sigma, policy_seed, policy_call, K, actions_out, obs, reward, done, trunc));
    }
    void rollout_uniform(uint64_t policy_seed, int K, void* actions_out, float* obs, float* reward, uint8_t* done, uint8_t* trunc) {
        check(mgym_rollout_uniform(env_, policy_seed, K, actions_out, obs, reward, done, trunc));
    }
    // env-steps that returned done or truncated since creation (synchronises)
    uint64_t episode_count() {
        uint64_t c = 0;
        check(mgym_episode_count(env_, &c));
        return c;
    }
    // the elapsed count of mgym_config::max_episode_steps (device arrays of n_envs uint32; on the handle's stream)
    void get_elapsed_steps(uint32_t* out) { check(mgym_get_elapsed_steps(env_, out)); }
    void set_elapsed_steps(const uint32_t* in) { check(mgym_set_elapsed_steps(env_, in)); }
    // The final observations of auto-reset episodes (mgym_set_final_obs_out): a device buffer [steps_cap][obs_dim][n_envs], written by every stepping call
    // where done | truncated is set, with the observation the step produced before the fused reset; nullptr turns the channel off.
    void set_final_obs_out(float* final_obs_out, int32_t steps_cap) { check(mgym_set_final_obs_out(env_, final_obs_out, steps_cap)); }
    // Generalised advantage estimation over a rollout's [K][n_envs] outputs in one launch (mgym_gae): device pointers; done / trunc / final_value may be
    // nullptr, and one of adv_out / ret_out; final_value is read only where trunc && !done
    void gae(int K, const float* reward, const uint8_t* done, const uint8_t* trunc, const float* value, const float* last_value, const float* final_value,
             float gamma, float lambda, float* adv_out, float* ret_out) {
        check(mgym_gae(env_, K, reward, done, trunc, value, last_value, final_value, gamma, lambda, adv_out, ret_out));
    }
    // A critic's values over a rollout's buffers, in the shapes gae() takes (mgym_value_mlp): critic is a HOST pointer in nn.Linear order, one hidden layer
    // (hidden2 == 0) or two; the rest are device pointers.  final_obs / final_value_out / trunc all set or the first two nullptr; done may be nullptr.
    // final_value_out is written only where trunc && !done, and final_obs is read only there
    void value_mlp(const float* critic, int hidden1, int hidden2, int activation, int K, const float* obs_first, const float* obs, const float* final_obs,
                   const uint8_t* done, const uint8_t* trunc, float* value_out, float* last_value_out, float* final_value_out) {
        check(mgym_value_mlp(env_, critic, hidden1, hidden2, activation, K, obs_first, obs, final_obs, done, trunc, value_out, last_value_out, final_value_out));
    }
    // The actor's log-probabilities of a rollout's actions (mgym_logprob_mlp): policy is a HOST pointer in nn.Linear order, one hidden layer (hidden2 == 0) or
    // two; head MGYM_HEAD_SAMPLE (discrete families) or MGYM_HEAD_GAUSS (continuous; sigma positive and normal); the rest are device pointers, actions the
    // rollout's actions_out words, logp_out [K][n_envs]
    void logprob_mlp(const float* policy, int hidden1, int hidden2, int activation, int head, float sigma, int K, const float* obs_first, const float* obs,
                     const void* actions, float* logp_out) {
        check(mgym_logprob_mlp(env_, policy, hidden1, hidden2, activation, head, sigma, K, obs_first, obs, actions, logp_out));
    }
    // PPO's loss and the actor's gradient, and a critic's squared-error loss and gradient, over a rollout's buffers (mgym_ppo_grad_mlp, mgym_value_grad_mlp):
    // one hidden layer; policy / critic are HOST pointers in nn.Linear order, the rest device pointers; the range is the environments env_first ..
    // env_first + env_count - 1 over all K steps; workspace: 16-byte aligned, at least min_bytes of grad_workspace_bytes; grad_out receives the parameters'
    // gradient in nn.Linear order and one more word (d / d log sigma, or +0), stats_out 8 floats
    static void grad_workspace_bytes(int kind, int hidden, size_t* min_bytes, size_t* best_bytes) {
        if (mgym_grad_workspace_bytes(kind, hidden, min_bytes, best_bytes) != MGYM_OK) throw std::runtime_error(mgym_last_error());
    }
    void ppo_grad_mlp(const float* policy, int hidden, int activation, int head, float sigma, int K, uint64_t env_first, uint64_t env_count, const float* obs_first,
                      const float* obs, const void* actions, const float* logp_old, const float* adv, float clip, float ent_coef, void* workspace,
                      size_t workspace_bytes, float* grad_out, float* stats_out) {
        check(mgym_ppo_grad_mlp(env_, policy, hidden, activation, head, sigma, K, env_first, env_count, obs_first, obs, actions, logp_old, adv, clip, ent_coef,
                                workspace, workspace_bytes, grad_out, stats_out));
    }
    void value_grad_mlp(const float* critic, int hidden, int activation, int K, uint64_t env_first, uint64_t env_count, const float* obs_first, const float* obs,
                        const float* ret, void* workspace, size_t workspace_bytes, float* grad_out, float* stats_out) {
        check(mgym_value_grad_mlp(env_, critic, hidden, activation, K, env_first, env_count, obs_first, obs, ret, workspace, workspace_bytes, grad_out, stats_out));
    }
    // The same for the two-hidden-layer net of rollout_mlp2 (mgym_grad_workspace_bytes2, mgym_ppo_grad_mlp2, mgym_value_grad_mlp2): policy / critic in the layout
    // of mgym_rollout_mlp2; grad_out receives dW1, db1, dW2, db2, dW3, db3 and one more word
    static void grad_workspace_bytes2(int kind, int hidden1, int hidden2, size_t* min_bytes, size_t* best_bytes) {
        if (mgym_grad_workspace_bytes2(kind, hidden1, hidden2, min_bytes, best_bytes) != MGYM_OK) throw std::runtime_error(mgym_last_error());
    }
    void ppo_grad_mlp2(const float* policy, int hidden1, int hidden2, int activation, int head, float sigma, int K, uint64_t env_first, uint64_t env_count,
                       const float* obs_first, const float* obs, const void* actions, const float* logp_old, const float* adv, float clip, float ent_coef,
                       void* workspace, size_t workspace_bytes, float* grad_out, float* stats_out) {
        check(mgym_ppo_grad_mlp2(env_, policy, hidden1, hidden2, activation, head, sigma, K, env_first, env_count, obs_first, obs, actions, logp_old, adv, clip,
                                 ent_coef, workspace, workspace_bytes, grad_out, stats_out));
    }
    void value_grad_mlp2(const float* critic, int hidden1, int hidden2, int activation, int K, uint64_t env_first, uint64_t env_count, const float* obs_first,
                         const float* obs, const float* ret, void* workspace, size_t workspace_bytes, float* grad_out, float* stats_out) {
        check(mgym_value_grad_mlp2(env_, critic, hidden1, hidden2, activation, K, env_first, env_count, obs_first, obs, ret, workspace, workspace_bytes, grad_out,
                                   stats_out));
    }
    // The return and length of the episodes that end inside a rollout (mgym_episode_returns): ep_return / ep_length [n_envs] are the caller's carry of the
    // running episodes (read and written); return_out / length_out [K][n_envs] (or nullptr) are written only where done | trunc
    void episode_returns(int K, const float* reward, const uint8_t* done, const uint8_t* trunc, float* ep_return, uint32_t* ep_length, float* return_out,
                         uint32_t* length_out) {
        check(mgym_episode_returns(env_, K, reward, done, trunc, ep_return, ep_length, return_out, length_out));
    }
    uint32_t max_episode_steps() const { return cfg_.max_episode_steps; }
    const float* observation(uint64_t* col_stride) {
        const float* p = nullptr;
        check(mgym_observation(env_, &p, col_stride));
        return p;
    }
    mgym_env* handle() { return env_; }
    int obs_dim() const { return obs_dim_; }
    uint64_t n_envs() const { return cfg_.n_envs; }
    int device() const { return cfg_.device; }

  private:
    mgym_config cfg_;
    mgym_env* env_ = nullptr;
    int obs_dim_ = 0;
};

// single environment with the reference's scalar signature (n_envs = 1)
class SingleGym {
  public:
    // owns five device allocations and a handle: not copyable (a copy would free them twice), movable
    SingleGym(const SingleGym&) = delete;
    SingleGym& operator=(const SingleGym&) = delete;
    SingleGym(SingleGym&& o) noexcept
        : vec_(o.vec_), d_act_(o.d_act_), d_obs_(o.d_obs_), d_rew_(o.d_rew_), d_done_(o.d_done_), d_trunc_(o.d_trunc_) {
        o.vec_ = nullptr; o.d_act_ = nullptr; o.d_obs_ = nullptr; o.d_rew_ = nullptr; o.d_done_ = nullptr; o.d_trunc_ = nullptr;
    }
    SingleGym& operator=(SingleGym&&) = delete;
    std::vector<float> reset() {
        vec_->reset(nullptr, d_obs_);
        vec_->sync();
        return fetch_obs();
    }
    StepInfo step(uint32_t action) { return step_bits(action); }

  protected:
    explicit SingleGym(const mgym_config& cfg) {
        vec_ = new VecGym(cfg);
        const int dev = cfg.device;
        void* p = nullptr;
        check(mgym_malloc(dev, 64, &p)); d_act_ = p;
        check(mgym_malloc(dev, sizeof(float) * 8, &p)); d_obs_ = static_cast<float*>(p);
        check(mgym_malloc(dev, sizeof(float) * 4, &p)); d_rew_ = static_cast<float*>(p);
        check(mgym_malloc(dev, 16, &p)); d_done_ = static_cast<uint8_t*>(p);
        check(mgym_malloc(dev, 16, &p)); d_trunc_ = static_cast<uint8_t*>(p);
    }
    ~SingleGym() {
        if (!vec_) return;  // moved from
        const int dev = vec_->device();
        mgym_free(dev, d_act_); mgym_free(dev, d_obs_); mgym_free(dev, d_rew_); mgym_free(dev, d_done_); mgym_free(dev, d_trunc_);
        delete vec_;
    }
    StepInfo step_bits(uint32_t bits) {
        const int dev = vec_->device();
        check(mgym_memcpy_h2d(dev, d_act_, &bits, 4));
        vec_->step(d_act_, d_obs_, d_rew_, d_done_, d_trunc_);
        vec_->sync();
        StepInfo si;
        si.state = fetch_obs();
        uint8_t d = 0, t = 0;
        check(mgym_memcpy_d2h(dev, &si.reward, d_rew_, 4));
        check(mgym_memcpy_d2h(dev, &d, d_done_, 1));
        check(mgym_memcpy_d2h(dev, &t, d_trunc_, 1));
        si.done = d != 0; si.truncated = t != 0;
        return si;
    }
    std::vector<float> fetch_obs() {
        std::vector<float> o(vec_->obs_dim());
        check(mgym_memcpy_d2h(vec_->device(), o.data(), d_obs_, sizeof(float) * o.size()));
        return o;
    }
    static mgym_config defaults(int kind, int device, uint64_t seed) {
        mgym_config c;
        check(mgym_default_config(kind, &c));
        c.device = device; c.seed = seed; c.n_envs = 1;
        return c;
    }
    VecGym* vec_ = nullptr;
    void* d_act_ = nullptr;
    float *d_obs_ = nullptr, *d_rew_ = nullptr;
    uint8_t *d_done_ = nullptr, *d_trunc_ = nullptr;
};

class CartPoleV1 : public SingleGym {  // cartpole.rs:13-357
  public:
    struct Builder {
        int device_ = 0; bool sutton_barto_reward_ = false; bool is_euler_ = true; uint64_t seed_ = 0;
        Builder& device(int d) { device_ = d; return *this; }
        Builder& sutton_barto_reward(bool b) { sutton_barto_reward_ = b; return *this; }
        Builder& is_euler(bool b) { is_euler_ = b; return *this; }
        Builder& seed(uint64_t s) { seed_ = s; return *this; }
        CartPoleV1* build() { return new CartPoleV1(*this); }
    };
    static Builder builder() { return Builder(); }

  private:
    static mgym_config cfg(const Builder& b) {
        mgym_config c = defaults(MGYM_CARTPOLE, b.device_, b.seed_);
        c.sutton_barto_reward = b.sutton_barto_reward_; c.is_euler = b.is_euler_;
        return c;
    }
    explicit CartPoleV1(const Builder& b) : SingleGym(cfg(b)) {}
};

class MountainCarV0 : public SingleGym {  // mountain_car.rs:10-339
  public:
    struct Builder {
        int device_ = 0; float goal_velocity_ = 0.0f; uint64_t seed_ = 0; uint32_t max_episode_steps_ = 0;
        Builder& device(int d) { device_ = d; return *this; }
        Builder& goal_velocity(float v) { goal_velocity_ = v; return *this; }
        Builder& max_episode_steps(uint32_t k) { max_episode_steps_ = k; return *this; }  // superset: not in the reference (0 = never truncates)
        Builder& seed(uint64_t s) { seed_ = s; return *this; }
        MountainCarV0* build() { return new MountainCarV0(*this); }
    };
    static Builder builder() { return Builder(); }

  private:
    static mgym_config cfg(const Builder& b) {
        mgym_config c = defaults(MGYM_MOUNTAINCAR, b.device_, b.seed_);
        c.goal_velocity = b.goal_velocity_;
        c.max_episode_steps = b.max_episode_steps_;
        return c;
    }
    explicit MountainCarV0(const Builder& b) : SingleGym(cfg(b)) {}
};

class LunarLanderV3 : public SingleGym {  // lunar_lander.rs:232-1201
  public:
    struct Builder {
        int device_ = 0; float gravity_ = -10.0f; bool enable_wind_ = false; float wind_power_ = 15.0f, turbulence_power_ = 1.5f;
        uint64_t seed_ = 0; uint32_t max_episode_steps_ = 0;
        Builder& device(int d) { device_ = d; return *this; }
        Builder& max_episode_steps(uint32_t k) { max_episode_steps_ = k; return *this; }  // superset: not in the reference (0 = never truncates)
        Builder& gravity(float g) { gravity_ = g; return *this; }
        Builder& enable_wind(bool b) { enable_wind_ = b; return *this; }
        Builder& wind_power(float p) { wind_power_ = p; return *this; }
        Builder& turbulence_power(float p) { turbulence_power_ = p; return *this; }
        Builder& seed(uint64_t s) { seed_ = s; return *this; }
        LunarLanderV3* build() { return new LunarLanderV3(*this); }
    };
    static Builder builder() { return Builder(); }

  private:
    static mgym_config cfg(const Builder& b) {
        mgym_config c = defaults(MGYM_LUNARLANDER, b.device_, b.seed_);
        c.gravity = b.gravity_; c.enable_wind = b.enable_wind_; c.wind_power = b.wind_power_; c.turbulence_power = b.turbulence_power_;
        c.max_episode_steps = b.max_episode_steps_;
        return c;
    }
    explicit LunarLanderV3(const Builder& b) : SingleGym(cfg(b)) {}
};

}  // namespace mgym_host
