// abi.hip — the extern "C" entry points declared in include/mgym.h.
// Thin: argument checks, device selection, dispatch to the per-family Env object.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>

#include "common.h"
#include "gae.h"
#include "grad.h"
#include "grad2.h"
#include "logprob.h"
#include "time_limit.h"
#include "value.h"

namespace mgym {

static thread_local std::string g_last_error;

void set_last_error(const std::string& msg) { g_last_error = msg; }

int hip_fail(hipError_t e, const char* what, const char* file, int line) {
    char buf[512];
    snprintf(buf, sizeof buf, "HIP error %d (%s) in `%s` at %s:%d", (int)e, hipGetErrorString(e), what, file, line);
    g_last_error = buf;
    return (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorInsufficientDriver) ? MGYM_ERR_NO_DEVICE
                                                                                                      : MGYM_ERR_HIP;
}

static int bad_arg(const char* msg) {
    g_last_error = msg;
    return MGYM_ERR_BAD_ARG;
}

struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

}  // namespace mgym

using namespace mgym;

// SoA [obs_dim][stride] -> AoS [n][obs_dim]; one lane per env, obs_dim (<= 8) consecutive words per lane
__global__ void obs_to_aos_kernel(const float* __restrict__ soa, uint64_t stride, int obs_dim, uint64_t n, float* __restrict__ aos) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int k = 0; k < obs_dim; ++k) aos[i * obs_dim + k] = soa[(uint64_t)k * stride + i];
}

// mgym_rollout_mlp2: a slice of the weight pack, by value (a kernel argument holds 4 KiB), stored to the handle's buffer
constexpr int kMlp2Slice = 1000;
struct Mlp2Slice { float w[kMlp2Slice]; };
static_assert(sizeof(Mlp2Slice) + 16 <= 4096, "mlp2_pack_kernel: by-value kernel arguments above 4096 bytes");
__global__ void __launch_bounds__(256) mlp2_pack_kernel(Mlp2Slice slice, float* __restrict__ dst, int count) {
    for (int i = threadIdx.x; i < count; i += blockDim.x) dst[i] = slice.w[i];
}

int mgym::Env::mlp2_store(const PolicyCall& call, int D, int A) { return mlp2_store_to(mlp2_dev, call.weights, D, A, call.hidden, call.hidden2); }

int mgym::Env::mlp2_store_to(float* dst, const float* weights, int D, int A, int H1, int H2) {
    static_assert(kMlp2PackMax == 5192, "the pack of mlp2_policy.h at its largest");
    float pack[kMlp2PackMax];
    mlp2_pack(weights, D, A, H1, H2, pack);
    const int total = mlp2_pack_floats(D, H1, H2);
    for (int at = 0; at < total; at += kMlp2Slice) {
        Mlp2Slice slice{};   // (value-initialised: the words past `count` travel in the launch and in a captured graph node too)
        const int count = total - at < kMlp2Slice ? total - at : kMlp2Slice;
        memcpy(slice.w, pack + at, (size_t)count * sizeof(float));
        hipLaunchKernelGGL(mlp2_pack_kernel, dim3(1), dim3(256), 0, stream, slice, dst + at, count);
        MGYM_HIP(hipGetLastError());
    }
    return MGYM_OK;
}

struct mgym_env {
    Env* impl;
};

constexpr int kKindUnassigned = 5;   // between MGYM_PENDULUM and MGYM_ACROBOT: no family, refused like any unknown kind

extern "C" {

int mgym_abi_version(void) { return MGYM_ABI_VERSION; }

int mgym_default_config(int kind, mgym_config* cfg) {
    if (!cfg) return bad_arg("mgym_default_config: cfg is NULL");
    if (kind < MGYM_CARTPOLE || kind > MGYM_ACROBOT || kind == kKindUnassigned) return bad_arg("mgym_default_config: unknown kind");
    memset(cfg, 0, sizeof *cfg);
    cfg->struct_size = (uint32_t)sizeof *cfg;
    cfg->kind = kind;
    cfg->n_envs = 1;
    cfg->sutton_barto_reward = 0;  // cartpole.rs:39
    cfg->is_euler = 1;             // cartpole.rs:40
    cfg->goal_velocity = 0.0f;     // mountain_car.rs:33
    cfg->gravity = kind == MGYM_PENDULUM ? 10.0f : -10.0f;  // lunar_lander.rs:282; Pendulum-v1: g = 10 (gymnasium)
    cfg->enable_wind = 0;          // :283
    cfg->wind_power = 15.0f;       // :284
    cfg->turbulence_power = 1.5f;  // :285
    return MGYM_OK;
}

int mgym_get_spec(int kind, mgym_spec* s) {
    if (!s) return bad_arg("mgym_get_spec: spec is NULL");
    memset(s, 0, sizeof *s);
    const float inf = __builtin_inff();
    switch (kind) {
    case MGYM_CARTPOLE: {  // cartpole.rs:58-69
        s->obs_dim = 4; s->n_actions = 2; s->state_cols = 7;
        const float thr = 12.0f * 2.0f * 3.14159265358979323846f / 360.0f;
        const float hi[4] = {2.4f * 2.0f, inf, thr * 2.0f, inf};
        for (int k = 0; k < 4; ++k) { s->obs_high[k] = hi[k]; s->obs_low[k] = -hi[k]; }
        break;
    }
    case MGYM_MOUNTAINCAR:
    case MGYM_MOUNTAINCAR_CONT:  // mountain_car.rs:42-48
        s->obs_dim = 2; s->state_cols = 3;
        s->obs_low[0] = -1.2f; s->obs_low[1] = -0.07f; s->obs_high[0] = 0.6f; s->obs_high[1] = 0.07f;
        if (kind == MGYM_MOUNTAINCAR) { s->n_actions = 3; }
        else { s->n_actions = 0; s->action_is_float = 1; s->action_low = -1.0f; s->action_high = 1.0f; }
        break;
    case MGYM_LUNARLANDER: {  // lunar_lander.rs:1169-1200
        s->obs_dim = 8; s->n_actions = 4; s->state_cols = 27;
        const float twopi = 2.0f * 3.14159265358979323846f;
        const float hi[8] = {2.5f, 2.5f, 10.0f, 10.0f, twopi, 10.0f, 1.0f, 1.0f};
        for (int k = 0; k < 8; ++k) { s->obs_high[k] = hi[k]; s->obs_low[k] = k < 6 ? -hi[k] : 0.0f; }
        break;
    }
    case MGYM_PENDULUM: {  // gymnasium Pendulum-v1 (not in the reference): (cos th, sin th, thdot), Box(-2, 2) torque
        s->obs_dim = 3; s->state_cols = 3; s->n_actions = 0; s->action_is_float = 1; s->action_low = -2.0f; s->action_high = 2.0f;
        const float hi[3] = {1.0f, 1.0f, 8.0f};
        for (int k = 0; k < 3; ++k) { s->obs_high[k] = hi[k]; s->obs_low[k] = -hi[k]; }
        break;
    }
    case MGYM_ACROBOT: {  // gymnasium Acrobot-v1 (not in the reference): (cos th1, sin th1, cos th2, sin th2, w1, w2), Discrete(3) torque
        s->obs_dim = 6; s->n_actions = 3; s->state_cols = 5;
        const float hi[6] = {1.0f, 1.0f, 1.0f, 1.0f, (float)(4.0 * 3.14159265358979323846), (float)(9.0 * 3.14159265358979323846)};
        for (int k = 0; k < 6; ++k) { s->obs_high[k] = hi[k]; s->obs_low[k] = -hi[k]; }
        break;
    }
    default:
        return bad_arg("mgym_get_spec: unknown kind");
    }
    return MGYM_OK;
}

int mgym_device_count(int* count) {
    if (!count) return bad_arg("mgym_device_count: NULL");
    MGYM_HIP(hipGetDeviceCount(count));
    return MGYM_OK;
}

int mgym_create(const mgym_config* cfg, mgym_env** out) {
    if (!cfg || !out) return bad_arg("mgym_create: NULL argument");
    *out = nullptr;
    if (cfg->struct_size != sizeof(mgym_config)) return bad_arg("mgym_create: struct_size mismatch (ABI version?)");
    if (cfg->kind == MGYM_LUNARLANDER && !(-12.0f < cfg->gravity && cfg->gravity < 0.0f)) {
        // lunar_lander.rs:292-296
        char buf[128];
        snprintf(buf, sizeof buf, "gravity (current value: %g) must be between -12 and 0", (double)cfg->gravity);
        set_last_error(buf);
        return MGYM_ERR_BAD_CONFIG;
    }
    if (cfg->kind == MGYM_PENDULUM && !__builtin_isfinite(cfg->gravity)) {
        char buf[128];
        snprintf(buf, sizeof buf, "gravity (current value: %g) must be finite for Pendulum", (double)cfg->gravity);
        set_last_error(buf);
        return MGYM_ERR_BAD_CONFIG;
    }
    // episode time limit (not in the reference): CartPole keeps the reference's 500 (cartpole.rs:297), the others count in 16 bits
    if (cfg->kind == MGYM_CARTPOLE ? (cfg->max_episode_steps != 0u && cfg->max_episode_steps != 500u) : cfg->max_episode_steps > kMaxEpisodeSteps) {
        char buf[160];
        if (cfg->kind == MGYM_CARTPOLE) snprintf(buf, sizeof buf, "max_episode_steps (current value: %u): CartPole keeps the reference's 500 — 0 or 500 only", cfg->max_episode_steps);
        else snprintf(buf, sizeof buf, "max_episode_steps (current value: %u) must be between 0 (off) and 65535", cfg->max_episode_steps);
        set_last_error(buf);
        return MGYM_ERR_BAD_CONFIG;
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        set_last_error("no HIP device visible: libmgym has no CPU fallback (build/run on an MI355X)");
        return MGYM_ERR_NO_DEVICE;
    }
    if (cfg->device < 0 || cfg->device >= ndev) return bad_arg("mgym_create: device ordinal out of range");
    DeviceGuard guard(cfg->device);
    if (!guard.ok) return hip_fail(hipErrorInvalidDevice, "hipSetDevice", __FILE__, __LINE__);

    Env* impl = nullptr;
    switch (cfg->kind) {
    case MGYM_CARTPOLE: impl = make_cartpole(); break;
    case MGYM_MOUNTAINCAR: impl = make_mountaincar(false); break;
    case MGYM_MOUNTAINCAR_CONT: impl = make_mountaincar(true); break;
    case MGYM_LUNARLANDER: impl = make_lunarlander(); break;
    case MGYM_PENDULUM: impl = make_pendulum(); break;
    case MGYM_ACROBOT: impl = make_acrobot(); break;
    default: return bad_arg("mgym_create: unknown kind");
    }
    if (!impl) { set_last_error("mgym_create: environment family not available in this build"); return MGYM_ERR_BAD_CONFIG; }
    impl->cfg = *cfg;
    { const char* q = getenv("GPU_MAX_HW_QUEUES"); impl->hwq_env = q ? q : "unset"; }
    impl->kind = cfg->kind;
    impl->n = cfg->n_envs;
    impl->n_pad = round_up(cfg->n_envs ? cfg->n_envs : 1, 1024);
    int st = MGYM_OK;
    do {
        if (hipStreamCreateWithFlags(&impl->stream, hipStreamNonBlocking) != hipSuccess) { st = MGYM_ERR_HIP; set_last_error("hipStreamCreate failed"); break; }
        impl->own_stream = true;
        if (hipMalloc((void**)&impl->d_err, sizeof(uint32_t)) != hipSuccess) { st = MGYM_ERR_HIP; set_last_error("hipMalloc failed"); break; }
        if (hipHostMalloc((void**)&impl->h_err, sizeof(uint32_t), 0) != hipSuccess) { st = MGYM_ERR_HIP; set_last_error("hipHostMalloc failed"); break; }
        if (hipMemsetAsync(impl->d_err, 0, sizeof(uint32_t), impl->stream) != hipSuccess) { st = MGYM_ERR_HIP; break; }
        if (hipMalloc((void**)&impl->d_done, kDoneShards * sizeof(unsigned long long)) != hipSuccess) { st = MGYM_ERR_HIP; set_last_error("hipMalloc failed"); break; }
        if (hipHostMalloc((void**)&impl->h_done, kDoneShards * sizeof(unsigned long long), 0) != hipSuccess) { st = MGYM_ERR_HIP; set_last_error("hipHostMalloc failed"); break; }
        if (hipMemsetAsync(impl->d_done, 0, kDoneShards * sizeof(unsigned long long), impl->stream) != hipSuccess) { st = MGYM_ERR_HIP; break; }
        if (hipMalloc((void**)&impl->mlp2_dev, kMlp2PackMax * sizeof(float)) != hipSuccess) { st = MGYM_ERR_HIP; set_last_error("hipMalloc failed"); break; }
        if (hipMalloc((void**)&impl->value_dev, kMlp2PackMax * sizeof(float)) != hipSuccess) { st = MGYM_ERR_HIP; set_last_error("hipMalloc failed"); break; }
        if (hipMalloc((void**)&impl->logp_dev, kMlp2PackMax * sizeof(float)) != hipSuccess) { st = MGYM_ERR_HIP; set_last_error("hipMalloc failed"); break; }
        if (hipMalloc((void**)&impl->ppo_grad_dev, kMlp2PackMax * sizeof(float)) != hipSuccess) { st = MGYM_ERR_HIP; set_last_error("hipMalloc failed"); break; }
        if (hipMalloc((void**)&impl->value_grad_dev, kMlp2PackMax * sizeof(float)) != hipSuccess) { st = MGYM_ERR_HIP; set_last_error("hipMalloc failed"); break; }
        if (hipEventCreate(&impl->ev0) != hipSuccess || hipEventCreate(&impl->ev1) != hipSuccess) { st = MGYM_ERR_HIP; break; }
        st = impl->init();
        if (st != MGYM_OK) break;
        if (hipStreamSynchronize(impl->stream) != hipSuccess) { st = MGYM_ERR_HIP; set_last_error("init sync failed"); break; }
    } while (0);
    if (st != MGYM_OK) {
        mgym_env tmp{impl};
        mgym_env* p = new mgym_env(tmp);
        mgym_destroy(p);
        return st;
    }
    *out = new mgym_env{impl};
    return MGYM_OK;
}

int mgym_destroy(mgym_env* env) {
    if (!env) return MGYM_OK;
    Env* e = env->impl;
    if (e) {
        DeviceGuard guard(e->cfg.device);
        if (e->stream) (void)hipStreamSynchronize(e->stream);
        if (e->ev0) (void)hipEventDestroy(e->ev0);
        if (e->ev1) (void)hipEventDestroy(e->ev1);
        if (e->d_err) (void)hipFree(e->d_err);
        if (e->h_err) (void)hipHostFree(e->h_err);
        if (e->d_done) (void)hipFree(e->d_done);
        if (e->h_done) (void)hipHostFree(e->h_done);
        if (e->mlp2_dev) (void)hipFree(e->mlp2_dev);
        if (e->value_dev) (void)hipFree(e->value_dev);
        if (e->logp_dev) (void)hipFree(e->logp_dev);
        if (e->ppo_grad_dev) (void)hipFree(e->ppo_grad_dev);
        if (e->value_grad_dev) (void)hipFree(e->value_grad_dev);
        hipStream_t s = e->own_stream ? e->stream : nullptr;
        delete e;
        if (s) (void)hipStreamDestroy(s);
    }
    delete env;
    return MGYM_OK;
}

// mgym_set_final_obs_out: a call that steps K times needs K slabs — refused before any launch, the state untouched
#define FINAL_CAP_OR_FAIL(api, K)                                                                                                     \
    if (e->final_obs && (K) > e->final_cap)                                                                                            \
        return bad_arg((std::string(api) + ": K = " + std::to_string(K) + " exceeds steps_cap = " + std::to_string(e->final_cap) +    \
                        " of mgym_set_final_obs_out").c_str());

#define ENV_OR_FAIL(env)                                        \
    if (!(env) || !(env)->impl) return bad_arg("NULL env handle"); \
    Env* e = (env)->impl;                                       \
    DeviceGuard guard(e->cfg.device);

int mgym_set_stream(mgym_env* env, void* hip_stream) {
    ENV_OR_FAIL(env);
    if (e->own_stream && e->stream) {
        (void)hipStreamSynchronize(e->stream);
        (void)hipStreamDestroy(e->stream);
    }
    e->stream = static_cast<hipStream_t>(hip_stream);
    e->own_stream = false;
    return MGYM_OK;
}

void* mgym_get_stream(mgym_env* env) { return (env && env->impl) ? (void*)env->impl->stream : nullptr; }

int mgym_reset(mgym_env* env, const uint8_t* mask, float* obs_out) {
    ENV_OR_FAIL(env);
    return e->reset(mask, nullptr, mask == nullptr, obs_out);
}

int mgym_reset_done(mgym_env* env, const uint8_t* done, const uint8_t* truncated, float* obs_out) {
    ENV_OR_FAIL(env);
    if (!done && !truncated) return bad_arg("mgym_reset_done: both masks NULL (use mgym_reset(env, NULL, ..) to reset all)");
    return e->reset(done, truncated, false, obs_out);
}

int mgym_reset_deterministic(mgym_env* env, float* obs_out) {
    ENV_OR_FAIL(env);
    return e->reset_deterministic(obs_out);
}

int mgym_step(mgym_env* env, const void* actions, float* obs_out, float* reward_out, uint8_t* done_out,
              uint8_t* trunc_out) {
    ENV_OR_FAIL(env);
    if (!actions && e->n) return bad_arg("mgym_step: actions is NULL");
    return e->step(actions, obs_out, reward_out, done_out, trunc_out);
}

int mgym_rollout(mgym_env* env, const void* actions, int32_t K, float* obs_out, float* reward_out, uint8_t* done_out,
                 uint8_t* trunc_out) {
    ENV_OR_FAIL(env);
    if (K < 0) return bad_arg("mgym_rollout: K < 0");
    FINAL_CAP_OR_FAIL("mgym_rollout", K);
    if (!actions && e->n && K) return bad_arg("mgym_rollout: actions is NULL");
    if (e->cfg.kind == MGYM_LUNARLANDER) {
        // While the stream is being captured a LunarLander rollout records K steps, not its persistent launch: replays of a captured persistent
        // launch ended in an abort inside the HIP runtime (35 of 40 fresh processes; eager launches of the same kernel and captured steps do not),
        // unexplained at the end of round 4 — the per-environment results are the same words either way.
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(e->stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
            return e->Env::rollout(actions, K, obs_out, reward_out, done_out, trunc_out);
    }
    return e->rollout(actions, K, obs_out, reward_out, done_out, trunc_out);
}

// The families by kind: the name a refusal uses and the key mgym_get_info prints (kKindUnassigned has neither).
static const struct { const char* name; const char* key; } kFamilies[] = {{"CartPole", "cartpole"}, {"MountainCar", "mountain_car"}, {"MountainCarContinuous", "mountain_car_continuous"},
                                                                          {"LunarLander", "lunar_lander"}, {"Pendulum", "pendulum"}, {"", ""}, {"Acrobot", "acrobot"}};
static bool box_actions(const Env* e) { return e->cfg.kind == MGYM_MOUNTAINCAR_CONT || e->cfg.kind == MGYM_PENDULUM; }

// The argument checks of the six policy entry points, written once.  An entry point states what it takes beyond K and the outputs (TAKES_*; DRAWS: its actions come
// from the policy stream, keyed per 4 consecutive global env ids — the uniform policy, the one that draws without weights, words that its own way) and, where it does
// not offer the handle's family, its refusal; the order below is the one order they all report in — a refusal comes first, or behind the head it depends on.
enum { TAKES_POLICY = 1, TAKES_HIDDEN = 2, TAKES_HIDDEN2 = 4, TAKES_HEAD = 8, TAKES_SIGMA = 16, DRAWS = 32 };
struct PolicyArgs { int32_t K; const float* policy = nullptr; int32_t hidden = 0, hidden2 = 0, activation = 0, head = 0; float sigma = 0.0f; };
static_assert(MGYM_ACT_RELU == MLP_ACT_RELU && MGYM_ACT_TANH == MLP_ACT_TANH && MGYM_ACT_TANH_FAST == MLP_ACT_TANH_FAST, "mgym.h and mlp_policy.h number the activations alike");
static_assert(MGYM_HEAD_GREEDY == MLP_HEAD_GREEDY && MGYM_HEAD_SAMPLE == MLP_HEAD_SAMPLE && MGYM_HEAD_GAUSS == MLP_HEAD_GAUSS, "mgym.h and mlp_policy.h number the heads alike");

// ---- checks the policy entry points and the learner calls (mgym_value_mlp, mgym_logprob_mlp, the gradient calls) share ----
// a call's refusal: "<api>: <what>" as the last error, MGYM_ERR_BAD_ARG
struct Bad {
    const char* api;
    int operator()(const std::string& what) const { return bad_arg((std::string(api) + ": " + what).c_str()); }
};

// The widths, then the activation.  NET_HIDDEN: one layer, worded "hidden".  NET_ROLLOUT2: two layers, hidden2 from 1.  NET_LEARNER: "hidden1" and "hidden2",
// hidden2 == 0 meaning one layer.  NET_GRAD2: the two-layer gradient calls, hidden2 from 1, the refusal naming the one-layer calls.  Two layers offer no
// exact tanh; the rollout and the learner calls word that refusal differently.
enum NetNames { NET_HIDDEN, NET_ROLLOUT2, NET_LEARNER, NET_GRAD2 };
static int net_shape_ok(const Bad& bad, int32_t h1, int32_t h2, int32_t activation, NetNames names) {
    if (h1 < 1 || h1 > 64) return bad(names == NET_HIDDEN ? "hidden must be between 1 and 64" : "hidden1 must be between 1 and 64");
    if (names == NET_ROLLOUT2 && (h2 < 1 || h2 > 64)) return bad("hidden2 must be between 1 and 64");
    if (names == NET_LEARNER && (h2 < 0 || h2 > 64)) return bad("hidden2 must be between 0 (one hidden layer) and 64");
    if (names == NET_GRAD2 && (h2 < 1 || h2 > 64)) return bad("hidden2 must be between 1 and 64 (one hidden layer: mgym_ppo_grad_mlp / mgym_value_grad_mlp)");
    const bool two = names != NET_HIDDEN && h2 >= 1;
    if (two && activation == MGYM_ACT_TANH)
        return bad(std::string("activation MGYM_ACT_TANH is not offered with two hidden layers (") +
                   (names == NET_ROLLOUT2 ? "the exact tanh would be nearly all of the launch" : "as in mgym_rollout_mlp2") + "): use MGYM_ACT_TANH_FAST or MGYM_ACT_RELU");
    if (activation != MGYM_ACT_RELU && activation != MGYM_ACT_TANH && activation != MGYM_ACT_TANH_FAST)   // (2 is not one)
        return bad(two ? "activation must be MGYM_ACT_RELU or MGYM_ACT_TANH_FAST" : "activation must be MGYM_ACT_RELU, MGYM_ACT_TANH or MGYM_ACT_TANH_FAST");
    return MGYM_OK;
}

// the head of a call that needs a density: a drawing head, the one the family's actions have, and for the Gaussian a sigma with a density
static int density_head_ok(const Bad& bad, const Env* e, int32_t head, float sigma) {
    if (head == MGYM_HEAD_GREEDY) return bad("head MGYM_HEAD_GREEDY: a deterministic policy has no density (use MGYM_HEAD_SAMPLE or MGYM_HEAD_GAUSS)");
    if (head != MGYM_HEAD_SAMPLE && head != MGYM_HEAD_GAUSS) return bad("head must be MGYM_HEAD_SAMPLE or MGYM_HEAD_GAUSS");
    if (head == MGYM_HEAD_SAMPLE && box_actions(e)) return bad(std::string("head MGYM_HEAD_SAMPLE: ") + kFamilies[e->cfg.kind].name + " has no discrete actions (use MGYM_HEAD_GAUSS)");
    if (head == MGYM_HEAD_GAUSS && !box_actions(e)) return bad(std::string("head MGYM_HEAD_GAUSS: ") + kFamilies[e->cfg.kind].name + " has discrete actions (use MGYM_HEAD_SAMPLE)");
    if (head == MGYM_HEAD_GAUSS && !logp_sigma_ok(sigma)) return bad("sigma must be a finite, normal, positive float (sigma == 0 has no density)");   // (a NaN fails the first test)
    return MGYM_OK;
}

// A call's device pointers.  Alignments first, in table order (alignment 0: not checked here; a null optional pointer is skipped); then every output against
// every input in table order and against the outputs before it — or, `any_output`, against every other output (mgym_value_mlp's wording).
struct Pointer { const char* name; const void* p; bool out; size_t alignment; };
static int pointers_ok(const Bad& bad, std::initializer_list<Pointer> table, bool any_output = false) {
    for (const Pointer& f : table)
        if (f.p && f.alignment && !aligned(f.p, f.alignment)) return bad(std::string(f.name) + " must be " + std::to_string(f.alignment) + "-byte aligned");
    for (const Pointer& f : table) {
        if (!f.out || !f.p) continue;
        for (const Pointer& g : table)
            if (!g.out && g.p == f.p) return bad(std::string(f.name) + " is the same pointer as " + g.name);
        for (const Pointer& g : table) {
            if (&g == &f && !any_output) break;
            if (g.out && &g != &f && g.p == f.p) return bad(std::string(f.name) + " is the same pointer as " + g.name);
        }
    }
    return MGYM_OK;
}

// a family's observation width and scores
static int family_dims(int kind, int* D, int* A) {
    mgym_spec spec;
    if (const int st = mgym_get_spec(kind, &spec)) return st;
    *D = spec.obs_dim;
    *A = spec.n_actions ? spec.n_actions : 1;   // a continuous family has one score, the mean
    return MGYM_OK;
}

static int policy_args_ok(const Env* e, const char* api, int takes, const std::string& refusal, const PolicyArgs& a) {
    const Bad bad{api};
    if (a.K < 0) return bad("K < 0");
    FINAL_CAP_OR_FAIL(api, a.K);
    if (!refusal.empty() && !(takes & TAKES_HEAD)) return bad(refusal);
    if ((takes & TAKES_POLICY) && !a.policy) return bad("policy is NULL");
    if (takes & TAKES_HIDDEN) {
        if (const int st = net_shape_ok(bad, a.hidden, a.hidden2, a.activation, (takes & TAKES_HIDDEN2) ? NET_ROLLOUT2 : NET_HIDDEN)) return st;
    }
    if (takes & TAKES_HEAD) {
        if (a.head != MGYM_HEAD_GREEDY && a.head != MGYM_HEAD_SAMPLE && a.head != MGYM_HEAD_GAUSS) return bad("head must be MGYM_HEAD_GREEDY, MGYM_HEAD_SAMPLE or MGYM_HEAD_GAUSS");
        if (!refusal.empty()) return bad(refusal);
    }
    if ((takes & TAKES_SIGMA) && (!(a.sigma >= 0.0f) || a.sigma > 3.402823466e+38f)) return bad("sigma must be finite and >= 0");   // (a NaN fails the first test)
    if ((takes & DRAWS) && e->cfg.env_id_base % 4 != 0)
        return bad(std::string("env_id_base must be a multiple of 4") + ((takes & TAKES_HEAD) ? " for a drawing head" : "") +
                   ((takes & TAKES_POLICY) ? " (one Philox block serves 4 consecutive global env ids)" : " (policy bits are keyed per 4 consecutive global env ids)"));
    return MGYM_OK;
}

int mgym_rollout_uniform(mgym_env* env, uint64_t policy_seed, int32_t K, void* actions_out, float* obs_out, float* reward_out,
                         uint8_t* done_out, uint8_t* trunc_out) {
    ENV_OR_FAIL(env);
    if (const int st = policy_args_ok(e, "mgym_rollout_uniform", DRAWS, "", PolicyArgs{K})) return st;
    return e->rollout_policy(PolicyCall{ROLL_ACT_UNIFORM, "mgym_rollout_uniform", nullptr, 0, policy_seed}, K, actions_out, obs_out, reward_out, done_out, trunc_out);
}

int mgym_rollout_linear(mgym_env* env, const float* policy, int32_t K, void* actions_out, float* obs_out, float* reward_out,
                        uint8_t* done_out, uint8_t* trunc_out) {
    ENV_OR_FAIL(env);
    if (const int st = policy_args_ok(e, "mgym_rollout_linear", TAKES_POLICY, "", PolicyArgs{K, policy})) return st;
    return e->rollout_policy(PolicyCall{ROLL_ACT_LINEAR, "mgym_rollout_linear", policy, 0, 0}, K, actions_out, obs_out, reward_out, done_out, trunc_out);
}

int mgym_rollout_mlp(mgym_env* env, const float* policy, int32_t hidden, int32_t activation, int32_t K, void* actions_out, float* obs_out,
                     float* reward_out, uint8_t* done_out, uint8_t* trunc_out) {
    ENV_OR_FAIL(env);
    if (const int st = policy_args_ok(e, "mgym_rollout_mlp", TAKES_POLICY | TAKES_HIDDEN, "", PolicyArgs{K, policy, hidden, 0, activation})) return st;
    return e->rollout_policy(PolicyCall{roll_act_mlp_plain(activation), "mgym_rollout_mlp", policy, hidden, 0}, K, actions_out, obs_out, reward_out, done_out,
                             trunc_out);
}

int mgym_rollout_mlp_sample(mgym_env* env, const float* policy, int32_t hidden, int32_t activation, uint64_t policy_seed, uint32_t policy_call, int32_t K,
                            void* actions_out, float* obs_out, float* reward_out, uint8_t* done_out, uint8_t* trunc_out) {
    ENV_OR_FAIL(env);
    const std::string refusal = box_actions(e) ? std::string(kFamilies[e->cfg.kind].name) + " has no discrete actions to draw from (a Gaussian head is not implemented)" : "";
    if (const int st = policy_args_ok(e, "mgym_rollout_mlp_sample", TAKES_POLICY | TAKES_HIDDEN | DRAWS, refusal, PolicyArgs{K, policy, hidden, 0, activation})) return st;
    return e->rollout_policy(PolicyCall{roll_act_mlp_sample(activation), "mgym_rollout_mlp_sample", policy, hidden, policy_seed, policy_call},
                             K, actions_out, obs_out, reward_out, done_out, trunc_out);
}

int mgym_rollout_mlp_gauss(mgym_env* env, const float* policy, int32_t hidden, int32_t activation, float sigma, uint64_t policy_seed, uint32_t policy_call, int32_t K,
                           void* actions_out, float* obs_out, float* reward_out, uint8_t* done_out, uint8_t* trunc_out) {
    ENV_OR_FAIL(env);
    const std::string refusal = box_actions(e) ? "" : std::string(kFamilies[e->cfg.kind].name) + " has discrete actions: use mgym_rollout_mlp_sample";
    if (const int st = policy_args_ok(e, "mgym_rollout_mlp_gauss", TAKES_POLICY | TAKES_HIDDEN | TAKES_SIGMA | DRAWS, refusal, PolicyArgs{K, policy, hidden, 0, activation, 0, sigma}))
        return st;
    return e->rollout_policy(PolicyCall{roll_act_mlp_gauss(activation), "mgym_rollout_mlp_gauss", policy, hidden, policy_seed, policy_call, sigma},
                             K, actions_out, obs_out, reward_out, done_out, trunc_out);
}

int mgym_rollout_mlp2(mgym_env* env, const float* policy, int32_t hidden1, int32_t hidden2, int32_t activation, int32_t head, float sigma, uint64_t policy_seed,
                      uint32_t policy_call, int32_t K, void* actions_out, float* obs_out, float* reward_out, uint8_t* done_out, uint8_t* trunc_out) {
    ENV_OR_FAIL(env);
    std::string refusal;
    if (head == MGYM_HEAD_SAMPLE && box_actions(e)) refusal = std::string("head MGYM_HEAD_SAMPLE: ") + kFamilies[e->cfg.kind].name + " has no discrete actions to draw from (use MGYM_HEAD_GAUSS)";
    if (head == MGYM_HEAD_GAUSS && !box_actions(e)) refusal = std::string("head MGYM_HEAD_GAUSS: ") + kFamilies[e->cfg.kind].name + " has discrete actions (use MGYM_HEAD_SAMPLE)";
    const int takes = TAKES_POLICY | TAKES_HIDDEN | TAKES_HIDDEN2 | TAKES_HEAD | (head == MGYM_HEAD_GAUSS ? TAKES_SIGMA : 0) | (head != MGYM_HEAD_GREEDY ? DRAWS : 0);
    if (const int st = policy_args_ok(e, "mgym_rollout_mlp2", takes, refusal, PolicyArgs{K, policy, hidden1, hidden2, activation, head, sigma})) return st;
    PolicyCall call{roll_act_mlp2(activation, head), "mgym_rollout_mlp2", policy, hidden1, policy_seed, policy_call, sigma};
    call.hidden2 = hidden2;
    return e->rollout_policy(call, K, actions_out, obs_out, reward_out, done_out, trunc_out);
}

int mgym_set_final_obs_out(mgym_env* env, float* final_obs_out, int32_t steps_cap) {
    ENV_OR_FAIL(env);
    if (final_obs_out) {
        if (e->cfg.kind == MGYM_LUNARLANDER) return bad_arg("mgym_set_final_obs_out: final_obs_out is not offered for LunarLander yet (CartPole, MountainCar, MountainCarContinuous, Pendulum and Acrobot only)");
        if (!(e->cfg.flags & MGYM_FLAG_AUTO_RESET))
            return bad_arg("mgym_set_final_obs_out: final_obs_out on a handle without MGYM_FLAG_AUTO_RESET: obs_out already holds the final observation there");
        if (steps_cap < 1) return bad_arg("mgym_set_final_obs_out: steps_cap must be at least 1");
        if (!aligned(final_obs_out, 4)) return bad_arg("mgym_set_final_obs_out: final_obs_out must be 4-byte aligned");
    }
    // (config_epoch stays: graphs captured earlier keep the pointer they froze, like every output pointer)
    e->final_obs = final_obs_out;
    e->final_cap = final_obs_out ? steps_cap : 0;
    return MGYM_OK;
}

int mgym_gae(mgym_env* env, int32_t K, const float* reward, const uint8_t* done, const uint8_t* trunc, const float* value, const float* last_value,
             const float* final_value, float gamma, float lambda, float* adv_out, float* ret_out) {
    ENV_OR_FAIL(env);
    if (K < 1) return bad_arg("mgym_gae: K must be at least 1");
    if (!reward) return bad_arg("mgym_gae: reward is NULL");
    if (!value) return bad_arg("mgym_gae: value is NULL");
    if (!last_value) return bad_arg("mgym_gae: last_value is NULL");
    if (!adv_out && !ret_out) return bad_arg("mgym_gae: adv_out and ret_out are both NULL");
    if (!(gamma >= 0.0f && gamma <= 1.0f)) return bad_arg("mgym_gae: gamma must lie in [0, 1]");   // (a NaN fails the test)
    if (!(lambda >= 0.0f && lambda <= 1.0f)) return bad_arg("mgym_gae: lambda must lie in [0, 1]");
    const struct { const char* name; const float* p; bool out; } fp[] = {{"reward", reward, false}, {"value", value, false}, {"last_value", last_value, false},
                                                                         {"final_value", final_value, false}, {"adv_out", adv_out, true}, {"ret_out", ret_out, true}};
    for (const auto& f : fp)
        if (!aligned(f.p, 4)) return bad_arg((std::string("mgym_gae: ") + f.name + " must be 4-byte aligned").c_str());
    const struct { const char* name; const void* p; } in[] = {{"reward", reward}, {"done", done}, {"trunc", trunc}, {"value", value}, {"last_value", last_value},
                                                              {"final_value", final_value}};
    for (const auto& f : fp)
        for (const auto& g : in)
            if (f.out && f.p && f.p == g.p) return bad_arg((std::string("mgym_gae: ") + f.name + " is the same pointer as " + g.name).c_str());
    if (e->n == 0) return MGYM_OK;
    return gae_launch(e->stream, GaeCall{e->n, K, reward, done, trunc, value, last_value, final_value, gamma, gamma * lambda, adv_out, ret_out});
}

int mgym_value_mlp(mgym_env* env, const float* critic, int32_t hidden1, int32_t hidden2, int32_t activation, int32_t K, const float* obs_first, const float* obs,
                   const float* final_obs, const uint8_t* done, const uint8_t* trunc, float* value_out, float* last_value_out, float* final_value_out) {
    ENV_OR_FAIL(env);
    const Bad bad{"mgym_value_mlp"};
    if (K < 1) return bad("K must be at least 1");
    if (!critic) return bad("critic is NULL");
    if (!obs_first) return bad("obs_first is NULL");
    if (!obs) return bad("obs is NULL");
    if (!value_out) return bad("value_out is NULL");
    if (!last_value_out) return bad("last_value_out is NULL");
    if (const int st = net_shape_ok(bad, hidden1, hidden2, activation, NET_LEARNER)) return st;
    if (final_obs && !final_value_out) return bad("final_value_out is NULL while final_obs is not");
    if (final_value_out && !final_obs) return bad("final_obs is NULL while final_value_out is not");
    if (final_obs && !trunc) return bad("trunc is NULL while final_obs and final_value_out are not");
    if (!final_obs) done = trunc = nullptr;   // ignored without the final arguments
    if (const int st = pointers_ok(bad, {{"obs_first", obs_first, false, 4}, {"obs", obs, false, 4}, {"final_obs", final_obs, false, 4}, {"done", done, false, 0},
                                         {"trunc", trunc, false, 0}, {"value_out", value_out, true, 4}, {"last_value_out", last_value_out, true, 4},
                                         {"final_value_out", final_value_out, true, 4}}, true)) return st;
    if (e->n == 0) return MGYM_OK;
    if (hidden2 >= 1) { if (const int st = e->mlp2_store_to(e->value_dev, critic, e->obs_dim, 1, hidden1, hidden2)) return st; }
    return value_launch(e->stream, ValueCall{e->n, K, obs_first, obs, final_obs, done, trunc, value_out, last_value_out, final_value_out}, e->obs_dim, critic, hidden1,
                        hidden2, activation, e->value_dev);
}

int mgym_logprob_mlp(mgym_env* env, const float* policy, int32_t hidden1, int32_t hidden2, int32_t activation, int32_t head, float sigma, int32_t K,
                     const float* obs_first, const float* obs, const void* actions, float* logp_out) {
    ENV_OR_FAIL(env);
    const Bad bad{"mgym_logprob_mlp"};
    if (K < 1) return bad("K must be at least 1");
    if (!policy) return bad("policy is NULL");
    if (!obs_first) return bad("obs_first is NULL");
    if (!obs) return bad("obs is NULL");
    if (!actions) return bad("actions is NULL");
    if (!logp_out) return bad("logp_out is NULL");
    if (const int st = net_shape_ok(bad, hidden1, hidden2, activation, NET_LEARNER)) return st;
    if (const int st = density_head_ok(bad, e, head, sigma)) return st;
    if (const int st = pointers_ok(bad, {{"obs_first", obs_first, false, 4}, {"obs", obs, false, 4}, {"actions", actions, false, 4}, {"logp_out", logp_out, true, 4}})) return st;
    if (e->n == 0) return MGYM_OK;
    int D = 0, A = 1;
    if (const int st = family_dims(e->cfg.kind, &D, &A)) return st;
    if (hidden2 >= 1) { if (const int st = e->mlp2_store_to(e->logp_dev, policy, D, A, hidden1, hidden2)) return st; }
    const float k = head == MGYM_HEAD_GAUSS ? logp_gauss_k(sigma) : 0.0f;   // f64 on the host, the header's own lines
    return logprob_launch(e->stream, LogpCall{e->n, K, sigma, k, obs_first, obs, static_cast<const uint32_t*>(actions), logp_out}, D, A, policy, hidden1,
                          hidden2, activation, e->logp_dev);
}

// ---- mgym_ppo_grad_mlp / mgym_value_grad_mlp and their two-layer forms: one argument check for the four (ppo: the actor's call; two: hidden2 is taken) ----
struct GradArgs {
    const char* name;
    bool ppo, two;
    const float* weights;
    int32_t hidden, hidden2, activation, head;
    float sigma;
    int32_t K;
    uint64_t env_first, env_count;
    const float *obs_first, *obs;
    const void* actions;
    const float *x0, *x1;   // logp_old, adv | ret, nothing
    float clip, ent_coef;
    void* workspace;
    size_t workspace_bytes;
    float *grad_out, *stats_out;
};

static int grad_call(Env* e, const GradArgs& a) {
    const Bad bad{a.name};
    const char *n0 = a.ppo ? "logp_old" : "ret", *wname = a.ppo ? "policy" : "critic";
    if (a.K < 1) return bad("K must be at least 1");
    if (!a.weights) return bad(std::string(wname) + " is NULL");
    if (!a.obs_first) return bad("obs_first is NULL");
    if (!a.obs) return bad("obs is NULL");
    if (a.ppo && !a.actions) return bad("actions is NULL");
    if (!a.x0) return bad(std::string(n0) + " is NULL");
    if (a.ppo && !a.x1) return bad("adv is NULL");
    if (!a.workspace) return bad("workspace is NULL");
    if (!a.grad_out) return bad("grad_out is NULL");
    if (!a.stats_out) return bad("stats_out is NULL");
    if (const int st = net_shape_ok(bad, a.hidden, a.hidden2, a.activation, a.two ? NET_GRAD2 : NET_HIDDEN)) return st;
    if (a.ppo) { if (const int st = density_head_ok(bad, e, a.head, a.sigma)) return st; }
    if (e->n != 0 && a.env_count == 0) return bad("env_count must be at least 1");   // (a handle without environments has no range to give: MGYM_OK below)
    if (e->n != 0 && (a.env_first > e->n || a.env_count > e->n - a.env_first)) return bad("env_first + env_count exceeds n_envs");
    if (a.ppo && !grad_clip_ok(a.clip)) return bad("clip must be at least 0 and below 1");
    if (a.ppo && !grad_ent_coef_ok(a.ent_coef)) return bad("ent_coef must be finite");
    int D = 0, A = 1;
    if (const int st = family_dims(e->cfg.kind, &D, &A)) return st;
    const uint64_t slab_bytes = a.two ? grad2_slab_bytes(D, A, a.hidden, a.hidden2) : grad_slab_bytes(D, A, a.hidden);
    if (a.workspace_bytes < slab_bytes)
        return bad(std::string("workspace_bytes is below min_bytes of ") + (a.two ? "mgym_grad_workspace_bytes2" : "mgym_grad_workspace_bytes") + " (" + std::to_string(slab_bytes) + ")");
    if (!aligned(a.workspace, 16)) return bad("workspace must be 16-byte aligned");
    if (const int st = pointers_ok(bad, {{"obs_first", a.obs_first, false, 4}, {"obs", a.obs, false, 4}, {"actions", a.actions, false, 4}, {n0, a.x0, false, 4},
                                         {"adv", a.x1, false, 4}, {"workspace", a.workspace, true, 0}, {"grad_out", a.grad_out, true, 4}, {"stats_out", a.stats_out, true, 4}}))
        return st;
    if (e->n == 0) return MGYM_OK;
    const uint64_t fit = a.workspace_bytes / slab_bytes;
    GradCall c{};
    c.n = e->n; c.env_first = a.env_first; c.env_count = a.env_count; c.K = a.K;
    const uint64_t cap = (uint64_t)(a.two ? kGrad2SlabCap : kGradSlabCap);
    c.slabs = (int32_t)(fit < cap ? fit : cap);
    c.lo = 1.0f - a.clip; c.hi = 1.0f + a.clip; c.ent_coef = a.ppo ? a.ent_coef : 0.0f;
    const bool gauss = a.ppo && a.head == MGYM_HEAD_GAUSS;
    c.sigma = a.sigma; c.k = gauss ? logp_gauss_k(a.sigma) : 0.0f; c.ent = gauss ? grad_gauss_entropy(a.sigma) : 0.0f;   // f64 on the host, the headers' own lines
    c.obs_first = a.obs_first; c.obs = a.obs; c.actions = static_cast<const uint32_t*>(a.actions); c.x0 = a.x0; c.x1 = a.x1;
    c.workspace = static_cast<double*>(a.workspace); c.grad_out = a.grad_out; c.stats_out = a.stats_out;
    const int head = !a.ppo ? GRAD_HEAD_VALUE : (gauss ? GRAD_HEAD_GAUSS : GRAD_HEAD_CATEGORICAL);
    if (!a.two) return grad_launch(e->stream, c, D, A, head, a.weights, a.hidden, a.activation);
    float* pack_dev = a.ppo ? e->ppo_grad_dev : e->value_grad_dev;
    if (const int st = e->mlp2_store_to(pack_dev, a.weights, D, a.ppo ? A : 1, a.hidden, a.hidden2)) return st;
    return grad2_launch(e->stream, c, D, A, head, pack_dev, a.hidden, a.hidden2, a.activation);
}

// the workspace query `name` of a gradient call with `depth` hidden layers of the widths hidden[0 .. depth - 1]; cap: the most slabs a launch uses
static int grad_workspace_bytes(const char* name, int kind, int depth, const int32_t (&hidden)[2], int cap, size_t* min_bytes, size_t* best_bytes) {
    const auto bad = [&](const std::string& what) { return bad_arg((std::string(name) + ": " + what).c_str()); };
    int D = 0, A = 1;
    if (family_dims(kind, &D, &A) != MGYM_OK) return bad("unknown kind");
    for (int l = 0; l < depth; ++l)
        if (hidden[l] < 1 || hidden[l] > 64) return bad((depth == 1 ? std::string("hidden") : "hidden" + std::to_string(l + 1)) + " must be between 1 and 64");
    if (!min_bytes || !best_bytes) return bad(!min_bytes ? "min_bytes is NULL" : "best_bytes is NULL");
    *min_bytes = (size_t)(depth == 1 ? grad_slab_bytes(D, A, hidden[0]) : grad2_slab_bytes(D, A, hidden[0], hidden[1]));
    *best_bytes = *min_bytes * (size_t)cap;
    return MGYM_OK;
}

int mgym_grad_workspace_bytes2(int kind, int32_t hidden1, int32_t hidden2, size_t* min_bytes, size_t* best_bytes) {
    return grad_workspace_bytes("mgym_grad_workspace_bytes2", kind, 2, {hidden1, hidden2}, kGrad2SlabCap, min_bytes, best_bytes);
}

int mgym_ppo_grad_mlp2(mgym_env* env, const float* policy, int32_t hidden1, int32_t hidden2, int32_t activation, int32_t head, float sigma, int32_t K,
                       uint64_t env_first, uint64_t env_count, const float* obs_first, const float* obs, const void* actions, const float* logp_old,
                       const float* adv, float clip, float ent_coef, void* workspace, size_t workspace_bytes, float* grad_out, float* stats_out) {
    ENV_OR_FAIL(env);
    return grad_call(e, GradArgs{"mgym_ppo_grad_mlp2", true, true, policy, hidden1, hidden2, activation, head, sigma, K, env_first, env_count, obs_first, obs, actions,
                                 logp_old, adv, clip, ent_coef, workspace, workspace_bytes, grad_out, stats_out});
}

int mgym_value_grad_mlp2(mgym_env* env, const float* critic, int32_t hidden1, int32_t hidden2, int32_t activation, int32_t K, uint64_t env_first,
                         uint64_t env_count, const float* obs_first, const float* obs, const float* ret, void* workspace, size_t workspace_bytes, float* grad_out,
                         float* stats_out) {
    ENV_OR_FAIL(env);
    return grad_call(e, GradArgs{"mgym_value_grad_mlp2", false, true, critic, hidden1, hidden2, activation, 0, 0.0f, K, env_first, env_count, obs_first, obs, nullptr,
                                 ret, nullptr, 0.0f, 0.0f, workspace, workspace_bytes, grad_out, stats_out});
}

int mgym_grad_workspace_bytes(int kind, int32_t hidden, size_t* min_bytes, size_t* best_bytes) {
    return grad_workspace_bytes("mgym_grad_workspace_bytes", kind, 1, {hidden, 0}, kGradSlabCap, min_bytes, best_bytes);
}

int mgym_ppo_grad_mlp(mgym_env* env, const float* policy, int32_t hidden, int32_t activation, int32_t head, float sigma, int32_t K, uint64_t env_first,
                      uint64_t env_count, const float* obs_first, const float* obs, const void* actions, const float* logp_old, const float* adv, float clip,
                      float ent_coef, void* workspace, size_t workspace_bytes, float* grad_out, float* stats_out) {
    ENV_OR_FAIL(env);
    return grad_call(e, GradArgs{"mgym_ppo_grad_mlp", true, false, policy, hidden, 0, activation, head, sigma, K, env_first, env_count, obs_first, obs, actions, logp_old, adv,
                                 clip, ent_coef, workspace, workspace_bytes, grad_out, stats_out});
}

int mgym_value_grad_mlp(mgym_env* env, const float* critic, int32_t hidden, int32_t activation, int32_t K, uint64_t env_first, uint64_t env_count,
                        const float* obs_first, const float* obs, const float* ret, void* workspace, size_t workspace_bytes, float* grad_out, float* stats_out) {
    ENV_OR_FAIL(env);
    return grad_call(e, GradArgs{"mgym_value_grad_mlp", false, false, critic, hidden, 0, activation, 0, 0.0f, K, env_first, env_count, obs_first, obs, nullptr, ret, nullptr,
                                 0.0f, 0.0f, workspace, workspace_bytes, grad_out, stats_out});
}

int mgym_episode_returns(mgym_env* env, int32_t K, const float* reward, const uint8_t* done, const uint8_t* trunc, float* ep_return, uint32_t* ep_length,
                         float* return_out, uint32_t* length_out) {
    ENV_OR_FAIL(env);
    if (K < 1) return bad_arg("mgym_episode_returns: K must be at least 1");
    if (!reward) return bad_arg("mgym_episode_returns: reward is NULL");
    if (!ep_return) return bad_arg("mgym_episode_returns: ep_return is NULL");
    if (!ep_length) return bad_arg("mgym_episode_returns: ep_length is NULL");
    const struct { const char* name; const void* p; } wp[] = {{"reward", reward}, {"ep_return", ep_return}, {"ep_length", ep_length}, {"return_out", return_out},
                                                              {"length_out", length_out}};
    for (const auto& f : wp)
        if (!aligned(f.p, 4)) return bad_arg((std::string("mgym_episode_returns: ") + f.name + " must be 4-byte aligned").c_str());
    if (e->n == 0) return MGYM_OK;
    return episode_returns_launch(e->stream, EpCall{e->n, K, reward, done, trunc, ep_return, ep_length, return_out, length_out});
}

int mgym_episode_count(mgym_env* env, uint64_t* finished) {
    ENV_OR_FAIL(env);
    if (!finished) return bad_arg("mgym_episode_count: NULL");
    MGYM_HIP(hipMemcpyAsync(e->h_done, e->d_done, kDoneShards * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
    MGYM_HIP(hipStreamSynchronize(e->stream));
    uint64_t tot = 0;
    for (int i = 0; i < kDoneShards; ++i) tot += e->h_done[i];
    *finished = tot;
    return MGYM_OK;
}

int mgym_observation(mgym_env* env, const float** obs, uint64_t* col_stride) {
    ENV_OR_FAIL(env);
    if (!obs || !col_stride) return bad_arg("mgym_observation: NULL out pointer");
    return e->observation(obs, col_stride);
}

int mgym_observation_aos(mgym_env* env, float* out_aos) {
    ENV_OR_FAIL(env);
    if (!out_aos && e->n) return bad_arg("mgym_observation_aos: out is NULL");
    if (e->n == 0) return MGYM_OK;
    const float* obs = nullptr;
    uint64_t stride = 0;
    int st = e->observation(&obs, &stride);
    if (st != MGYM_OK) return st;
    hipLaunchKernelGGL(obs_to_aos_kernel, dim3((unsigned)((e->n + 255) / 256)), dim3(256), 0, e->stream, obs, stride, e->obs_dim, e->n, out_aos);
    MGYM_HIP(hipGetLastError());
    return MGYM_OK;
}

int mgym_get_state(mgym_env* env, void* blob) {
    ENV_OR_FAIL(env);
    if (!blob && e->n) return bad_arg("mgym_get_state: blob is NULL");
    return e->get_state(blob);
}

int mgym_set_state(mgym_env* env, const void* blob) {
    ENV_OR_FAIL(env);
    if (!blob && e->n) return bad_arg("mgym_set_state: blob is NULL");
    return e->set_state(blob);
}

int mgym_get_elapsed_steps(mgym_env* env, uint32_t* out) {
    ENV_OR_FAIL(env);
    if (!out && e->n) return bad_arg("mgym_get_elapsed_steps: out is NULL");
    return e->elapsed(out, nullptr);
}

int mgym_set_elapsed_steps(mgym_env* env, const uint32_t* in) {
    ENV_OR_FAIL(env);
    if (!in && e->n) return bad_arg("mgym_set_elapsed_steps: in is NULL");
    return e->elapsed(nullptr, in);
}

int mgym_set_dispersion_override(mgym_env* env, const float* disp) {
    ENV_OR_FAIL(env);
    return e->set_dispersion(disp);
}

int mgym_sync(mgym_env* env) {
    ENV_OR_FAIL(env);
    MGYM_HIP(hipMemcpyAsync(e->h_err, e->d_err, sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
    MGYM_HIP(hipMemsetAsync(e->d_err, 0, sizeof(uint32_t), e->stream));
    MGYM_HIP(hipStreamSynchronize(e->stream));
    uint32_t bits = *e->h_err;
    if (bits & DEV_ERR_INVALID_ACTION) {
        set_last_error("invalid action: assertion `action_space.contains(&action)` failed for at least one environment");
        return MGYM_ERR_INVALID_ACTION;
    }
    if (bits & DEV_ERR_CONTACT_OVERFLOW) {
        set_last_error("LunarLander: contact cache overflow (more than 12 body/ground-edge pairs with overlapping broad-phase boxes in one "
                       "environment: a pair was dropped; that environment's results are undefined until it is reset)");
        return MGYM_ERR_CAPACITY;
    }
    if (bits & DEV_ERR_SOLVER_OVERFLOW) {
        set_last_error("LunarLander: island solver overflow (more than 9 touching contacts in one environment: the extra constraints were "
                       "not solved; that environment's results are undefined until it is reset)");
        return MGYM_ERR_CAPACITY;
    }
    if (bits & DEV_ERR_INTERNAL) {
        set_last_error("LunarLander: internal error — a finished environment had no fitting prepared reset while the engine believed every one had "
                       "(staged resets, lunar_lander.hip direct_possible); that environment was not reset.  Please report; MGYM_LL_STAGED_RESET=0 avoids the path");
        return MGYM_ERR_HIP;
    }
    if (bits & DEV_ERR_NOT_RESET) {
        set_last_error("You forgot to call reset()");
        return MGYM_ERR_NOT_RESET;
    }
    return MGYM_OK;
}

const char* mgym_last_error(void) { return g_last_error.c_str(); }

int mgym_get_info(mgym_env* env, char* buf, size_t cap) {
    ENV_OR_FAIL(env);
    if (!buf || cap == 0) return bad_arg("mgym_get_info: buf is NULL or cap is 0");
    std::string out = std::string("kind=") + kFamilies[e->kind].key +"\nn_envs=" + std::to_string(e->n) + "\ndevice=" + std::to_string(e->cfg.device) +
                      "\nauto_reset=" + ((e->cfg.flags & MGYM_FLAG_AUTO_RESET) ? "1" : "0") + "\nmax_episode_steps=" + std::to_string(e->cfg.max_episode_steps) +
                      "\nGPU_MAX_HW_QUEUES=" + e->hwq_env + "\n";
    int st = e->info(out);
    if (st != MGYM_OK) return st;
    if (out.size() + 1 > cap) { buf[0] = 0; return bad_arg("mgym_get_info: buffer too small"); }
    memcpy(buf, out.c_str(), out.size() + 1);
    return MGYM_OK;
}

int mgym_malloc(int device, size_t bytes, void** out) {
    if (!out) return bad_arg("mgym_malloc: NULL");
    DeviceGuard guard(device);
    if (!guard.ok) { set_last_error("mgym_malloc: no such HIP device"); return MGYM_ERR_NO_DEVICE; }
    MGYM_HIP(hipMalloc(out, bytes ? bytes : 16));
    return MGYM_OK;
}

int mgym_free(int device, void* ptr) {
    DeviceGuard guard(device);
    MGYM_HIP(hipFree(ptr));
    return MGYM_OK;
}

// The engine's kernels run on a hipStreamNonBlocking stream, which the null stream does not order against: these
// helpers therefore return only when the copy has fully completed (hipMemcpy blocks the host; the explicit null-stream
// synchronise covers staged pageable-memory copies), so a launch issued afterwards on any stream sees the data.
int mgym_memcpy_h2d(int device, void* dst, const void* src, size_t bytes) {
    DeviceGuard guard(device);
    if (bytes) {
        MGYM_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
        MGYM_HIP(hipStreamSynchronize(nullptr));
    }
    return MGYM_OK;
}

int mgym_memcpy_d2h(int device, void* dst, const void* src, size_t bytes) {
    DeviceGuard guard(device);
    if (bytes) MGYM_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return MGYM_OK;
}

int mgym_timer_start(mgym_env* env) {
    ENV_OR_FAIL(env);
    MGYM_HIP(hipEventRecord(e->ev0, e->stream));
    return MGYM_OK;
}

int mgym_timer_stop(mgym_env* env, float* elapsed_ms) {
    ENV_OR_FAIL(env);
    if (!elapsed_ms) return bad_arg("mgym_timer_stop: NULL");
    MGYM_HIP(hipEventRecord(e->ev1, e->stream));
    MGYM_HIP(hipEventSynchronize(e->ev1));
    MGYM_HIP(hipEventElapsedTime(elapsed_ms, e->ev0, e->ev1));
    return MGYM_OK;
}

int mgym_graph_begin(mgym_env* env) {
    ENV_OR_FAIL(env);
    { int st = e->join_helpers(); if (st != MGYM_OK) return st; }  // helper-stream work issued so far is waited for OUTSIDE the capture
    MGYM_HIP(hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal));
    return MGYM_OK;
}

// What mgym_graph_end hands out: the executable graph and the handle configuration it was captured under.  Kernel arguments are
// frozen at capture — among them the dispersion source of mgym_set_dispersion_override — so a graph captured under another
// configuration is refused at launch (loudly) instead of silently stepping with the old one.
struct GraphBox { hipGraphExec_t exec; uint64_t config_epoch; };

int mgym_graph_end(mgym_env* env, void** graph_exec_out) {
    ENV_OR_FAIL(env);
    if (!graph_exec_out) return bad_arg("mgym_graph_end: NULL");
    hipGraph_t g = nullptr;
    { int st = e->join_helpers(); if (st != MGYM_OK) return st; }
    MGYM_HIP(hipStreamEndCapture(e->stream, &g));
    hipGraphExec_t ge = nullptr;
    hipError_t err = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (err != hipSuccess) return hip_fail(err, "hipGraphInstantiate", __FILE__, __LINE__);
    *graph_exec_out = new GraphBox{ge, e->config_epoch};
    return MGYM_OK;
}

int mgym_graph_launch(mgym_env* env, void* graph_exec) {
    ENV_OR_FAIL(env);
    if (!graph_exec) return bad_arg("mgym_graph_launch: NULL");
    GraphBox* b = static_cast<GraphBox*>(graph_exec);
    if (b->config_epoch != e->config_epoch)
        return bad_arg("mgym_graph_launch: the handle's configuration has changed since this graph was captured (mgym_set_dispersion_override): capture it again");
    MGYM_HIP(hipGraphLaunch(b->exec, e->stream));
    return MGYM_OK;
}

int mgym_graph_destroy(void* graph_exec) {
    if (graph_exec) {
        GraphBox* b = static_cast<GraphBox*>(graph_exec);
        hipError_t err = hipGraphExecDestroy(b->exec);
        delete b;
        MGYM_HIP(err);
    }
    return MGYM_OK;
}

}  // extern "C"
