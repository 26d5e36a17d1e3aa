/* mgym.h — C ABI of libmgym: the MI355X (gfx950) batched environment-step engine.
 *
 * This is the drop-in boundary for the hot path of ModuRL/ModuRL_Gym: the bodies of
 * `impl Gym for CartPoleV1 / MountainCarV0 / LunarLanderV3` — reset() and step() —
 * re-expressed as struct-of-arrays HIP kernels over n_envs independent environments.
 * Plain C: opaque handle, raw device pointers, sizes and status codes; no C++ or
 * PyTorch types.  Each entry point cites the reference interface it replaces
 * (paths relative to the reference repo).  A Rust `Gym` shim / cgo / ctypes stub binds
 * exactly these symbols.
 *
 * Conventions
 *  - All `*_out` / `actions` / `mask` / `blob` pointers are DEVICE pointers on the
 *    env's HIP device.  The engine owns only its internal state (its layout is private: columns for
 *    CartPole / MountainCar, one record per env for LunarLander — DESIGN.md section 3); callers own
 *    every buffer they pass.  No allocation or synchronisation happens inside
 *    mgym_reset/mgym_step/mgym_reset_done (they are hipGraph-capturable).
 *  - Observations are SoA: obs_out[k * n_envs + i] is component k of env i
 *    (reference: rank-1 f32 tensor of 4 / 2 / 8 per env — cartpole.rs:285-290,
 *    mountain_car.rs:315, lunar_lander.rs:1112-1123).
 *  - Discrete actions are uint32_t[n_envs] (reference: rank-0 u32 tensor,
 *    cartpole.rs:257,377); MountainCarContinuous and Pendulum take float[n_envs].
 *  - reward f32, done/truncated uint8 (StepInfo, cartpole.rs:300-305).
 *  - Episode semantics are the reference's: NO auto-reset; stepping a finished env
 *    keeps integrating (cartpole.rs:330-346).  MGYM_FLAG_AUTO_RESET opts into a fused
 *    same-step reset (a superset feature, off by default).
 *  - Where the reference panics (assert!/expect) the engine returns a status code;
 *    errors detected on the device (invalid action) are sticky and reported by the
 *    next mgym_sync().
 *  - One handle = one device + one stream; calls on one handle are not thread-safe,
 *    different handles are independent (reference: &mut self, single-threaded).
 */
#ifndef MGYM_H
#define MGYM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGYM_ABI_VERSION 4

typedef struct mgym_env mgym_env;

typedef enum mgym_status {
    MGYM_OK = 0,
    MGYM_ERR_INVALID_ACTION = 1, /* assert!(action_space.contains(&action)): cartpole.rs:252, mountain_car.rs:294 */
    MGYM_ERR_NOT_RESET = 2,      /* assert!(self.lander.is_some(), "You forgot to call reset()"): lunar_lander.rs:920 */
    MGYM_ERR_BAD_CONFIG = 3,     /* assert!(-12.0 < gravity && gravity < 0.0): lunar_lander.rs:292-296 */
    MGYM_ERR_HIP = 4,            /* HIP runtime failure (reference: candle_core::Error from tensor ops) */
    MGYM_ERR_BAD_ARG = 5,        /* null/misaligned pointer, wrong kind */
    MGYM_ERR_NO_DEVICE = 6,      /* no gfx950 device / HIP runtime unusable: the engine has no CPU fallback */
    MGYM_ERR_CAPACITY = 7        /* LunarLander: more body/ground-edge pairs than the per-env contact cache holds (12: reachable only
                                    at horizontal speeds > 8 m/s next to the ground) or more touching contacts than the island solver
                                    holds (9 = the geometric bound of the scene); mgym_last_error() says which.  The affected
                                    environment's results are undefined until it is reset.  The reference has no such limit. */
} mgym_status;

typedef enum mgym_kind {
    MGYM_CARTPOLE = 0,         /* CartPoleV1      — src/classic_control/cartpole.rs */
    MGYM_MOUNTAINCAR = 1,      /* MountainCarV0   — src/classic_control/mountain_car.rs */
    MGYM_MOUNTAINCAR_CONT = 2, /* MountainCarContinuous-v0 — NOT in the reference (parity unpinned) */
    MGYM_LUNARLANDER = 3,      /* LunarLanderV3   — src/box_2d/lunar_lander.rs */
    MGYM_PENDULUM = 4,         /* Pendulum-v1 — NOT in the reference (parity unpinned); defined below */
    MGYM_ACROBOT = 6           /* Acrobot-v1 — NOT in the reference (parity unpinned); defined below.  5 is not assigned: it stays the
                                  "unknown kind" it has always been (MGYM_ERR_BAD_ARG from every entry point that takes a kind), and a
                                  later family does not take it either */
} mgym_kind;

/* MGYM_PENDULUM = 4 is gymnasium's Pendulum-v1 with m = l = 1, dt = 0.05, max_speed = 8 and max_torque = 2.  It is not in the reference: parity
 * unpinned, as for MGYM_MOUNTAINCAR_CONT.  Gymnasium integrates in float64; this engine is f32, so the f32 words are defined here exactly.  All
 * arithmetic is f32, nothing is fused and nothing is reassociated.
 *
 * Constants:
 *     PI_F  = 3.14159274f        TWO_PI_F = 6.28318548f
 *     c_g   = 1.5f * g           one f32 multiply on the host
 *  - g is mgym_config::gravity.
 *  - mgym_default_config(MGYM_PENDULUM) sets gravity to 10.0f.
 *  - mgym_create rejects a non-finite g with MGYM_ERR_BAD_CONFIG.
 *  - The other config fields are ignored (max_episode_steps, flags and the batching / sharding fields mean what they mean for every family).
 *
 * State per environment: th, thdot, and a u32 episode number.  th is not wrapped and grows without bound, as in gymnasium.
 * The observation is (cos th, sin th, thdot), using mg_cosf and mg_sinf (csrc/mgym_math.h), i.e. glibc's cosf and sinf.
 *
 * Step with action word a (an f32):
 *     if a is NaN: sticky MGYM_ERR_INVALID_ACTION, reward 0, done 0, state untouched
 *     u      = a < -2 ? -2 : (a > 2 ? 2 : a)
 *     x      = th + PI_F
 *     r      = fmodf(x, TWO_PI_F);  if (r < 0) r += TWO_PI_F      (fmod is exact by definition: every correct fmodf gives the same word)
 *     an     = r - PI_F
 *     cost   = (an*an + 0.1f*(thdot*thdot)) + 0.001f*(u*u)
 *     acc    = c_g * sinf(th) + 3.0f * u
 *     thdot' = clamp(thdot + acc * 0.05f, -8, 8)                  (the same compare form as u)
 *     th'    = th + thdot' * 0.05f
 *     obs    = (cosf(th'), sinf(th'), thdot');   reward = -cost;   done = 0 always
 *  - The NaN case follows the MountainCarContinuous rule (+-inf is a valid action and clamps; under a time limit the elapsed count advances on every
 *    step, a refused one included, as MountainCar's does).
 *  - truncated and MGYM_FLAG_AUTO_RESET follow max_episode_steps exactly as they do for MountainCar: the limit is 0 (off, the default) or 1 .. 65535;
 *    the count is a u16, saturating; the reset is fused in place on done | truncated.  Pendulum has no termination, so with the limit off an episode
 *    never ends.  Gymnasium registers Pendulum-v1 with a limit of 200.
 *
 * Reset: the draw is env_draw(seed, env_id_base + i, episode, SLOT_RESET0) (csrc/philox.h), words w0 .. w3;
 *     th = uniform_f64_to_f32(-pi, pi, w0, w1) and thdot = uniform_f64_to_f32(-1, 1, w2, w3), with pi the double M_PI
 * (uniform_f64_to_f32(lo, hi, a, b) = (float)(u53(a, b) * (hi - lo) + lo) in f64, u53 the 53-bit uniform of every family's reset).  Then
 * episode += 1 and elapsed = 0.  mgym_reset_deterministic sets th = 0, thdot = 0, so the observation is (1, 0, 0); mgym_create leaves that state too.
 *
 * mgym_get_spec: obs_dim 3, n_actions 0, action_is_float 1; action_low / action_high -2 / 2; obs_low / obs_high -+(1, 1, 8); state_cols 3.
 * State blob: columns th, thdot, episode.  mgym_set_state recomputes the stored cos and sin and sets elapsed to 0.  mgym_get_elapsed_steps and
 * mgym_set_elapsed_steps behave as for MountainCar.  mgym_observation is a zero-copy view: the engine keeps cos, sin, thdot as three adjacent
 * columns with stride n_pad.
 *
 * Policies, all taking the observation held before the step, with actions_out holding f32 words:
 *  - mgym_rollout_uniform: word g % 4 of Philox(key = policy_seed; counter = (g & ~3 lo, g & ~3 hi, uniform call count, 0x40000000 + t));
 *    a = (float)(w >> 8) * 2^-22 - 2.0f, which is exact, over the multiples of 2^-22 in [-2, 2); n_envs and env_id_base must be multiples of 4.
 *  - mgym_rollout_linear: policy holds 4 floats (w_cos, w_sin, w_thdot, b), and a = ((w0*c + w1*s) + w2*thdot) + b.  The step clamps a.
 *  - mgym_rollout_mlp: D = 3, A = 1, and s_0 is the torque, exactly as in the MountainCarContinuous form.
 *  - mgym_rollout_mlp_sample: MGYM_ERR_BAD_ARG before any launch (no discrete actions to draw from).
 *  - mgym_rollout_mlp_gauss: D = 3, A = 1, the torque is s_0 + sigma * z (the text of that entry point); the step clamps it.
 *  - The fused forms need n_envs to be a multiple of 4 and the buffers 16-byte aligned; mgym_rollout with an action table falls back to K steps
 *    otherwise, as MountainCar's does. */

/* MGYM_ACROBOT = 6 is gymnasium's Acrobot-v1: the "book" dynamics with m1 = m2 = l1 = 1, lc1 = lc2 = 0.5, I1 = I2 = 1, g = 9.8, dt = 0.2, one RK4 step and
 * no torque noise.  It is not in the reference: parity unpinned, as for MGYM_PENDULUM.  Gymnasium integrates in float64; this engine is f32, so the f32
 * words are defined here exactly.  All arithmetic is f32, every operation is individually rounded, nothing is fused and nothing is reassociated.  The
 * cos(x - pi/2) terms of the dynamics are written as sines and sin(th1 + th2) by the addition formula, so one (sin, cos) pair per angle serves a
 * derivative evaluation.
 *
 *     PI_F = 3.14159274f   TWO_PI_F = 6.28318548f   V1 = (float)(4 pi)   V2 = (float)(9 pi)
 *     h = 0.1f   dt = 0.2f   dt6 = 0.2f / 6.0f (one f32 divide)
 *
 *     deriv(th1, th2, w1, w2, tau):
 *         s1, c1 = sinf(th1), cosf(th1);   s2, c2 = sinf(th2), cosf(th2)     mg_sinf / mg_cosf (csrc/mgym_math.h), i.e. glibc's
 *         s12  = s1*c2 + c1*s2
 *         d1   = 3.5f + c2
 *         d2   = 1.25f + 0.5f*c2
 *         phi2 = 4.9f * s12
 *         phi1 = (((-(0.5f*(w2*w2))*s2) - (w2*w1)*s2) + 14.7f*s1) + phi2
 *         dd2  = (((tau + (d2/d1)*phi1) - (0.5f*(w1*w1))*s2) - phi2) / (1.25f - (d2*d2)/d1)
 *         dd1  = -((d2*dd2 + phi1) / d1)
 *         return (w1, w2, dd1, dd2)
 *
 *     step, action word a (u32):
 *         a > 2: sticky MGYM_ERR_INVALID_ACTION, reward 0, done 0, state untouched (MountainCar's rule, the elapsed count included: it advances)
 *         tau = (float)a - 1.0f
 *         k1 = deriv(y);  k2 = deriv(y + h*k1);  k3 = deriv(y + h*k2);  k4 = deriv(y + dt*k3)      (componentwise, one multiply and one add)
 *         y' = y + dt6 * (((k1 + 2.0f*k2) + 2.0f*k3) + k4)
 *         th1', th2':  if (x > PI_F || x < -PI_F) { r = fmodf(x + PI_F, TWO_PI_F); if (r < 0) r += TWO_PI_F; x = r - PI_F; }
 *         w1' = clamp(w1', -V1, V1);  w2' = clamp(w2', -V2, V2)      (Pendulum's compare form: a NaN passes through)
 *         obs = (cos th1', sin th1', cos th2', sin th2', w1', w2')
 *         done = (-c1' - (c1'*c2' - s1'*s2')) > 1.0f          from the observation's own words
 *         reward = done ? 0.0f : -1.0f
 *  - The wrap is loop-free on purpose: gymnasium's `while x > pi: x -= 2 pi` never ends for an infinity, and no data-dependent loop appears anywhere in
 *    the step.  A non-finite state (reachable only through mgym_set_state) yields NaNs, done = 0, and the call returns.
 *  - A finished environment that is stepped again keeps integrating: done is recomputed by every step, nothing is sticky.
 *  - max_episode_steps (0 = off, 1 .. 65535; gymnasium registers Acrobot-v1 with 500) and MGYM_FLAG_AUTO_RESET (the fused reset on done | truncated)
 *    follow MountainCar's rules exactly.  The other config fields (gravity, wind, ...) are ignored.
 *
 * Reset: th1, th2 = uniform_f64_to_f32(-0.1, 0.1, w0, w1), (.., w2, w3) of env_draw(seed, env_id_base + i, episode, SLOT_RESET0) and w1, w2 the same of
 * env_draw(.., SLOT_RESET1) (csrc/philox.h).  Then episode += 1 and elapsed = 0.  mgym_reset_deterministic sets the four state words to 0, so the
 * observation is (1, 0, 1, 0, 0, 0); mgym_create leaves that state too.
 *
 * mgym_get_spec: obs_dim 6, n_actions 3, action_is_float 0; obs_high (1, 1, 1, 1, V1, V2), obs_low its negative; state_cols 5.
 * State blob: columns th1, th2, w1, w2, episode.  mgym_set_state takes the angle and velocity words as they are (no wrap, no clamp), recomputes the
 * stored cos and sin words and sets elapsed to 0.  mgym_get_elapsed_steps and mgym_set_elapsed_steps behave as for MountainCar.  mgym_observation is a
 * zero-copy view: the engine keeps the six observation words as adjacent columns with stride n_pad.
 *
 * Policies, all taking the observation o held before the step, with actions_out holding u32 words:
 *  - mgym_rollout_uniform: MountainCar's Discrete(3) draw — word g % 4 of Philox(key = policy_seed; counter = (g & ~3 lo, g & ~3 hi, uniform call count,
 *    0x40000000 + t / 2)), its low half at even t and its high half at odd t, h, and a = (3 h) >> 16.
 *  - mgym_rollout_linear: policy holds three rows of (6 weights, bias), 21 floats; s_j = ((((((w_j0 o0 + w_j1 o1) + w_j2 o2) + w_j3 o3) + w_j4 o4) + w_j5 o5) + b_j
 *    and the sequential strict argmax of the LunarLander form.
 *  - mgym_rollout_mlp: D = 6, A = 3.  mgym_rollout_mlp_sample: A = 3.  mgym_rollout_mlp_gauss: MGYM_ERR_BAD_ARG before any launch (discrete actions).
 *  - The fused forms need n_envs to be a multiple of 4 and the buffers 16-byte aligned (env_id_base a multiple of 4 where a draw is involved);
 *    mgym_rollout with an action table falls back to K steps otherwise, as MountainCar's does.
 *  - mgym_set_final_obs_out is offered. */

enum {
    MGYM_FLAG_AUTO_RESET = 1u /* fused same-step reset of finished envs inside mgym_step (superset; default off) */
};

/* Builder arguments of the three reference constructors, plus batching/sharding fields.
 *   CartPoleV1::builder():  sutton_barto_reward=false, is_euler=true      (cartpole.rs:36-44)
 *   MountainCarV0::builder(): goal_velocity=0.0                           (mountain_car.rs:27-34)
 *   LunarLanderV3::builder(): gravity=-10, enable_wind=false, wind_power=15,
 *                             turbulence_power=1.5, seed                  (lunar_lander.rs:280-291)
 * `device` is the HIP ordinal (reference: candle Device).  `env_id_base` is the global index
 * of this handle's env 0: per-env random streams are keyed by (seed, env_id_base + i), so
 * results do not depend on how a population is sharded over GPUs. */
typedef struct mgym_config {
    uint32_t struct_size; /* = sizeof(mgym_config) */
    int32_t kind;         /* mgym_kind */
    int32_t device;
    uint32_t flags;
    uint64_t n_envs;
    uint64_t env_id_base;
    uint64_t seed;
    int32_t sutton_barto_reward;
    int32_t is_euler;
    float goal_velocity;
    float gravity;
    int32_t enable_wind;
    float wind_power;
    float turbulence_power;
    uint32_t max_episode_steps; /* episode time limit in caller-visible steps; 0 = off (the reference's behaviour).  See below. */
} mgym_config;

/* max_episode_steps — an episode time limit inside the step kernels (NOT in the reference: its MountainCarV0 and LunarLanderV3 never
 * truncate, mountain_car.rs:324-329, lunar_lander.rs:1165; this is gymnasium's TimeLimit rule, and the one thing a caller of the fused
 * mgym_rollout* launches cannot add from outside).  0 = off: every output word and every step / rollout kernel is what it is without the field (MountainCar's reset and state-import
 * kernels additionally clear a 2-byte count per environment they touch).
 *   1 .. 65535: MountainCar, MountainCarContinuous, Pendulum, Acrobot, LunarLander.  Larger: MGYM_ERR_BAD_CONFIG.
 *   CartPole keeps the reference's 500 (cartpole.rs:297): it accepts 0 and 500, which both mean what it does today, and rejects
 *   anything else with MGYM_ERR_BAD_CONFIG.
 * Every environment has an ELAPSED count of caller-visible steps since its last reset: 0 after mgym_reset / mgym_reset_done /
 * mgym_reset_deterministic (for the environments they reset) and after an auto-reset; LunarLander's implicit step(0) inside reset()
 * (lunar_lander.rs:911-916) does not count.  A step first does exactly what it does without a limit — the same obs, reward and done
 * words — then elapsed += 1 and truncated = (elapsed >= max_episode_steps).  `done` is not changed by the limit (both flags can be 1
 * on one step); no reward is added or removed.  The same for every entry point that steps (mgym_step, mgym_rollout,
 * mgym_rollout_uniform, mgym_rollout_linear, replays of graphs captured from them: the count lives in device memory).
 * Without MGYM_FLAG_AUTO_RESET an environment stepped past its limit keeps integrating and reports truncated = 1 on every later step
 * (the count saturates, it never wraps).  With it, "finished" is done | truncated: the environment is reset in the same step by the
 * same route and with the same Philox keys as a `done` one, and obs_out of that step holds the reset observation.
 * The final observation of an episode that ends under auto-reset (by either flag) is delivered through mgym_set_final_obs_out for CartPole,
 * MountainCar, MountainCarContinuous, Pendulum and Acrobot; for LunarLander it is not delivered yet. */

/* Space metadata (reference: observation_space()/action_space(), cartpole.rs:58-69,350-356;
 * mountain_car.rs:42-48; lunar_lander.rs:1169-1200). */
typedef struct mgym_spec {
    int32_t obs_dim;
    int32_t n_actions;      /* Discrete(n); 0 for a continuous (Box) action space */
    int32_t action_is_float;
    int32_t state_cols;     /* columns of the get/set_state blob */
    float obs_low[8], obs_high[8];
    float action_low, action_high; /* continuous only */
} mgym_spec;

int mgym_abi_version(void);

/* Fill `cfg` with the reference builder defaults for `kind` (n_envs = 1, device 0, seed 0). */
int mgym_default_config(int kind, mgym_config *cfg);

/* Replaces {CartPoleV1,MountainCarV0,LunarLanderV3}::builder()...build()
 * (cartpole.rs:37-96, mountain_car.rs:27-69, lunar_lander.rs:281-352).
 * Initial state as constructed by the reference: zeros; CartPole steps_beyond_terminated=Some(0).
 * Populations per handle.  The 16-byte kernels address the engine's columns by 32-bit byte offsets from one buffer resource, which bounds n_envs:
 *   CartPole: at most 134 217 728 (2^27) environments; a larger n_envs is refused with MGYM_ERR_BAD_ARG before anything is allocated (shard larger
 *     populations over handles: env_id_base makes the split invisible).
 *   MountainCar, MountainCarContinuous, Pendulum: the 16-byte step kernel runs up to 2^27 environments, Acrobot's up to 2^26; beyond that (as for n_envs no
 *     multiple of 4 or buffers off their alignment) mgym_step runs the generic kernel with 64-bit addresses — the same words, any n_envs.
 *   LunarLander: any n_envs; mgym_rollout's persistent launch needs n_envs <= 16 777 215 and its records (1152 bytes per environment, n_envs rounded up to
 *     a multiple of 1024) below 4 GiB, that is at most 3 727 360 environments; beyond that it runs as K steps (mgym_get_info: rollout=k_steps).  (By default the engine
 *     chooses K steps long before that bound: see mgym_rollout.)
 * Every [K][n_envs] buffer of the rollout entry points, of mgym_set_final_obs_out, mgym_gae, mgym_value_mlp and mgym_episode_returns may exceed 4 GiB: rows are addressed
 * in 64 bits.  The one exception is CartPole's fused rollout kernel (mgym_rollout below). */
int mgym_create(const mgym_config *cfg, mgym_env **out);
int mgym_destroy(mgym_env *env);

/* Launch stream (hipStream_t).  Default: a stream created by the engine.  Every call is ordered on this stream as far
 * as the caller can tell.  A LunarLander step may run part of its kernels on an engine-owned helper stream, forked
 * from and joined back into this stream by events inside the call (so it is also capturable by mgym_graph_begin). */
int mgym_set_stream(mgym_env *env, void *hip_stream);
void *mgym_get_stream(mgym_env *env);

/* Gym::reset (cartpole.rs:238-249, mountain_car.rs:279-291, lunar_lander.rs:727-917) for the
 * envs with mask[i] != 0 (mask == NULL: all).  obs_out may be NULL. */
int mgym_reset(mgym_env *env, const uint8_t *mask, float *obs_out);

/* mgym_reset with mask = done | truncated (either may be NULL): the "reset what just finished"
 * call a rollout loop issues after every step. */
int mgym_reset_done(mgym_env *env, const uint8_t *done, const uint8_t *truncated, float *obs_out);

/* Gym::step (cartpole.rs:251-348, mountain_car.rs:293-330, lunar_lander.rs:919-1167).
 * Any of obs_out / reward_out / done_out / trunc_out may be NULL (not written).  trunc_out: CartPole's 500-step rule (cartpole.rs:297);
 * MountainCar / LunarLander: 0 as in the reference unless mgym_config::max_episode_steps sets a limit. */
int mgym_step(mgym_env *env, const void *actions, float *obs_out, float *reward_out,
              uint8_t *done_out, uint8_t *trunc_out);

/* K consecutive Gym::step calls on every env in ONE launch (fused rollout).  Results are
 * identical to K calls of mgym_step with the same per-step action columns, including the
 * MGYM_FLAG_AUTO_RESET behaviour between steps and the truncated flags of mgym_config::max_episode_steps (MountainCar keeps the elapsed
 * count in registers across the K steps: one read and one write per launch); for CartPole/MountainCar the state stays in registers
 * across the K steps, so per-step HBM traffic is the action read and the reward/flag writes only.
 * actions: [K][n_envs]; reward_out/done_out/trunc_out: [K][n_envs] or NULL; obs_out: [K][obs_dim][n_envs] or NULL.
 * The fused kernels need n_envs a multiple of 4 and the buffers 16-byte aligned (flags 4-byte), and CartPole's, which addresses the [K][n_envs] word
 * buffers by 32-bit byte offsets, K * n_envs below 2^30 (1 Mi environments x 1023 steps, 2^27 x 7); a call outside these runs as K launches of the step
 * kernel — the same words.  The policy entry points below have no K-step form for the classic families: there such a call is MGYM_ERR_BAD_ARG (the
 * message names the entry point), nothing launched, the state, mgym_episode_count and the uniform call count untouched.
 * LunarLander: ONE persistent launch in which every environment advances as soon as IT is ready (free-flight environments stay in
 * registers from step to step, environments on the contact path travel through device queues in batches of their own kind, whatever step
 * index each is at) — a step of mgym_step ends with its slowest environment, K steps of mgym_rollout cost the mean one.  Per-environment
 * results are those of K mgym_step calls, word for word (the loop being fused: lunar_lander.rs:919-1167 called K times).  Which form runs is the
 * engine's choice by K and population (mgym_get_info: rollout, rollout_min_k, rollout_waves, rollout_helper_blocks): K >= 8 (K >= 12 below 163 840 envs) below 491 520 envs per handle
 * the persistent launch, otherwise K steps — and always K steps while the stream is being captured (mgym_graph_begin or an external capture): replays
 * of a captured persistent launch aborted inside the HIP runtime at the end of round 4, unexplained; the words are the same either way. */
int mgym_rollout(mgym_env *env, const void *actions, int32_t K, float *obs_out, float *reward_out,
                 uint8_t *done_out, uint8_t *trunc_out);

/* mgym_rollout under an on-device uniform random policy (SURVEY §8f-1 "policy hook": random), so a rollout needs no
 * [K][n] action table: env with global id g takes, at step t of this call, bit (t % 32) of word (g % 4) of
 * Philox4x32-10(key = policy_seed; counter = (g & ~3, number of earlier mgym_rollout_uniform calls on this handle,
 * 0x40000000 + t / 32)).  actions_out ([K][n_envs] uint32, may be NULL) receives the drawn actions.  n_envs and env_id_base must be
 * multiples of 4.  Reference loop it fuses: a trainer calling `action_space().sample()` then `step()` (cartpole.rs:251-348, 350-356;
 * mountain_car.rs:293-330).
 * MountainCar (Discrete(3)): same key and the first two counter words, fourth word 0x40000000 + t / 2; env g takes half (t % 2) (low half first)
 * of word (g % 4), h, and the action (3 h) >> 16 — every action within 2^-16 of probability 1/3.  MountainCarContinuous (Box(-1, 1)): fourth
 * word 0x40000000 + t, the top 24 bits u of word (g % 4) give the force u * 2^-23 - 1 (actions_out then holds f32 words).
 * LunarLander (Discrete(4)): same key and the first two counter words, fourth word 0x40000000 + t / 16; env g takes bits 2 (t % 16) and
 * 2 (t % 16) + 1 of word (g % 4): action (word >> (2 * (t % 16))) & 3.  t counts the steps of this call (a call of more than 240 steps runs as
 * several launches; t goes on across them).  Any n_envs; env_id_base a multiple of 4.  A handle that was never reset reports MGYM_ERR_NOT_RESET
 * (at the next mgym_sync), as mgym_step does.  Reference loop: lunar_lander.rs:919-1167 behind `action_space().sample()`. */
int mgym_rollout_uniform(mgym_env *env, uint64_t policy_seed, int32_t K, void *actions_out, float *obs_out,
                         float *reward_out, uint8_t *done_out, uint8_t *trunc_out);

/* mgym_rollout under an on-device LINEAR policy (SURVEY §8f-1 "policy hook"; §8f-4: the step either side of the path — policy inference consumes the
 * observation, produces the action): at every step env i takes action 1 if ((w[0]*x + w[1]*x_dot) + w[2]*theta) + w[3]*theta_dot + b > 0 (f32, evaluated in
 * exactly that order, nothing fused), else 0, on the observation it holds BEFORE the step — the loop a trainer's rollout collector runs
 * (`let a = policy(&obs); let info = env.step(a)`, cartpole.rs:251-348) without leaving the GPU's registers.  `policy` is a HOST pointer to obs_dim weights
 * followed by the bias (5 floats, read during the call).  actions_out ([K][n_envs] uint32, may be NULL) receives the actions taken.
 * MountainCar (Discrete(3), mountain_car.rs:293-330): `policy` = three rows of (w_position, w_velocity, bias), 9 floats; the action is the index of the largest
 * score s_j = (w_j0 * position + w_j1 * velocity) + b_j, the first of equal ones.  MountainCarContinuous: one row, 3 floats; the score itself is the force
 * (actions_out then holds f32 words).  n_envs a multiple of 4.
 * LunarLander (Discrete(4), lunar_lander.rs:919-1167): `policy` = four rows of (w_j0 .. w_j7, b_j), 36 floats; the score of row j is
 * s_j = (((((((w_j0*o0 + w_j1*o1) + w_j2*o2) + w_j3*o3) + w_j4*o4) + w_j5*o5) + w_j6*o6) + w_j7*o7) + b_j in f32, in exactly that order, nothing fused;
 * the action starts as 0 with best = s_0, and row j = 1..3 replaces it when s_j > best (strict): the first of equal scores wins, a NaN score never
 * replaces an earlier one, and a NaN s_0 gives action 0.  o is the observation the env holds before the step: at the first step of the call the handle's
 * current observation (mgym_observation), later the one the previous step returned (under MGYM_FLAG_AUTO_RESET, for an env that finished there, its
 * reset observation).  Any n_envs.  A handle that was never reset reports MGYM_ERR_NOT_RESET (at the next mgym_sync), as mgym_step does.  From
 * MGYM_LL_ROLLOUT_MIN_K steps up the call is one persistent launch (ll_roll.h) in which each environment's next action is decided where its observation
 * is produced; below that, above the launch's population limit, or while the stream is being captured it runs as K x (a policy kernel, mgym_step) —
 * the same words either way. */
int mgym_rollout_linear(mgym_env *env, const float *policy, int32_t K, void *actions_out, float *obs_out,
                        float *reward_out, uint8_t *done_out, uint8_t *trunc_out);

/* mgym_rollout under an on-device policy with ONE HIDDEN LAYER (the small MLP a trainer actually has: 4 / 2 / 8 inputs, up to 64 hidden units, ReLU or
 * tanh), evaluated where the observation already sits in registers — no [n][H] activation and no observation or action round trip through memory.
 * Symbols: D = obs_dim; A = n_actions for the discrete families (CartPole 2, MountainCar 3, LunarLander 4) and 1 for MountainCarContinuous;
 * H = hidden, 1 <= H <= 64.
 * `policy` is a HOST pointer, read during the call, to H (D + 1) + A (H + 1) floats in nn.Linear order: W1[H][D] row-major, b1[H], W2[A][H] row-major, b2[A].
 * At every step env i uses the observation o it holds BEFORE the step (as mgym_rollout_linear: at the first step of the call the handle's current
 * observation, later the one the previous step returned — under MGYM_FLAG_AUTO_RESET, for an env that finished there, its reset observation):
 *   hidden pre-activation  pre_j = b1[j], then for q = 0 .. D-1 ascending  pre_j = fmaf(W1[j][q], o[q], pre_j);
 *   hidden activation      MGYM_ACT_RELU: h_j = pre_j > 0.0f ? pre_j : 0.0f (NaN and -0 both give +0);  MGYM_ACT_TANH: h_j = tanhf(pre_j), glibc's, bit for bit
 *                          (mg_tanhf of csrc/mgym_math.h);  MGYM_ACT_TANH_FAST: h_j = mg_tanhf_fast(pre_j), the cheap tanh defined below;
 *   scores                 s_a = b2[a], then for j = 0 .. H-1 ascending  s_a = fmaf(W2[a][j], h_j, s_a);
 *   discrete action        the sequential strict argmax of mgym_rollout_linear's LunarLander form: start with action 0 and best = s_0; row a replaces it when
 *                          s_a > best; the first of equal scores wins, a NaN never replaces an earlier score, a NaN s_0 gives action 0;
 *   MountainCarContinuous  s_0 is the force, handed to the step as it is (actions_out then holds f32 words).
 * Each fmaf is ONE correctly rounded f32 fused multiply-add (C's fmaf); nothing else is fused and nothing is reassociated.  That is what a v_fma_f32 loop,
 * a packed-FMA loop, an f32 MFMA with the bias as its C input and glibc's fmaf on the host all compute, so the words do not depend on the form the engine runs.
 * Everything else is as mgym_rollout_linear: actions_out ([K][n_envs], may be NULL) receives the actions taken, the output shapes are the same, and the K
 * steps equal K mgym_step calls fed those actions, word for word, MGYM_FLAG_AUTO_RESET and mgym_config::max_episode_steps included.  CartPole and
 * MountainCar: n_envs a multiple of 4 and the buffers 16-byte aligned (CartPole: K * n_envs below 2^30), the state stays in registers across the K steps.
 * LunarLander: any n_envs; by default this entry point is K x (a policy kernel, mgym_step) at every K.  The persistent launch of mgym_rollout (ll_roll.h)
 * carries this policy too — each environment's next action decided where its observation is produced, ReLU and tanh alike, the same words — and runs it
 * under the conditions of mgym_rollout_linear (from MGYM_LL_ROLLOUT_MIN_K steps up, below the launch's population limit, not while the stream is being
 * captured) for an activation that has been measured faster there (none yet) and, with MGYM_LL_ROLLOUT_MLP=1 in the environment at mgym_create, for
 * both; mgym_get_info's rollout_persistent_launches tells which form ran.  MGYM_ACT_TANH_FAST is not among them: the persistent launch has no form for it,
 * so on LunarLander it always runs as K x (a policy kernel, mgym_step), MGYM_LL_ROLLOUT_MLP=1 included, and rollout_persistent_launches does not move.  The weights are copied during the call in both forms: consecutive calls on
 * one stream each use their own.  A handle that was never reset reports MGYM_ERR_NOT_RESET at the next mgym_sync.
 * Errors, reported before any launch with the argument named in mgym_last_error: NULL policy, hidden outside 1 .. 64, an unknown activation -> MGYM_ERR_BAD_ARG.
 * Under graph capture the weights are frozen into the captured launches, as the linear policy's are.
 *
 * MGYM_ACT_TANH_FAST = 3:  h_j = mg_tanhf_fast(pre_j), a tanh for collectors.  MGYM_ACT_TANH is glibc's tanhf to the bit and is nearly all of a launch's time; the
 * hidden units of a collector's policy need no such thing (the learner recomputes with its own tanh), only words that are defined here and that a host
 * reproduces.  All arithmetic is f32; every fmaf is one correctly rounded fused multiply-add; nothing else is fused and nothing is reassociated; the divide is
 * the IEEE-correct f32 divide.  Branch-free: about 30 VALU instructions, one divide.
 *
 *   x is a NaN: the result is a NaN (compared as a class)
 *   a  = |x|;  a = a < 10.0f ? a : 10.0f                 (an infinity gives 10)
 *   u  = -2.0f * a                                       exact
 *   n  = rintf(u * 0x1.715476p+0f)                       one f32 multiply, then round to nearest integer, ties to even: n in -29 .. 0
 *   r  = fmaf(n, -0x1.62e4p-1f, u)
 *   r  = fmaf(n, -0x1.7f7d1cp-20f, r)                    |r| <= ~0.347: u = n ln2 + r
 *   q  = 0x1.a01a02p-13f                                 1/5040
 *   q  = fmaf(q, r, 0x1.6c16c2p-10f)                     1/720
 *   q  = fmaf(q, r, 0x1.111112p-7f)                      1/120
 *   q  = fmaf(q, r, 0x1.555556p-5f)                      1/24
 *   q  = fmaf(q, r, 0x1.555556p-3f)                      1/6
 *   q  = fmaf(q, r, 0.5f)
 *   p  = fmaf(q, r * r, r)                               expm1(r), relative accuracy kept down to r = 0
 *   s  = the f32 with bits (127 + n) << 23               2^n, always a normal number
 *   em = fmaf(s, p, s - 1.0f)                            expm1(u) = 2^n expm1(r) + (2^n - 1); s - 1 is exact for n >= -24
 *   z  = (-em) / (em + 2.0f)                             tanh(a) = -expm1(-2a) / (expm1(-2a) + 2); the denominator lies in [1, 2]
 *   result = copysignf(z, x)                             odd by construction; +-0 give +-0
 *
 * Enumerated over all 2^31 non-negative patterns with glibc's fmaf (tests/test_tanh_fast_host.py) against float64 tanh: the largest error is 2.50 f32
 * spacings of the exact value and the largest absolute error 1.49e-7, both at x = 4.5050907 (pattern 0x409029b4); no result exceeds 1.0f, the results never
 * decrease as x grows, n stays within -29 .. 0, the first x with result 1.0f is 8.4910536 (0x4107db5b), an infinity gives 1.0f.  The device's words equal the host's
 * (tests/test_gpu_tanh_fast_probe.py).  The value 2 is not assigned: it stays the unknown activation it has always been (MGYM_ERR_BAD_ARG naming `activation` from
 * all three entry points), and a later activation does not take it either. */
enum { MGYM_ACT_RELU = 0, MGYM_ACT_TANH = 1, MGYM_ACT_TANH_FAST = 3 };
int mgym_rollout_mlp(mgym_env *env, const float *policy, int32_t hidden, int32_t activation, int32_t K,
                     void *actions_out, float *obs_out, float *reward_out, uint8_t *done_out, uint8_t *trunc_out);

/* mgym_rollout_mlp with the action DRAWN from the categorical (softmax) distribution over the scores instead of their argmax: what the collector of an
 * on-policy trainer (REINFORCE, A2C, PPO) runs.  Everything is as in mgym_rollout_mlp — the `policy` layout, hidden 1 .. 64, MGYM_ACT_RELU / MGYM_ACT_TANH /
 * MGYM_ACT_TANH_FAST, the scores s_a as fmaf chains from the bias on the observation held before the step, the output shapes, and the rule that the K steps equal K mgym_step calls
 * fed the actions in actions_out, word for word, MGYM_FLAG_AUTO_RESET and mgym_config::max_episode_steps included — except how a discrete action follows
 * from the scores.
 *
 * The draw.  All arithmetic is f32 with nothing fused.  A is the family's n_actions.
 *
 *   m   = s_0;  for a = 1 .. A-1:  if (s_a > m) m = s_a          (the running best of the existing argmax)
 *   e_a = expm1f(s_a - m) + 1.0f                                   glibc's expm1f, bit for bit (mg_expm1f)
 *   c_0 = e_0;  c_a = c_{a-1} + e_a                                ascending a
 *   w   = word (g % 4) of Philox4x32-10(key = policy_seed;
 *             counter = (lo32(g & ~3), hi32(g & ~3), policy_call, 0x50000000 + t))
 *   u   = (float)(w >> 8) * 2^-24                                  exact, in [0, 1)
 *   thr = u * c_{A-1}                                              one multiply
 *   action = the first a in 0 .. A-2 with thr < c_a, else A-1
 *
 * g is the global environment id, env_id_base + i; t is the step index within this call.  The slot base 0x50000000 is this entry point's own: no draw of
 * the uniform policy (0x40000000 + ...) can coincide with it.
 *  - The draw is a pure function of (policy_seed, policy_call, g, t) and the scores.
 *  - It does not depend on how a population is sharded over handles.
 *  - The handle keeps no count for it, and the count of mgym_rollout_uniform calls is not touched: a caller passes a new policy_call (or seed) for each call
 *    that is to draw afresh.  The same (seed, call) on the same state draws the same actions again.
 *  - An action whose score lies about 17 or more below the best has weight 0 or 2^-24: probabilities are resolved to 2^-24.
 *  - A temperature is the caller dividing W2 and b2 by it beforehand.
 *  - Non-finite scores give a defined but meaningless action; a NaN makes every comparison false, hence A-1.  This is specified only so that every form
 *    of the code agrees (NaNs compare as a class: the weight of the best action is computed as (m - m) + 1.0f, the same word as the text's for a finite m).
 * No log-probabilities are returned from inside the rollout; mgym_logprob_mlp computes them, in this arithmetic, in a pass of its own over obs_out and actions_out.
 *
 * CartPole (A = 2), MountainCar (A = 3): inside the fused rollout kernels, one Philox evaluation per lane per step serving the lane's four environments;
 * the conditions of mgym_rollout_mlp (n_envs a multiple of 4, 16-byte aligned buffers, CartPole K * n_envs below 2^30) plus env_id_base a multiple of 4.
 * LunarLander (A = 4): any n_envs, env_id_base a multiple of 4; always K x (a sampling policy kernel, mgym_step) — the persistent launch does not carry this
 * source, MGYM_LL_ROLLOUT_MLP changes nothing for this entry point and rollout_persistent_launches does not move.
 * MountainCarContinuous, Pendulum: MGYM_ERR_BAD_ARG — these have no discrete actions; their drawn form is mgym_rollout_mlp_gauss below.
 * Errors are those of mgym_rollout_mlp, each message starting with "mgym_rollout_mlp_sample:".
 * Under graph capture the weights, the seed and the call word are frozen into the captured launches: a replay draws the same u again (on the state it
 * finds), so a loop that replays one graph does not explore — capture one graph per call word, or call eagerly. */
int mgym_rollout_mlp_sample(mgym_env *env, const float *policy, int32_t hidden, int32_t activation, uint64_t policy_seed, uint32_t policy_call,
                            int32_t K, void *actions_out, float *obs_out, float *reward_out, uint8_t *done_out, uint8_t *trunc_out);

/* mgym_rollout_mlp for the two CONTINUOUS families with the action DRAWN from a diagonal Gaussian around the score: a = mu + sigma * z, sigma a
 * state-independent standard deviation passed by the caller (the usual continuous PPO / A2C parameterisation; a second output row for a state-dependent
 * sigma is not offered).  As in mgym_rollout_mlp with D = 2 (MountainCarContinuous) or 3 (Pendulum) and A = 1: the `policy` layout, hidden 1 .. 64,
 * MGYM_ACT_RELU / MGYM_ACT_TANH / MGYM_ACT_TANH_FAST, the fmaf chain from the bias on the observation held before the step, the output shapes, the conditions of the fused form
 * (n_envs a multiple of 4, 16-byte aligned buffers), and the rule that the K steps equal K mgym_step calls fed the actions in actions_out, word for word,
 * MGYM_FLAG_AUTO_RESET and mgym_config::max_episode_steps included.
 *
 * The action.  mu is the one score s_0.  a = mu + sigma * z: one f32 multiply, then one f32 add, nothing fused.  actions_out receives a BEFORE any clamp;
 * the step clamps as it does for any action.  The learner needs the unclamped word for its log-probability and recovers z as (a - mu) / sigma in its own
 * forward pass over obs_out and actions_out; as with mgym_rollout_mlp_sample no log-probabilities are returned (mgym_logprob_mlp).  sigma == 0 gives a = mu, the words of
 * mgym_rollout_mlp (a -0 mu becomes +0: equal as a value).  A NaN mu gives a NaN action and the step's sticky MGYM_ERR_INVALID_ACTION.
 *
 * The draw of z.  A pure function of (policy_seed, policy_call, g, t), g = env_id_base + i the global environment id and t the step index within this call:
 * independent of how a population is sharded over handles, and the handle keeps no count for it (the count of mgym_rollout_uniform calls is not touched) —
 * pass a new policy_call (or seed) for each call that is to draw afresh; the same (seed, call) on the same state draws the same actions again.  One Philox
 * evaluation serves four consecutive ids:
 *
 *   (w0, w1, w2, w3) = Philox4x32-10(key = policy_seed; counter = (lo32(g & ~3), hi32(g & ~3), policy_call, 0x60000000 + t))
 *
 * 0x60000000 is this entry point's own slot base (csrc/philox.h), disjoint from the uniform policy's 0x40000000 + ... and the categorical draw's
 * 0x50000000 + ....  Environments with g % 4 in {0, 1} share the pair (wa, wb) = (w0, w1), those with g % 4 in {2, 3} the pair (w2, w3).  One Box-Muller
 * transform per pair gives two independent normals: the even member of the pair takes the cosine branch, the odd member the sine branch.
 *
 *   k1 = wa >> 8;  k2 = wb >> 8                        24 bits each
 *   n  = 2 * k1 + 1                                    odd, 1 .. 2^25 - 1;  u1 = n * 2^-25 lies in (0, 1), never 0 or 1
 *   L  = mg_log_u25(n)                                 f64, ln(u1): defined below
 *   q  = (float)(-2.0 * L)                             one f64 multiply, one rounding to f32
 *   r  = sqrtf(q)                                      the correctly rounded f32 square root
 *   phi = ((float)k2 * 2^-24f) * 6.28318548f           the first product is exact, one f32 rounding; phi in [0, 2 pi)
 *   s, c = sinf(phi), cosf(phi)                        glibc's, bit for bit (mg_sinf / mg_cosf of csrc/mgym_math.h, any of its forms: all are word-equal)
 *   z_even = r * c;   z_odd = r * s                    f32
 *
 * |z| <= sqrt(50 ln 2) = 5.88705 (k1 = 0), and the tails are resolved to 2^-25.
 *
 * mg_log_u25(n), all f64, every operation individually rounded (no fused multiply-add), so that a language without one restates it:
 *
 *   x = (double)n = m * 2^e with m in [1, 2) (read from the bits);  if (m > 0x1.6a09e667f3bcdp+0) { m = m * 0.5; e = e + 1; }
 *   s  = (m - 1.0) / (m + 1.0)                         IEEE f64 division
 *   s2 = s * s
 *   p  = 2/15;  then for c in (2/13, 2/11, 2/9, 2/7, 2/5, 2/3, 2):  p = p * s2 + c        (each constant the nearest double)
 *   p  = p * s
 *   L  = (double)(e - 25) * 0x1.62e42fefa39efp-1 + p
 *
 * This is ln m = 2 atanh(s) as the odd series up to s^15 with |s| <= 0.1716: over all 2^24 values of k1 it stays within 3.4e-14 relative of a float64
 * reference built from log / log1p (the first dropped term), there is no cancellation (when e = 25 the second term is all of L), and q > 0 always.  No
 * library logarithm is used anywhere: none is defined to the word.
 *
 * Families: MountainCarContinuous and Pendulum, inside their fused rollout kernels, one Philox evaluation per lane per step serving the lane's four
 * environments; env_id_base must be a multiple of 4.  Any other kind: MGYM_ERR_BAD_ARG ("... has discrete actions: use mgym_rollout_mlp_sample").
 * sigma must be finite and >= 0: a NaN, an infinity or a negative value is MGYM_ERR_BAD_ARG naming sigma, before any launch.  The other errors are those
 * of mgym_rollout_mlp, each message starting with "mgym_rollout_mlp_gauss:".
 * Under graph capture the weights, sigma, the seed and the call word are frozen into the captured launch: a replay draws the same z again (on the state it
 * finds) — capture one graph per call word, or call eagerly. */
int mgym_rollout_mlp_gauss(mgym_env *env, const float *policy, int32_t hidden, int32_t activation, float sigma, uint64_t policy_seed,
                           uint32_t policy_call, int32_t K, void *actions_out, float *obs_out, float *reward_out, uint8_t *done_out, uint8_t *trunc_out);

/* K fused steps under a policy with TWO hidden layers: Linear(D, H1) - act - Linear(H1, H2) - act - Linear(H2, A), the default network of the common PPO / A2C
 * code bases, so that a collector runs the network its learner trains.  `policy` is a HOST pointer, read during the call, in nn.Linear order:
 *   W1[H1][D], b1[H1], W2[H2][H1], b2[H2], W3[A][H2], b3[A]          1 <= H1 = hidden1 <= 64, 1 <= H2 = hidden2 <= 64; D and A per family as in mgym_rollout_mlp.
 * The words — o is the observation the environment holds before the step, every link one correctly rounded f32 fmaf, nothing else fused, nothing
 * reassociated, and each chain over exactly its D, H1 or H2 terms (no chain is padded: fmaf(+0, +0, -0) is +0, and the sign of a zero reaches the action):
 *   pre1_j = b1[j];  q = 0 .. D-1  ascending: pre1_j = fmaf(W1[j][q], o[q], pre1_j);   h1_j = act(pre1_j)
 *   pre2_k = b2[k];  j = 0 .. H1-1 ascending: pre2_k = fmaf(W2[k][j], h1_j, pre2_k);   h2_k = act(pre2_k)
 *   s_a    = b3[a];  k = 0 .. H2-1 ascending: s_a    = fmaf(W3[a][k], h2_k, s_a)
 * (modurl_gym_amd/csrc/mlp2_policy.h is this text as the kernels and a g++ build compile it.)
 * activation: the one hidden activation of both layers, MGYM_ACT_RELU or MGYM_ACT_TANH_FAST with their definitions above.  MGYM_ACT_TANH is refused
 * (MGYM_ERR_BAD_ARG naming activation): the exact tanh already makes the one-layer call slower than a torch loop at 64 units, and two layers double that.
 * head: what becomes of the scores, word for word what the one-layer entry points do with theirs —
 *   MGYM_HEAD_GREEDY  every family: the strict sequential argmax (discrete families), s_0 itself (MountainCarContinuous, Pendulum), as mgym_rollout_mlp
 *   MGYM_HEAD_SAMPLE  the discrete families: the categorical draw of mgym_rollout_mlp_sample — same text, same slot base 0x50000000, same key
 *                     (policy_seed, policy_call, global env id, t)
 *   MGYM_HEAD_GAUSS   MountainCarContinuous, Pendulum: mu + sigma * z of mgym_rollout_mlp_gauss — same text, slot base 0x60000000
 * sigma, policy_seed and policy_call are ignored by the heads that do not use them.
 * Everything else is as mgym_rollout_mlp: the K steps equal K mgym_step calls fed actions_out, word for word, MGYM_FLAG_AUTO_RESET and max_episode_steps
 * included; the output shapes; the conditions of the classic families' fused form (n_envs a multiple of 4, 16-byte alignment, CartPole's K * n_envs bound);
 * env_id_base a multiple of 4 for a drawing head; mgym_set_final_obs_out is honoured, its K > steps_cap refusal too.  The classic families decide inside
 * their fused rollout kernels; LunarLander runs K x (policy kernel, mgym_step) for any n_envs and never its persistent launch.
 * The weights do not fit a kernel argument (up to 20 KB): each handle owns a device buffer for them, allocated at mgym_create, and the call fills it on the
 * handle's stream ahead of its launches by small kernels that take the weights in slices as arguments.  So nothing is allocated in the call, consecutive
 * calls on one stream each find their own weights, and under graph capture the weights, sigma, the seed and the call word are frozen into the captured
 * launches.
 * Errors, all MGYM_ERR_BAD_ARG before any launch with the state untouched, each message starting with "mgym_rollout_mlp2:": a NULL policy; hidden1 or hidden2
 * outside 1 .. 64 (naming which); activation (MGYM_ACT_TANH as above; 2 and any other value are unknown); an unknown head; MGYM_HEAD_SAMPLE on a continuous
 * family or MGYM_HEAD_GAUSS on a discrete one; under MGYM_HEAD_GAUSS a sigma that is NaN, infinite or negative; env_id_base % 4 != 0 under a drawing head. */
enum { MGYM_HEAD_GREEDY = 0, MGYM_HEAD_SAMPLE = 1, MGYM_HEAD_GAUSS = 2 };
int mgym_rollout_mlp2(mgym_env *env, const float *policy, int32_t hidden1, int32_t hidden2, int32_t activation, int32_t head,
                      float sigma, uint64_t policy_seed, uint32_t policy_call, int32_t K,
                      void *actions_out, float *obs_out, float *reward_out, uint8_t *done_out, uint8_t *trunc_out);

/* The final observations of auto-reset episodes (gymnasium's final_obs / final_observation): what a learner bootstraps a truncated episode from.
 * final_obs_out is a DEVICE pointer to [steps_cap][obs_dim][n_envs] floats — the layout of a rollout's obs_out — and stays set on the handle until it
 * is replaced.  NULL turns the channel off and is always accepted (steps_cap is ignored then).
 * While it is set, every call that steps writes to it — mgym_step, mgym_rollout (its K x step form too), mgym_rollout_uniform, _linear, _mlp, _mlp_sample,
 * _mlp_gauss, _mlp2 — and nothing else does (mgym_reset* never).  Take env i at step t of the call (mgym_step: t = 0): if that step returns done | truncated, the
 * call writes the obs_dim words final_obs_out[(t * obs_dim + k) * n_envs + i], k = 0 .. obs_dim - 1: the observation this step produced BEFORE the fused
 * reset — exactly the words obs_out would hold for that env-step on a handle without MGYM_FLAG_AUTO_RESET.  No other word of the buffer is written
 * (read it where done | truncated is set), and obs_out and every other output are unchanged word for word.  The stores are sparse 4-byte ones made by
 * the lane that owns the environment: any n_envs, 4-byte alignment.  A handle with the channel off launches exactly the kernels it always did.
 * MGYM_ERR_BAD_ARG, the message naming the argument: a non-NULL final_obs_out on a handle without MGYM_FLAG_AUTO_RESET (obs_out already holds the final
 * observation there); steps_cap < 1; a pointer that is not 4-byte aligned; MGYM_LUNARLANDER (not offered yet: its resets run through shadow records,
 * staged copies and the persistent rollout's queues).  A stepping call with K > steps_cap: MGYM_ERR_BAD_ARG naming the entry point, before any launch,
 * the state untouched.
 * Graph capture: the pointer is frozen into captured launches like every output pointer; setting it later does not invalidate earlier graphs, and
 * each captured call indexes t from 0.
 * Not a compacted list of finished env-steps: that would be smaller, but needs atomics and has a run-dependent order; the dense buffer is
 * deterministic and can be checked word for word against a handle without auto-reset. */
int mgym_set_final_obs_out(mgym_env *env, float *final_obs_out, int32_t steps_cap);

/* Generalised advantage estimation over the outputs of a K-step rollout: one launch, a reverse scan per environment.  A pure function of its arguments: the
 * handle supplies only the device, the stream and n_envs; every kind is accepted and no state of the handle is read or written.  All pointers are DEVICE
 * pointers; nothing is allocated or synchronised, so the call is capturable (mgym_graph_begin or an external capture).
 *   reward, done, trunc   [K][n_envs], the rollout's outputs; done / trunc may be NULL = all 0
 *   value                 [K][n_envs]: V of the observation each env held BEFORE step t (the one the policy acted on)
 *   last_value            [n_envs]: V of the observation held after the last step (obs_out[K-1])
 *   final_value           [K][n_envs] or NULL: V(final observation, mgym_set_final_obs_out), used ONLY where trunc != 0 && done == 0
 *   adv_out, ret_out      [K][n_envs] each; either may be NULL, not both
 * The words, for environment i.  All arithmetic is f32; fmaf is one correctly rounded fused multiply-add; nothing else is fused or reassociated.
 *
 *   gl = gamma * lambda                       one f32 multiply, on the host
 *   carry = +0.0f;  nxt = last_value[i]
 *   for t = K-1 down to 0:
 *       d = done[t][i] != 0;  u = trunc[t][i] != 0;  fin = d | u
 *       nv    = fin ? (d ? +0.0f : (final_value ? final_value[t][i] : +0.0f)) : nxt
 *       c     = fin ? +0.0f : carry
 *       delta = fmaf(gamma, nv, reward[t][i]) - value[t][i]
 *       adv   = fmaf(gl, c, delta)
 *       adv_out[t][i] = adv;   ret_out[t][i] = adv + value[t][i]
 *       carry = adv;  nxt = value[t][i]
 *
 * (modurl_gym_amd/csrc/gae.h is this text as the kernels and a g++ build compile it.)
 *  - done wins over trunc: a terminated episode has no future, also when both flags are set.
 *  - The three ?: are selections, not multiplications by a mask.  A word that is not selected cannot reach any result, whatever it holds: final_value where
 *    the episode did not end by truncation alone (the final-observation buffer holds whatever the caller filled it with there), nxt and carry across an
 *    episode end.  A NaN there leaves every output finite.  (The kernels load final_value only where it is selected.)
 *  - final_value == NULL treats truncation as termination (LunarLander has no other form yet).
 *  - lambda = 1 with value = 0 gives discounted returns-to-go; lambda = 0 gives the one-step TD error.
 * Four environments per lane and 16-byte accesses when n_envs is a multiple of 4, the float pointers are 16-byte aligned and the flag pointers 4-byte
 * aligned; otherwise one environment per lane.  The words are the same.
 * MGYM_ERR_BAD_ARG before any launch, the message naming the argument: K < 1; a NULL reward, value or last_value; adv_out and ret_out both NULL; gamma or
 * lambda NaN or outside [0, 1]; a float pointer that is not 4-byte aligned; an output pointer equal to an input pointer (overlap beyond pointer equality is
 * the caller's error and undefined).  n_envs == 0 returns MGYM_OK without a launch. */
int mgym_gae(mgym_env *env, int32_t K, const float *reward, const uint8_t *done, const uint8_t *trunc, const float *value, const float *last_value,
             const float *final_value, float gamma, float lambda, float *adv_out, float *ret_out);

/* A critic's values over the buffers of a K-step rollout: exactly the three inputs of mgym_gae that nothing else in the engine produces.  A pure function
 * of its arguments like mgym_gae: the handle supplies the device, the stream, n_envs and D = obs_dim of its kind (2, 3, 4, 6 or 8); every kind is accepted, no
 * state of the handle is read or written (a LunarLander handle that was never reset is accepted), nothing is allocated or synchronised, the call is capturable.
 * critic is a HOST pointer, read during the call, in nn.Linear order; 1 <= H1 = hidden1 <= 64:
 *   hidden2 == 0   one hidden layer:   W1[H1][D], b1[H1], W2[1][H1], b2[1]                                   the words of mgym_rollout_mlp with A = 1
 *   hidden2 >= 1   two hidden layers:  W1[H1][D], b1[H1], W2[H2][H1], b2[H2], W3[1][H2], b3[1], H2 <= 64     the words of mgym_rollout_mlp2 with A = 1
 * V(o) is that text's one score s_0 for the observation o: every link one correctly rounded f32 fmaf, in ascending order from the bias, nothing else fused,
 * no chain padded (the words of mlp_scores<D, 1, ACT, N> of modurl_gym_amd/csrc/mlp_policy.h and mlp2_policy.h; this entry point adds no arithmetic definition).
 * activation: MGYM_ACT_RELU, MGYM_ACT_TANH or MGYM_ACT_TANH_FAST with one hidden layer; with two MGYM_ACT_TANH is refused, as in mgym_rollout_mlp2.
 * All other pointers are DEVICE pointers.
 *   obs_first         [D][n_envs]     dense: the observation held before step 0 of the rollout
 *   obs               [K][D][n_envs]  the rollout's obs_out
 *   final_obs         [K][D][n_envs]  the buffer of mgym_set_final_obs_out, or NULL
 *   done, trunc       [K][n_envs]     the rollout's flags; they select the final values and are ignored when final_obs is NULL; done may be NULL = all 0
 *   value_out         [K][n_envs]     value_out[0][i] = V(obs_first[:, i]);  value_out[t][i] = V(obs[t-1][:, i]) for t = 1 .. K-1
 *   last_value_out    [n_envs]        last_value_out[i] = V(obs[K-1][:, i])
 *   final_value_out   [K][n_envs]     final_value_out[t][i] = V(final_obs[t][:, i]), written ONLY where trunc[t][i] != 0 && (done == NULL || done[t][i] == 0)
 * (modurl_gym_amd/csrc/value.h is this mapping as the kernels and a g++ build compile it.)
 *  - value_out and last_value_out are mgym_gae's value and last_value: under MGYM_FLAG_AUTO_RESET obs holds the reset observation where an episode ended,
 *    which is the observation the policy acts on next, so it is the right input.
 *  - The set where final_value_out is written is the set mgym_gae selects.  No other word of final_value_out is written, and no word of final_obs outside
 *    that set is read into any result: a NaN there reaches nothing (the kernels load final_obs only where it is selected).
 *  - final_obs, final_value_out and trunc are either all non-NULL or the first two are NULL (LunarLander callers pass them NULL: it has no final-observation
 *    channel yet).
 * The one-layer critic travels by value as a kernel argument.  The two-layer critic goes through a device pack the handle owns from mgym_create — a second
 * one, not the actor's of mgym_rollout_mlp2 — which the call fills on the stream ahead of its launches as mgym_rollout_mlp2 does: consecutive calls on one
 * stream each find their own weights, a captured graph that holds a mgym_rollout_mlp2 and a mgym_value_mlp replays each with its own, and under capture the
 * weights are frozen.
 * The dense values: four environments per lane and 16-byte accesses when n_envs is a multiple of 4 and below 2^30 and the float pointers are 16-byte aligned,
 * otherwise one environment per lane; the [K][D][n_envs] buffers may exceed 4 GiB.  The final values: a second launch whose cost follows the number of
 * selected env-steps (the flag rows are walked, the selected (t, i) compacted per wave, and only those evaluated); no atomics, no run-dependent order.
 * The words are the same in every form.
 * MGYM_ERR_BAD_ARG before any launch, the message starting "mgym_value_mlp:" and naming the argument: K < 1; a NULL critic, obs_first, obs, value_out or
 * last_value_out; hidden1 outside 1 .. 64; hidden2 outside 0 .. 64; an unknown activation (2 is unknown), or MGYM_ACT_TANH with hidden2 >= 1; one of final_obs
 * and final_value_out without the other, or either of them without trunc; a float pointer that is not 4-byte aligned; an output pointer equal to an input
 * pointer or to another output (overlap beyond pointer equality is the caller's error and undefined).  n_envs == 0 returns MGYM_OK after the checks
 * without a launch. */
int mgym_value_mlp(mgym_env *env, const float *critic, int32_t hidden1, int32_t hidden2, int32_t activation, int32_t K,
                   const float *obs_first, const float *obs, const float *final_obs,
                   const uint8_t *done, const uint8_t *trunc,
                   float *value_out, float *last_value_out, float *final_value_out);

/* The actor's log-probabilities over the buffers of a K-step rollout: log pi(a | o) of every env-step, under the distribution the rollout entry points draw
 * from — PPO's "old" log-probability, in the arithmetic of the behaviour policy itself (a torch forward pass of the same weights differs from it by rounding
 * and by the tanh).  A pure function of its arguments like mgym_gae and mgym_value_mlp: the handle supplies the device, the stream, n_envs and the family's
 * (D, A) — CartPole (4, 2), MountainCar (2, 3), MountainCarContinuous (2, 1), Pendulum (3, 1), Acrobot (6, 3), LunarLander (8, 4); every kind is accepted, no
 * state of the handle is read or written (a LunarLander handle that was never reset is accepted), nothing is allocated or synchronised, the call is capturable.
 * policy is a HOST pointer, read during the call; 1 <= H1 = hidden1 <= 64:
 *   hidden2 == 0   the layout and the scores of mgym_rollout_mlp:   W1[H1][D], b1[H1], W2[A][H1], b2[A]
 *   hidden2 >= 1   the layout and the scores of mgym_rollout_mlp2:  W1[H1][D], b1[H1], W2[H2][H1], b2[H2], W3[A][H2], b3[A], H2 <= 64
 * activation: MGYM_ACT_RELU, MGYM_ACT_TANH or MGYM_ACT_TANH_FAST with one hidden layer; with two MGYM_ACT_TANH is refused, as in mgym_rollout_mlp2.
 * All other pointers are DEVICE pointers.
 *   obs_first   [D][n_envs]      the observation held before step 0 of the rollout
 *   obs         [K][D][n_envs]   the rollout's obs_out
 *   actions     [K][n_envs]      the rollout's actions_out: uint32 words for the discrete families, f32 words for the continuous ones (the word BEFORE the step's clamp)
 *   logp_out    [K][n_envs]      logp_out[t][i] = log pi(actions[t][i] | o),  o = t == 0 ? obs_first[:, i] : obs[t-1][:, i]
 * o is the observation the policy acted on (the row mgym_value_mlp's value_out[t] reads); under MGYM_FLAG_AUTO_RESET, where an episode ended, it is the reset
 * observation.  The scores s_a of o are those of the rollout entry points, unchanged.  All arithmetic below is f32 unless marked f64; nothing is fused beyond
 * the chains' fmaf, nothing reassociated.
 *
 * mg_log_pos(x), an f64 function of a positive normal f32 x — the series of mg_log_u25 above, every operation individually rounded:
 *   (double)x = m * 2^e with m in [1, 2) (read from the bits);  if (m > 0x1.6a09e667f3bcdp+0) { m = m * 0.5; e = e + 1; }
 *   s  = (m - 1.0) / (m + 1.0);   s2 = s * s
 *   p  = 2/15;  then for c in (2/13, 2/11, 2/9, 2/7, 2/5, 2/3, 2):  p = p * s2 + c;      p = p * s
 *   L  = (double)e * 0x1.62e42fefa39efp-1 + p
 *
 * head = MGYM_HEAD_SAMPLE (the discrete families), the distribution of mgym_rollout_mlp_sample:
 *   m, e_a, c_{A-1}   exactly as in "The draw" there
 *   lse  = (float)mg_log_pos(c_{A-1})
 *   d    = s_act - m                       ((m - m) for the best action, as the draw has it)
 *   logp = d - lse
 *   the quiet NaN 0x7fc00000 instead if !(c_{A-1} >= 1.0f && c_{A-1} <= (float)A) — which covers non-finite scores — or if the action word is >= A.  No
 *   error is raised for such a word: this is a function of buffers, not a step.
 * head = MGYM_HEAD_GAUSS (MountainCarContinuous, Pendulum), the distribution of mgym_rollout_mlp_gauss:
 *   mu = s_0;   z = (a - mu) / sigma       the IEEE f32 divide;      q = z * z;      logp = k - 0.5f * q
 *   k  = (float)(-(mg_log_pos(sigma) + 0.91893853320467274))         f64, once on the host
 *   sigma must be a finite, normal, positive f32: sigma == 0 has no density, unlike in the rollout call.  sigma is ignored under MGYM_HEAD_SAMPLE.
 * MGYM_HEAD_GREEDY is refused: a deterministic policy has no density.  (modurl_gym_amd/csrc/logprob.h is this text as the kernels and a g++ build compile it.)
 *  - Entropy is not returned: the learner's entropy bonus needs a gradient, which its own forward pass has.  Under the Gaussian head the entropy is the
 *    constant log sigma + 1.4189385.
 *  - Nothing is returned from inside the rollout kernels: this is a separate pass over their outputs, and they are unchanged.
 * The one-layer actor travels by value as a kernel argument.  The two-layer actor goes through a third device pack the handle owns from mgym_create — neither
 * the actor's of mgym_rollout_mlp2 nor the critic's of mgym_value_mlp — which the call fills on the stream ahead of its launch: consecutive calls on one stream
 * each find their own weights, a captured graph that holds a mgym_rollout_mlp2, a mgym_value_mlp and a mgym_logprob_mlp replays each with its own, and under
 * capture the weights and sigma are frozen.
 * One launch: four environments per lane and 16-byte accesses when n_envs is a multiple of 4 and below 2^30 and obs_first, obs, actions and logp_out are
 * 16-byte aligned, otherwise one environment per lane; the words are the same.
 * MGYM_ERR_BAD_ARG before any launch, the message starting "mgym_logprob_mlp:" and naming the argument: K < 1; a NULL policy, obs_first, obs, actions or
 * logp_out; hidden1 outside 1 .. 64; hidden2 outside 0 .. 64; an unknown activation (2 is unknown), or MGYM_ACT_TANH with hidden2 >= 1; MGYM_HEAD_GREEDY, an
 * unknown head, MGYM_HEAD_SAMPLE on a continuous family or MGYM_HEAD_GAUSS on a discrete one; under MGYM_HEAD_GAUSS a sigma that is zero, denormal, negative,
 * NaN or infinite; a device pointer that is not 4-byte aligned; logp_out equal to an input pointer (overlap beyond pointer equality is the caller's error and
 * undefined).  n_envs == 0 returns MGYM_OK after the checks without a launch. */
int mgym_logprob_mlp(mgym_env *env, const float *policy, int32_t hidden1, int32_t hidden2, int32_t activation, int32_t head, float sigma, int32_t K,
                     const float *obs_first, const float *obs, const void *actions, float *logp_out);

/* PPO's loss and the actor's gradient, and a critic's squared-error loss and gradient, over the buffers of a K-step rollout: the update a learner handed to a
 * torch forward pass (a [K n][H] activation written), a surrogate and autograd's backward pass (the activation read back).  One hidden layer, 1 <= H = hidden
 * <= 64; the six (D, A) of mgym_logprob_mlp; MGYM_HEAD_SAMPLE on the discrete families and MGYM_HEAD_GAUSS on the continuous ones; MGYM_ACT_RELU, MGYM_ACT_TANH
 * and MGYM_ACT_TANH_FAST.  Two hidden layers are the calls after these, mgym_ppo_grad_mlp2 and mgym_value_grad_mlp2 (dW2[H2][H1] is a tiled product over
 * the batch dimension, kernels of their own).  Out of scope: the optimizer step; advantage normalisation; flat-index minibatches; a clipped value loss; any
 * state of the handle.
 *
 * Purity.  As mgym_logprob_mlp: the handle supplies the device, the stream, n_envs and (D, A); every kind is accepted and no state of the handle is read or
 * written.  policy / critic is a HOST pointer in nn.Linear order, W1[H][D], b1[H], W2[A][H], b2[A] (A = 1 for the critic), read during the call and passed to the
 * kernels by value.  Every other pointer is a DEVICE pointer.  Nothing is allocated and nothing synchronised — the caller owns the workspace — so the calls are
 * capturable (the weights, sigma, clip and ent_coef are frozen under capture).
 *   obs_first [D][n_envs], obs [K][D][n_envs], actions [K][n_envs]     the rollout's buffers, as for mgym_logprob_mlp
 *   logp_old  [K][n_envs]     the output of mgym_logprob_mlp;     adv, ret  [K][n_envs]     the outputs of mgym_gae.  Every row keeps the stride n_envs.
 * Minibatch.  The call covers every step t in 0 .. K-1 of the environments env_first <= i < env_first + env_count: environments are independent, so contiguous
 * slices partition a batch, and the full range is one batch.  B = K * env_count.  No word of any input outside the range reaches any result — a NaN there is
 * harmless — and the kernels do not load those words.
 *   grad_out  mlp_policy_floats(D, A, H) + 1 = H (D + 1) + A (H + 1) + 1 floats: dW1[H][D], db1[H], dW2[A][H], db2[A] in nn.Linear order (an optimizer can view
 *             them as the parameters' .grad), then one word: dL / d log sigma under the Gaussian head, +0 under the sample head and for the critic
 *   stats_out 8 floats.  Actor: [0] the policy loss -mean(min(r adv, clamp(r) adv)) (without the entropy bonus), [1] the mean entropy, [2] the approximate KL
 *             mean(r - 1 - d), [3] the clipped fraction, [4] the mean ratio, [5] (float)B, [6] and [7] +0.  Critic: [0] the loss, [5] (float)B, the rest +0.
 *
 * Per env-step, f32 words; the chains keep the fmaf rule of mgym_rollout_mlp, nothing else is fused, nothing reassociated, every selection is a selection:
 *   s_a        exactly the scores of mgym_rollout_mlp on o = t == 0 ? obs_first[:, i] : obs[t-1][:, i]
 *   logp_new   exactly the word of mgym_logprob_mlp (logp_head of csrc/logprob.h) — with unchanged weights d is +0 and the ratio exactly 1
 *   d = logp_new - logp_old;     r = mg_expm1f(d) + 1.0f
 *   L = -mean(min(r adv, clamp(r, lo, hi) adv)) - ent_coef mean(entropy),     lo = 1.0f - clip and hi = 1.0f + clip computed on the host
 *   clipped = (adv > 0 && r > hi) || (adv < 0 && r < lo);     g = clipped ? +0 : (-adv) * r          a selection, not a mask multiply: at r == hi or r == lo the
 *             gradient passes, as torch's clamp and min pass it
 *   the statistics' terms:  rc = r < lo ? lo : (r > hi ? hi : r);  u = r * adv;  uc = rc * adv;  loss = -(uc < u ? uc : u);  kl = (r - 1.0f) - d
 * MGYM_HEAD_SAMPLE:  m, e_a, c_{A-1} exactly as in "The draw" of mgym_rollout_mlp_sample;  lse = (float)mg_log_pos(c_{A-1});  p_a = e_a / c_{A-1};
 *   lp_a = (s_a - m) - lse;     t = p_0 * lp_0, then a = 1 .. A-1: t = t + p_a * lp_a;     Hent = -t                      (the env-step's entropy)
 *   ds_a = g * ((a == act ? 1.0f : 0.0f) - p_a) + (ent_coef * p_a) * (lp_a + Hent)
 * MGYM_HEAD_GAUSS:  z = (a - mu) / sigma;     ds_0 = (g * z) / sigma;     the log-sigma word receives g * (z * z - 1.0f) per env-step and -ent_coef * B once, so
 *   after the division by B it is the mean of g (z z - 1) minus ent_coef.  The entropy is the constant (float)(mg_log_pos(sigma) + 1.4189385332046727).
 * Critic:  L = 1/2 mean((V - ret)^2);     e = V - ret;     ds_0 = e;     the loss term 0.5f * (e * e).
 * Backward pass, all heads, hidden unit j:  pre_j and h_j as mgym_rollout_mlp computes them;
 *   dh = W2[0][j] * ds_0, then a = 1 .. A-1: dh = dh + W2[a][j] * ds_a;     dpre = dh * act',  act' = (pre_j > 0 ? 1.0f : 0.0f) under ReLU, 1.0f - h_j * h_j of the
 *   h_j word under both tanh forms (tanh_fast is differentiated as the tanh it approximates)
 *   dW2[a][j] += ds_a * h_j;     db2[a] += ds_a;     dW1[j][q] += dpre * o_q;     db1[j] += dpre
 * Every sum is divided by B once, at the end.  (modurl_gym_amd/csrc/grad.h is this text as the kernels and a g++ build compile it.)
 *  - An env-step whose logp_new is the NaN word (an action word that is no action, scores without a finite softmax) makes the gradient NaN: the caller's error,
 *    not special-cased.
 * The sums over the B env-steps are the one part that is not word-defined: their order belongs to the kernels.  (a) No float atomics, no tickets, no
 * run-dependent order: two calls with the same arguments (workspace_bytes included) on the same device return identical words.  (b) The values are bounded
 * against float64 (tests/grad_ref.py: GRAD_BOUND times the word's mean absolute per-env-step term).  A lane adds its own env-steps' terms, a wave adds across its
 * lanes, each wave owns an f64 slab in LDS, each block stores one f64 slab of P + 8 sums to the workspace, and a second small launch adds the slabs in index
 * order in f64, scales by 1 / B, rounds to f32 and writes grad_out and stats_out.
 * Workspace.  mgym_grad_workspace_bytes(kind, hidden) gives min_bytes, one slab, and best_bytes, 1024 slabs (four blocks on each of the chip's 256 compute
 * units); the same sizes serve both calls.  A call uses min(1024, workspace_bytes / min_bytes) slabs, and its blocks stride over the tiles when there are more
 * tiles than slabs; no word at or beyond workspace_bytes is written.  Four environments per lane with 16-byte rows when n_envs, env_first and env_count are
 * multiples of 4, n_envs < 2^30 and obs_first, obs, actions, logp_old / ret and adv are 16-byte aligned; otherwise one environment per lane.
 * MGYM_ERR_BAD_ARG before any launch, the message starting with the entry point's name and naming the argument: K < 1; a NULL policy / critic, obs_first, obs,
 * actions, logp_old / ret, adv, workspace, grad_out or stats_out; hidden outside 1 .. 64; an unknown activation (2 is unknown); the head and sigma rules of
 * mgym_logprob_mlp; env_count == 0, or env_first + env_count > n_envs; clip NaN, negative or >= 1; ent_coef NaN or infinite; workspace_bytes below min_bytes;
 * workspace not 16-byte aligned; another device pointer not 4-byte aligned; grad_out, stats_out or workspace equal to an input or to each other.  n_envs == 0
 * returns MGYM_OK after the other checks without a launch (there is no range to refuse).  mgym_grad_workspace_bytes refuses an unknown kind, hidden outside
 * 1 .. 64 and a NULL output. */
int mgym_grad_workspace_bytes(int kind, int32_t hidden, size_t *min_bytes, size_t *best_bytes);

int mgym_ppo_grad_mlp(mgym_env *env, const float *policy, int32_t hidden, int32_t activation, int32_t head, float sigma,
                      int32_t K, uint64_t env_first, uint64_t env_count,
                      const float *obs_first, const float *obs, const void *actions, const float *logp_old, const float *adv,
                      float clip, float ent_coef, void *workspace, size_t workspace_bytes, float *grad_out, float *stats_out);

int mgym_value_grad_mlp(mgym_env *env, const float *critic, int32_t hidden, int32_t activation,
                        int32_t K, uint64_t env_first, uint64_t env_count,
                        const float *obs_first, const float *obs, const float *ret,
                        void *workspace, size_t workspace_bytes, float *grad_out, float *stats_out);

/* The same two calls for the net of mgym_rollout_mlp2, Linear(D, H1) - act - Linear(H1, H2) - act - Linear(H2, A): the update of the network a collector runs
 * with mgym_rollout_mlp2 and a learner evaluates with mgym_value_mlp / mgym_logprob_mlp at hidden2 >= 1.  Everything not named here is as in mgym_ppo_grad_mlp /
 * mgym_value_grad_mlp: purity and capturability; obs_first, obs, actions, logp_old, adv, ret; the env_first / env_count slice, no word outside it loaded;
 * clip, ent_coef and the stats_out layout; no float atomics, no tickets, a call repeats to the word; four environments per lane under the same conditions, else
 * one; the refusals, each message starting with the entry point's name.  The optimizer step, advantage normalisation, flat-index minibatches, a clipped value
 * loss and any state of the handle stay out of scope.
 *   policy / critic   a HOST pointer in the layout of mgym_rollout_mlp2: W1[H1][D], b1[H1], W2[H2][H1], b2[H2], W3[A][H2], b3[A] (A = 1 for the critic), read
 *             during the call; the kernels read the weights from device packs the handle owns from mgym_create (a fourth and a fifth: the actor's and the
 *             critic's under these calls), filled on the stream ahead of the launch — so a captured graph that holds a rollout, a value, a log-probability and
 *             both gradient calls replays each with its own weights
 *   1 <= hidden1, hidden2 <= 64; hidden2 == 0 is refused (the one-layer calls above).  MGYM_ACT_RELU or MGYM_ACT_TANH_FAST; MGYM_ACT_TANH is refused as in
 *             every two-layer entry point
 *   grad_out  P2 + 1 floats, P2 = mlp2_policy_floats(D, A, H1, H2) = H1 (D + 1) + H2 (H1 + 1) + A (H2 + 1): dW1, db1, dW2, db2, dW3, db3 in nn.Linear order,
 *             then the log-sigma word (+0 under the sample head and for the critic).  stats_out 8 floats.
 * Per env-step, f32 words, nothing fused beyond the named fmaf, nothing reassociated, every selection a selection:
 *   pre1_j, h1_j, pre2_k, h2_k, s_a     exactly mgym_rollout_mlp2's text (the chains of csrc/mlp2_policy.h, unpadded)
 *   logp_new, d, r, g, ds_a, the log-sigma term, the statistics' terms, the critic's e and ds_0     exactly mgym_ppo_grad_mlp's text applied to these s_a;
 *             logp_new is the word mgym_logprob_mlp returns at hidden2 >= 1, so with unchanged weights the ratio is exactly 1
 *   dh2_k   = W3[0][k] * ds_0;  a = 1 .. A-1: dh2_k = dh2_k + W3[a][k] * ds_a
 *   dpre2_k = dh2_k * act'(k)           act' = pre2_k > 0 ? 1.0f : 0.0f (ReLU), 1.0f - h2_k * h2_k (tanh_fast)
 *   dh1_j   = +0.0f;  k = 0 .. H2-1 ascending: dh1_j = fmaf(W2[k][j], dpre2_k, dh1_j)
 *   dpre1_j = dh1_j * act'(j)           the same rule on pre1_j / h1_j
 *   terms:  dW3[a][k] += ds_a * h2_k;  db3[a] += ds_a;  dW2[k][j] += dpre2_k * h1_j;  db2[k] += dpre2_k;  dW1[j][q] += dpre1_j * o_q;  db1[j] += dpre1_j
 * (modurl_gym_amd/csrc/grad2.h is this text as the kernels and a g++ build compile it.)  The SUMS over the B env-steps are not word-defined, and neither are the
 * products inside them: the kernels form them on the f32 matrix pipe (exact f32 products, an f32 accumulator over at most 128 env-steps of a wave) and add
 * everything beyond in f64; every sum is divided by B once at the end, in f64.  The values are bounded against float64 (tests/grad_ref.py: GRAD2_BOUND times
 * the word's mean absolute per-env-step term).
 * Workspace.  A slab is P2 + 8 f64 words.  mgym_grad_workspace_bytes2(kind, hidden1, hidden2) gives min_bytes, one slab, and best_bytes, 256 slabs: a block of
 * these kernels holds most of a compute unit's LDS, so one block is resident on each of the chip's 256 compute units and more slabs would only lengthen the last
 * sum.  The query uses the family's own A, so one size serves both calls; a workspace sized by mgym_grad_workspace_bytes for the same hidden1 is too small and
 * refused.  A call uses min(256, workspace_bytes / min_bytes) slabs; its blocks stride over the tiles when there are more tiles than slabs; no word at or beyond
 * workspace_bytes is written.  mgym_grad_workspace_bytes2 refuses an unknown kind, hidden1 or hidden2 outside 1 .. 64 and a NULL output. */
int mgym_grad_workspace_bytes2(int kind, int32_t hidden1, int32_t hidden2, size_t *min_bytes, size_t *best_bytes);

int mgym_ppo_grad_mlp2(mgym_env *env, const float *policy, int32_t hidden1, int32_t hidden2, int32_t activation, int32_t head, float sigma,
                       int32_t K, uint64_t env_first, uint64_t env_count,
                       const float *obs_first, const float *obs, const void *actions, const float *logp_old, const float *adv,
                       float clip, float ent_coef, void *workspace, size_t workspace_bytes, float *grad_out, float *stats_out);

int mgym_value_grad_mlp2(mgym_env *env, const float *critic, int32_t hidden1, int32_t hidden2, int32_t activation,
                         int32_t K, uint64_t env_first, uint64_t env_count,
                         const float *obs_first, const float *obs, const float *ret,
                         void *workspace, size_t workspace_bytes, float *grad_out, float *stats_out);

/* The return and length of every episode that ends inside a K-step rollout: one launch, a forward scan per environment whose carry the CALLER owns, so
 * that episodes span calls.  A pure function of its arguments like mgym_gae (every kind, no handle state, capturable); all pointers are DEVICE pointers.
 *   reward, done, trunc      [K][n_envs]; done / trunc may be NULL = all 0
 *   ep_return, ep_length     [n_envs], IN and OUT: the return and length so far of the episode each environment is in
 *   return_out, length_out   [K][n_envs] or NULL each: written ONLY where done | trunc
 *
 *   acc = ep_return[i];  len = ep_length[i]
 *   for t = 0 .. K-1 ascending:
 *       acc = acc + reward[t][i]     one f32 add;      len = len + 1   (u32)
 *       if (done[t][i] != 0 || trunc[t][i] != 0):
 *           return_out[t][i] = acc;  length_out[t][i] = len;  acc = +0.0f;  len = 0
 *   ep_return[i] = acc;  ep_length[i] = len
 *
 *  - No other word of return_out / length_out is written: dense, sparsely written buffers like the final-observation channel, read where done | trunc is
 *    set, for the reason given there (no atomics, no run-dependent order).
 *  - The reward of the step that ends an episode belongs to that episode, as in the engine.
 *  - Two calls of K1 and K2 steps leave the words of one call of K1 + K2 steps.
 *  - The caller zeroes the carry where it resets environments by hand.  No sum across environments is returned: the learner masks and reduces.
 * MGYM_ERR_BAD_ARG before any launch, the message naming the argument: K < 1; a NULL reward, ep_return or ep_length; a float or uint32 pointer that is not
 * 4-byte aligned.  n_envs == 0 returns MGYM_OK without a launch. */
int mgym_episode_returns(mgym_env *env, int32_t K, const float *reward, const uint8_t *done, const uint8_t *trunc, float *ep_return, uint32_t *ep_length,
                         float *return_out, uint32_t *length_out);

/* Number of env-steps of this handle that returned done or truncated since mgym_create (StepInfo.done / .truncated,
 * cartpole.rs:300-305): accumulated inside the step kernels by __ballot/popcount reductions of the done mask,
 * one fire-and-forget atomic per wave.  Synchronises the stream. */
int mgym_episode_count(mgym_env *env, uint64_t *finished);

/* Zero-copy view of the engine-owned current observation, SoA with column stride *col_stride
 * floats (for CartPole/MountainCar the state columns ARE the observation — `self.state.clone()`,
 * cartpole.rs:301).  Valid until the handle is destroyed; contents follow the stream order. */
int mgym_observation(mgym_env *env, const float **obs, uint64_t *col_stride);

/* Row-major copy of the current observation for consumers that want `[n_envs][obs_dim]` (one row per env,
 * the shape of the reference's per-env state tensor stacked over envs): out_aos[i * obs_dim + k]. */
int mgym_observation_aos(mgym_env *env, float *out_aos);

/* Test seam / checkpoint ≙ Testable::set_state (src/testing.rs:15-18).  blob = [state_cols][n_envs]
 * 4-byte words (integer columns as bit patterns); column meaning per kind in DESIGN.md.
 * LunarLander: the blob carries the bodies, legs, counters and the episode number, not the terrain — as in the reference,
 * where set_state moves the lander of an existing world (lunar_lander.rs Testable impl) — so the handle must have been reset
 * before a state is imported; an environment without a world keeps none and mgym_step reports MGYM_ERR_NOT_RESET for it.
 *
 * LIMITS of the CartPole counters (the engine keeps steps_since_reset, steps_beyond_terminated and the per-env
 * episode number in ONE 32-bit word per env, cartpole_step.h):
 *  - blob column 4, steps_since_reset, saturates at 1023 and column 5, steps_beyond_terminated, at Some(2): the
 *    reference only ever tests "steps >= 500" and None/Some (cartpole.rs:297, 319, 330), so no result depends on more;
 *    larger imported values are clamped.
 *  - blob column 6, the episode number (= resets of this env so far), is kept MODULO 2^20, on import too.  It is word 2
 *    of the Philox counter of the env's next reset draw, so after 1 048 576 resets of ONE env its initial states
 *    repeat from the first one (same seed, same env id).  With a uniform random policy (~22-step episodes) that is
 *    ~2.3e7 steps of that env — about four minutes at this engine's CartPole rate.  The reference draws from an RNG
 *    that never cycles in practice (cartpole.rs:240); a trainer that steps one handle past that horizon and needs
 *    fresh initial states should create the next handle with a new `seed`.  Nothing else depends on the wrap.
 *    MountainCar and LunarLander keep a full 32-bit episode counter. */
int mgym_get_state(mgym_env *env, void *blob);
int mgym_set_state(mgym_env *env, const void *blob);

/* The elapsed count of mgym_config::max_episode_steps, for checkpoints and tests: out / in are DEVICE arrays of n_envs uint32.  Both are
 * ordered on the handle's stream and capturable.
 *   LunarLander: the step counter of blob column 25 minus 1 (mgym_get_state / mgym_set_state go on carrying it; on import, plus 1);
 *   kept whether or not a limit is set.
 *   MountainCar(+Continuous), Pendulum: a counter of its own beside the 3-column blob; mgym_set_state sets it to 0, mgym_set_elapsed_steps
 *   overrides it, values above 65535 are clamped.  A handle WITHOUT a limit runs the kernels as they were, which do not touch the
 *   counter: it is 0 after a reset and is not advanced by steps.
 *   CartPole: MGYM_ERR_BAD_ARG (its counter is blob column 4). */
int mgym_get_elapsed_steps(mgym_env *env, uint32_t *out);
int mgym_set_elapsed_steps(mgym_env *env, const uint32_t *in);

/* Test seam ≙ Testable::reset_deterministic (cartpole.rs:437-442: reset() then state = 0;
 * mountain_car.rs:403-408: state = 0; lunar_lander.rs:1249-1442: flat terrain, lander at
 * (W/2, 0.8 H) falling at 1 m/s, deterministic_mode = true) applied to every env. obs_out may be NULL. */
int mgym_reset_deterministic(mgym_env *env, float *obs_out);

/* LunarLander: deterministic_mode (lunar_lander.rs:967-970) generalised — disp = [2][n_envs]
 * raw U(-1,1) draws used instead of the per-env generator; NULL restores the generator. */
int mgym_set_dispersion_override(mgym_env *env, const float *disp);

int mgym_get_spec(int kind, mgym_spec *spec);

/* Wait for the stream and return (then clear) the sticky device-side status. */
int mgym_sync(mgym_env *env);

/* Thread-local message for the last failing call on this thread. */
const char *mgym_last_error(void);

/* Describes how this handle runs, as NUL-terminated "key=value" lines written to buf (at most cap bytes, always terminated;
 * returns MGYM_ERR_BAD_ARG if cap is too small).  Keys every family reports: kind, n_envs, device, auto_reset, max_episode_steps,
 * GPU_MAX_HW_QUEUES (the HIP runtime knob as this process's environment held it when the handle was created, or "unset").
 * LunarLander adds its launch structure — contact_block, launch_order, staged_resets, the rollout's form (rollout, rollout_min_k, rollout_waves,
 * rollout_helper_blocks) and rollout_persistent_launches, the number of persistent rollout launches this handle has issued since mgym_create
 * (mgym_rollout, _linear, _uniform and _mlp alike, never _mlp_sample; a call of more than 240 steps is several launches; 0 for a call that ran as K x mgym_step: the
 * words are the same either way, this line tells which form ran) — and `concurrent_streams`: the
 * reference is single-threaded (lunar_lander.rs:240-249), this engine steps one population on up to three streams
 * (caller's stream, two helpers), and they only run side by side when the runtime put them on different hardware queues.
 * The call launches a ~50 us probe kernel on each of them at once and reports how many were seen running at the same
 * time (3 of 3 is the measured configuration; fewer: set GPU_MAX_HW_QUEUES=8 before the first HIP call of the
 * process).  Synchronises the stream. */
int mgym_get_info(mgym_env *env, char *buf, size_t cap);

/* Plain device-memory helpers for callers without their own HIP allocator (C/C++/ctypes). */
int mgym_malloc(int device, size_t bytes, void **out);
int mgym_free(int device, void *ptr);
int mgym_memcpy_h2d(int device, void *dst_dev, const void *src_host, size_t bytes);
int mgym_memcpy_d2h(int device, void *dst_host, const void *src_dev, size_t bytes);
int mgym_device_count(int *count);

/* Stream timing helpers (hipEvent on the env's stream) so harnesses can time launches
 * on the stream the kernels actually run on. */
int mgym_timer_start(mgym_env *env);
int mgym_timer_stop(mgym_env *env, float *elapsed_ms); /* synchronises */

/* Test seam: evaluates, on the device, the exhaustive bit-identity checks of the cheap CartPole instruction sequences
 * against the reference-form arithmetic (cartpole.rs:264-271 with IEEE divide and glibc-equal sin/cos); see
 * modurl_gym_amd/csrc/selftest.hip.  mismatches[5] = {CartPole sincos, x / total_mass, n / d, whole CartPole step, fused lock-step
 * sincos / cos of the LunarLander and MountainCar kernels}; all must be 0. */
int mgym_selftest_cartpole_math(int device, uint64_t *mismatches);

/* Test seam: the result bits of one entry point of modurl_gym_amd/csrc/mgym_math.h (the glibc-equal f32 sin / cos / tanh the
 * kernels use), evaluated on the device for the input bit patterns first .. first + count - 1 (first + count <= 2^32).
 * out is device memory of count words, 2 * count for the sincos forms (sin at out[i], cos at out[count + i]).  Runs on the
 * null stream and synchronises the device.  tests/test_gpu_math_exhaustive.py compares every pattern with the host's glibc. */
enum {
    MGYM_MATH_SINF = 0,      /* mg_sinf */
    MGYM_MATH_COSF = 1,      /* mg_cosf */
    MGYM_MATH_SINCOSF = 2,   /* mg_sincosf */
    MGYM_MATH_SINCOSF_U = 3, /* mg_sincosf_u (LunarLander's lock-step form) */
    MGYM_MATH_COSF_U = 4,    /* mg_cosf_u (MountainCar's lock-step form) */
    MGYM_MATH_TANHF = 5      /* mg_tanhf */
};
int mgym_math_probe(int device, int fn, uint32_t first, uint64_t count, uint32_t *out);

/* Test seam: the result bits of the hidden activation of mgym_rollout_mlp (mlp_activate of modurl_gym_amd/csrc/mlp_policy.h) evaluated on the device for the
 * input bit patterns first .. first + count - 1 (first + count <= 2^32); out is device memory of count words.  activation is MGYM_ACT_RELU, MGYM_ACT_TANH or
 * MGYM_ACT_TANH_FAST; anything else, a NULL out, an empty or out-of-range span -> MGYM_ERR_BAD_ARG.  Runs on the null stream and synchronises the device.
 * A seam of its own: mgym_math_probe keeps the entry points of mgym_math.h that follow glibc.  tests/test_gpu_tanh_fast_probe.py compares with the
 * host-compiled header. */
int mgym_act_probe(int device, int activation, uint32_t first, uint64_t count, uint32_t *out);

/* Test seam: the draw of mgym_rollout_mlp_sample (mlp_sample of modurl_gym_amd/csrc/mlp_policy.h) evaluated on the device, one case per lane.
 * n_actions = A is 2, 3 or 4; scores is [A][count] floats, words [count] Philox words w, actions_out [count], cum_out [A][count] (c_0 .. c_{A-1}) or NULL;
 * all device memory; count at most 2^31.  Runs on the null stream and synchronises the device.  tests/test_gpu_sample_probe.py compares with the
 * restatement of the text above. */
int mgym_sample_probe(int device, int32_t n_actions, uint64_t count, const float *scores, const uint32_t *words, uint32_t *actions_out, float *cum_out);

/* Test seam: the Box-Muller pair of mgym_rollout_mlp_gauss (mlp_gauss_pair of modurl_gym_amd/csrc/mlp_policy.h) evaluated on the device, one pair of Philox
 * words (wa, wb) per lane: z_even_out and z_odd_out [count], and q_out [count] (q = -2 ln(u1) as an f32) or NULL; all device memory; count at most 2^31.
 * Runs on the null stream and synchronises the device.  tests/test_gpu_gauss_probe.py compares with the host-compiled header. */
int mgym_gauss_probe(int device, uint64_t count, const uint32_t *wa, const uint32_t *wb, float *z_even_out, float *z_odd_out, float *q_out);

/* Test seam: LunarLander's collision-geometry primitives (modurl_gym_amd/csrc/ll_b2.h) evaluated on the device as pure functions,
 * one case per lane.  in and out are device memory, columns [cols][count] of 32-bit words; integer fields are bit patterns.  The
 * ground edge v1-v2 is in the world frame, pi selects the polygon (0 lander hexagon, 1 leg box).
 *   SHAPES    in ignored (may be NULL), count must be 1.  out, 30 columns per polygon (pi 0, then pi 1): vertex count, 6 vertices
 *             x,y, 6 normals x,y (unused slots 0), mass, invMass, invI, localCenter x,y - as the kernels' staged tables hold them.
 *   DISTANCE  in: v1.x v1.y v2.x v2.y pi p.x p.y angle (polygon transform: p, rot(angle)).
 *             out: b2Distance with an empty simplex cache; b2Distance called again with the cache the first call wrote; that
 *             cache's vertex count.
 *   MANIFOLD  in: as DISTANCE.  out: pointCount, type (1 face A = the edge, 2 face B = the polygon; 0 without points), world normal
 *             x,y, then per point: world point x,y, separation (distance from the reference plane minus both polygon radii), the
 *             contact-feature id (indexA | indexB << 8 | typeA << 16 | typeB << 24); unused points 0.
 *   TOI       in: v1.x v1.y v2.x v2.y pi c0.x c0.y a0 c.x c.y a (the polygon body's sweep; localCenter is the engine's, alpha0 = 0).
 *             out: b2TimeOfImpact's state (0 unknown, 1 failed, 2 overlapped, 3 touching, 4 separated), t.
 * Runs on the null stream and synchronises the device.  tests/test_gpu_ll_geom.py checks the results against a float64 reference. */
enum {
    MGYM_LL_GEOM_SHAPES = 0,
    MGYM_LL_GEOM_DISTANCE = 1,
    MGYM_LL_GEOM_MANIFOLD = 2,
    MGYM_LL_GEOM_TOI = 3
};
int mgym_ll_geom_probe(int device, int fn, uint64_t count, const float *in, float *out);

/* hipGraph capture of a caller-issued launch sequence on the env's stream.  What a captured launch freezes and what it does not:
 *  - environment STATE is read when the graph runs: mgym_set_state, mgym_reset (any form) and eager steps between replays are fine.
 *    (LunarLander: a captured step always carries the launches that reset a finished environment WITHOUT a prepared next episode —
 *    empty when every environment has one — because only the run can tell; reset semantics: lunar_lander.rs:727-917 incl. the implicit
 *    step(0) at :911-916.)
 *  - the handle's CONFIGURATION is frozen into kernel arguments: after mgym_set_dispersion_override (deterministic_mode,
 *    lunar_lander.rs:967-970) mgym_graph_launch refuses graphs captured before it with MGYM_ERR_BAD_ARG — capture again.
 *    The pointers passed to the captured calls are frozen too, of course.
 * mgym_get_info may not be called between mgym_graph_begin and mgym_graph_end (it synchronises): MGYM_ERR_BAD_ARG. */
int mgym_graph_begin(mgym_env *env);
int mgym_graph_end(mgym_env *env, void **graph_exec_out);
int mgym_graph_launch(mgym_env *env, void *graph_exec);
int mgym_graph_destroy(void *graph_exec);

#ifdef __cplusplus
}
#endif
#endif /* MGYM_H */
