//! Batched superset of `Gym`: n_envs environments behind one handle, device buffers only.
//! The reference cannot express a batch (StepInfo carries scalars, cartpole.rs:300-305); this is the
//! surface the GPU engine exists for.  Semantics of each call: include/mgym.h.
use crate::sys::*;
use std::ffi::CStr;
use std::os::raw::c_void;

#[derive(Debug)]
pub struct MgymError {
    pub status: i32,
    pub message: String,
}

impl std::fmt::Display for MgymError {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        write!(f, "mgym status {}: {}", self.status, self.message)
    }
}
impl std::error::Error for MgymError {}

pub(crate) fn check(status: i32) -> Result<(), MgymError> {
    if status == MGYM_OK {
        return Ok(());
    }
    let message = unsafe { CStr::from_ptr(mgym_last_error()) }.to_string_lossy().into_owned();
    Err(MgymError { status, message })
}

/// A typed allocation in the env's GPU memory (mgym_malloc / mgym_free).
pub struct DeviceBuf<T: Copy> {
    ptr: *mut T,
    len: usize,
    device: i32,
}

impl<T: Copy> DeviceBuf<T> {
    pub fn new(device: i32, len: usize) -> Result<Self, MgymError> {
        let mut p: *mut c_void = std::ptr::null_mut();
        check(unsafe { mgym_malloc(device, len.max(1) * std::mem::size_of::<T>(), &mut p) })?;
        Ok(Self { ptr: p as *mut T, len, device })
    }
    pub fn as_ptr(&self) -> *mut T {
        self.ptr
    }
    pub fn len(&self) -> usize {
        self.len
    }
    pub fn upload(&mut self, host: &[T]) -> Result<(), MgymError> {
        assert_eq!(host.len(), self.len);
        check(unsafe { mgym_memcpy_h2d(self.device, self.ptr as _, host.as_ptr() as _, std::mem::size_of_val(host)) })
    }
    pub fn download(&self, host: &mut [T]) -> Result<(), MgymError> {
        assert_eq!(host.len(), self.len);
        check(unsafe { mgym_memcpy_d2h(self.device, host.as_mut_ptr() as _, self.ptr as _, std::mem::size_of_val(host)) })
    }
}

impl<T: Copy> Drop for DeviceBuf<T> {
    fn drop(&mut self) {
        unsafe { mgym_free(self.device, self.ptr as _) };
    }
}

/// Output buffers of one step: SoA observation `[obs_dim][n]`, reward, done, truncated.
pub struct StepBuffers {
    pub obs: DeviceBuf<f32>,
    pub reward: DeviceBuf<f32>,
    pub done: DeviceBuf<u8>,
    pub truncated: DeviceBuf<u8>,
}

pub struct VecGym {
    env: *mut mgym_env,
    pub cfg: mgym_config,
    pub spec: mgym_spec,
}

impl VecGym {
    pub fn default_config(kind: i32) -> mgym_config {
        let mut cfg: mgym_config = unsafe { std::mem::zeroed() };
        check(unsafe { mgym_default_config(kind, &mut cfg) }).expect("mgym_default_config");
        cfg
    }

    pub fn new(cfg: mgym_config) -> Result<Self, MgymError> {
        assert_eq!(unsafe { mgym_abi_version() }, MGYM_ABI_VERSION, "libmgym ABI mismatch");
        let mut env: *mut mgym_env = std::ptr::null_mut();
        check(unsafe { mgym_create(&cfg, &mut env) })?;
        let mut spec: mgym_spec = unsafe { std::mem::zeroed() };
        check(unsafe { mgym_get_spec(cfg.kind, &mut spec) })?;
        Ok(Self { env, cfg, spec })
    }

    pub fn n_envs(&self) -> usize {
        self.cfg.n_envs as usize
    }

    pub fn buffers(&self) -> Result<StepBuffers, MgymError> {
        let (n, d) = (self.n_envs(), self.cfg.device);
        Ok(StepBuffers {
            obs: DeviceBuf::new(d, n * self.spec.obs_dim as usize)?,
            reward: DeviceBuf::new(d, n)?,
            done: DeviceBuf::new(d, n)?,
            truncated: DeviceBuf::new(d, n)?,
        })
    }

    /// Enqueue later launches on a caller-owned HIP stream (e.g. candle's / the trainer's).
    pub fn set_stream(&mut self, hip_stream: *mut c_void) -> Result<(), MgymError> {
        check(unsafe { mgym_set_stream(self.env, hip_stream) })
    }

    /// `mask`: device `u8[n]` (non-zero = reset) or None for all.
    pub fn reset(&mut self, mask: Option<&DeviceBuf<u8>>, obs_out: Option<&mut DeviceBuf<f32>>) -> Result<(), MgymError> {
        let m = mask.map_or(std::ptr::null(), |b| b.as_ptr() as *const u8);
        let o = obs_out.map_or(std::ptr::null_mut(), |b| b.as_ptr());
        check(unsafe { mgym_reset(self.env, m, o) })
    }

    /// Reset exactly the envs the last step reported finished (done | truncated).
    pub fn reset_done(&mut self, out: &StepBuffers) -> Result<(), MgymError> {
        check(unsafe { mgym_reset_done(self.env, out.done.as_ptr(), out.truncated.as_ptr(), std::ptr::null_mut()) })
    }

    /// `actions`: device `u32[n]` (f32[n] for MountainCarContinuous).  Asynchronous on the env's stream.
    pub fn step(&mut self, actions: *const c_void, out: &mut StepBuffers) -> Result<(), MgymError> {
        check(unsafe {
            mgym_step(self.env, actions, out.obs.as_ptr(), out.reward.as_ptr(), out.done.as_ptr(), out.truncated.as_ptr())
        })
    }

    /// K fused steps for a caller-supplied action table `[K][n]`; outputs are `[K]`-leading.
    pub fn rollout(
        &mut self,
        actions: *const c_void,
        k: i32,
        obs: *mut f32,
        reward: *mut f32,
        done: *mut u8,
        truncated: *mut u8,
    ) -> Result<(), MgymError> {
        check(unsafe { mgym_rollout(self.env, actions, k, obs, reward, done, truncated) })
    }

    /// K fused steps under an on-device linear policy (`mgym_rollout_linear`): the loop `let a = policy(&obs); env.step(a)` of
    /// cartpole.rs:251-348 / mountain_car.rs:293-330 / lunar_lander.rs:919-1167 without leaving the GPU.  `policy`: CartPole 4 weights + bias
    /// (action 1 if the score is positive); MountainCar three rows of (w_position, w_velocity, bias), LunarLander four rows of (w_0 .. w_7, bias):
    /// the action is the index of the largest score, the first of equal ones; MountainCarContinuous one row, the score is the force.
    /// # Safety
    /// the output pointers are device pointers of `[K][n]` (`[K][obs_dim][n]` for `obs`) elements, or null.
    pub unsafe fn rollout_linear(
        &mut self,
        policy: &[f32],
        k: i32,
        actions_out: *mut c_void,
        obs: *mut f32,
        reward: *mut f32,
        done: *mut u8,
        truncated: *mut u8,
    ) -> Result<(), MgymError> {
        let rows: usize = if self.cfg.kind == MGYM_MOUNTAINCAR { 3 } else if self.cfg.kind == MGYM_LUNARLANDER { 4 } else { 1 };
        let want: usize = rows * (self.spec.obs_dim + 1) as usize;
        if policy.len() != want {
            return Err(MgymError { status: MGYM_ERR_BAD_ARG, message: format!("rollout_linear: {} policy floats for this family, got {}", want, policy.len()) });
        }
        check(unsafe { mgym_rollout_linear(self.env, policy.as_ptr(), k, actions_out, obs, reward, done, truncated) })
    }
    /// K fused steps under an on-device one-hidden-layer policy (`mgym_rollout_mlp`): `policy` holds `W1[H][D]`, `b1[H]`, `W2[A][H]`, `b2[A]` in that order
    /// (the `weight` / `bias` tensors of two `Linear` layers, flattened), D = obs_dim, A = n_actions (1 for MountainCarContinuous, whose score is the force),
    /// 1 <= `hidden` <= 64, `activation` = `MGYM_ACT_RELU` or `MGYM_ACT_TANH`.  Both layers are ascending-index `fmaf` chains from the bias; the action is the
    /// first largest score.  LunarLander runs it as K x (policy kernel, step) by default, and inside its persistent rollout launch (under the conditions of
    /// `rollout_linear`) with `MGYM_LL_ROLLOUT_MLP=1` in the environment: the same words either way.
    /// # Safety
    /// the output pointers are device pointers of `[K][n]` (`[K][obs_dim][n]` for `obs`) elements, or null.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn rollout_mlp(
        &mut self,
        policy: &[f32],
        hidden: i32,
        activation: i32,
        k: i32,
        actions_out: *mut c_void,
        obs: *mut f32,
        reward: *mut f32,
        done: *mut u8,
        truncated: *mut u8,
    ) -> Result<(), MgymError> {
        let (d, a) = (self.spec.obs_dim as usize, if self.spec.action_is_float != 0 { 1 } else { self.spec.n_actions as usize });
        if (1..=64).contains(&hidden) {
            let h = hidden as usize;
            let want = h * (d + 1) + a * (h + 1);
            if policy.len() != want {
                return Err(MgymError { status: MGYM_ERR_BAD_ARG, message: format!("rollout_mlp: {} policy floats for hidden = {}, got {}", want, hidden, policy.len()) });
            }
        }
        check(unsafe { mgym_rollout_mlp(self.env, policy.as_ptr(), hidden, activation, k, actions_out, obs, reward, done, truncated) })
    }
    /// `rollout_mlp` with the action drawn from the softmax of the scores (`mgym_rollout_mlp_sample`): the draw is a pure function of (`policy_seed`,
    /// `policy_call`, global env id, step) and the scores, as `include/mgym.h` states it to the word; the handle keeps no count, so pass a new `policy_call` for
    /// each call that is to draw afresh.  Discrete families only (MountainCarContinuous: `MGYM_ERR_BAD_ARG`); `env_id_base` a multiple of 4; LunarLander always
    /// runs it as K x (policy kernel, step).
    /// # Safety
    /// the output pointers are device pointers of `[K][n]` (`[K][obs_dim][n]` for `obs`) elements, or null.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn rollout_mlp_sample(
        &mut self,
        policy: &[f32],
        hidden: i32,
        activation: i32,
        policy_seed: u64,
        policy_call: u32,
        k: i32,
        actions_out: *mut c_void,
        obs: *mut f32,
        reward: *mut f32,
        done: *mut u8,
        truncated: *mut u8,
    ) -> Result<(), MgymError> {
        let (d, a) = (self.spec.obs_dim as usize, if self.spec.action_is_float != 0 { 1 } else { self.spec.n_actions as usize });
        if (1..=64).contains(&hidden) {
            let h = hidden as usize;
            let want = h * (d + 1) + a * (h + 1);
            if policy.len() != want {
                return Err(MgymError { status: MGYM_ERR_BAD_ARG, message: format!("rollout_mlp_sample: {} policy floats for hidden = {}, got {}", want, hidden, policy.len()) });
            }
        }
        check(unsafe { mgym_rollout_mlp_sample(self.env, policy.as_ptr(), hidden, activation, policy_seed, policy_call, k, actions_out, obs, reward, done, truncated) })
    }
    /// `rollout_mlp` for MountainCarContinuous and Pendulum with the action drawn from a Gaussian around the score (`mgym_rollout_mlp_gauss`): a = mu + sigma * z,
    /// `sigma` finite and >= 0, z a pure function of (`policy_seed`, `policy_call`, global env id, step) as `include/mgym.h` states it to the word; the handle keeps
    /// no count, so pass a new `policy_call` for each call that is to draw afresh.  `actions_out` receives the f32 words before the step's clamp.  The discrete
    /// families: `MGYM_ERR_BAD_ARG`; `env_id_base` a multiple of 4.
    /// # Safety
    /// the output pointers are device pointers of `[K][n]` (`[K][obs_dim][n]` for `obs`) elements, or null.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn rollout_mlp_gauss(
        &mut self,
        policy: &[f32],
        hidden: i32,
        activation: i32,
        sigma: f32,
        policy_seed: u64,
        policy_call: u32,
        k: i32,
        actions_out: *mut c_void,
        obs: *mut f32,
        reward: *mut f32,
        done: *mut u8,
        truncated: *mut u8,
    ) -> Result<(), MgymError> {
        let d = self.spec.obs_dim as usize;
        if (1..=64).contains(&hidden) {
            let h = hidden as usize;
            let want = h * (d + 1) + (h + 1);
            if policy.len() != want {
                return Err(MgymError { status: MGYM_ERR_BAD_ARG, message: format!("rollout_mlp_gauss: {} policy floats for hidden = {}, got {}", want, hidden, policy.len()) });
            }
        }
        check(unsafe { mgym_rollout_mlp_gauss(self.env, policy.as_ptr(), hidden, activation, sigma, policy_seed, policy_call, k, actions_out, obs, reward, done, truncated) })
    }
    /// K fused steps under the on-device two-hidden-layer policy (`mgym_rollout_mlp2`): `policy` = `W1[H1][D], b1[H1], W2[H2][H1], b2[H2], W3[A][H2], b3[A]`
    /// (nn.Linear order), 1 <= `hidden1`, `hidden2` <= 64, `activation` = `MGYM_ACT_RELU` or `MGYM_ACT_TANH_FAST` (the exact tanh is refused), `head` =
    /// `MGYM_HEAD_GREEDY`, `MGYM_HEAD_SAMPLE` (discrete families) or `MGYM_HEAD_GAUSS` (MountainCarContinuous, Pendulum).  `sigma`, `policy_seed` and
    /// `policy_call` are ignored by the heads that do not use them; a drawing head needs `env_id_base` a multiple of 4.
    /// # Safety
    /// the output pointers are device pointers of `[K][n]` (`[K][obs_dim][n]` for `obs`) elements, or null.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn rollout_mlp2(
        &mut self,
        policy: &[f32],
        hidden1: i32,
        hidden2: i32,
        activation: i32,
        head: i32,
        sigma: f32,
        policy_seed: u64,
        policy_call: u32,
        k: i32,
        actions_out: *mut c_void,
        obs: *mut f32,
        reward: *mut f32,
        done: *mut u8,
        truncated: *mut u8,
    ) -> Result<(), MgymError> {
        let d = self.spec.obs_dim as usize;
        let a = if self.spec.action_is_float != 0 { 1 } else { self.spec.n_actions as usize };
        if (1..=64).contains(&hidden1) && (1..=64).contains(&hidden2) {
            let (h1, h2) = (hidden1 as usize, hidden2 as usize);
            let want = h1 * (d + 1) + h2 * (h1 + 1) + a * (h2 + 1);
            if policy.len() != want {
                return Err(MgymError {
                    status: MGYM_ERR_BAD_ARG,
                    message: format!("rollout_mlp2: {} policy floats for hidden1 = {}, hidden2 = {}, got {}", want, hidden1, hidden2, policy.len()),
                });
            }
        }
        check(unsafe {
            mgym_rollout_mlp2(self.env, policy.as_ptr(), hidden1, hidden2, activation, head, sigma, policy_seed, policy_call, k, actions_out, obs, reward, done, truncated)
        })
    }
    /// K fused steps under the on-device uniform random policy (`mgym_rollout_uniform`; every family, the draws as `include/mgym.h` documents them): no action table.
    /// `actions_out` (`[K][n]` u32, may be null) receives the drawn actions.
    #[allow(clippy::too_many_arguments)]
    pub fn rollout_uniform(
        &mut self,
        policy_seed: u64,
        k: i32,
        actions_out: *mut c_void,
        obs: *mut f32,
        reward: *mut f32,
        done: *mut u8,
        truncated: *mut u8,
    ) -> Result<(), MgymError> {
        check(unsafe { mgym_rollout_uniform(self.env, policy_seed, k, actions_out, obs, reward, done, truncated) })
    }

    /// Env-steps that returned `done` or `truncated` since creation (ballot/popcount reduction inside the step
    /// kernels); synchronises the stream.
    pub fn episode_count(&mut self) -> Result<u64, MgymError> {
        let mut c = 0u64;
        check(unsafe { mgym_episode_count(self.env, &mut c) })?;
        Ok(c)
    }

    /// Zero-copy view of the engine-owned observation columns: (pointer, column stride in floats).
    pub fn observation(&self) -> Result<(*const f32, u64), MgymError> {
        let (mut p, mut stride) = (std::ptr::null(), 0u64);
        check(unsafe { mgym_observation(self.env, &mut p, &mut stride) })?;
        Ok((p, stride))
    }

    /// Wait for the stream and surface the sticky device status (invalid action, step before reset).
    pub fn sync(&mut self) -> Result<(), MgymError> {
        check(unsafe { mgym_sync(self.env) })
    }

    // test seams (≙ `Testable`, testing.rs:15-18; `deterministic_mode`, lunar_lander.rs:967-970)
    pub fn set_state(&mut self, blob: &DeviceBuf<f32>) -> Result<(), MgymError> {
        check(unsafe { mgym_set_state(self.env, blob.as_ptr() as _) })
    }
    pub fn get_state(&mut self, blob: &mut DeviceBuf<f32>) -> Result<(), MgymError> {
        check(unsafe { mgym_get_state(self.env, blob.as_ptr() as _) })
    }
    /// The elapsed count of `mgym_config::max_episode_steps` (caller-visible steps since each env's last reset), device `u32[n]`.
    pub fn get_elapsed_steps(&mut self, out: &mut DeviceBuf<u32>) -> Result<(), MgymError> {
        check(unsafe { mgym_get_elapsed_steps(self.env, out.as_ptr()) })
    }
    pub fn set_elapsed_steps(&mut self, input: &DeviceBuf<u32>) -> Result<(), MgymError> {
        check(unsafe { mgym_set_elapsed_steps(self.env, input.as_ptr() as *const u32) })
    }
    /// The final observations of auto-reset episodes (`mgym_set_final_obs_out`): `buf` holds `[steps_cap][obs_dim][n_envs]` floats and is written by every
    /// stepping call where `done | truncated` is set, with the observation the step produced before the fused reset; `None` turns the channel off.
    /// The caller keeps `buf` alive while it is set.
    pub fn set_final_obs_out(&mut self, buf: Option<&mut DeviceBuf<f32>>, steps_cap: i32) -> Result<(), MgymError> {
        check(unsafe { mgym_set_final_obs_out(self.env, buf.map_or(std::ptr::null_mut(), |b| b.as_ptr()), steps_cap) })
    }
    /// Generalised advantage estimation over a rollout's `[K][n]` outputs in one launch (`mgym_gae`, defined to the f32 word in `include/mgym.h`).  Device
    /// pointers: `done` / `truncated` / `final_value` may be null, and one of `adv_out` / `ret_out`; `final_value` is read only where `truncated && !done`.
    #[allow(clippy::too_many_arguments)]
    pub fn gae(
        &mut self,
        k: i32,
        reward: *const f32,
        done: *const u8,
        truncated: *const u8,
        value: *const f32,
        last_value: *const f32,
        final_value: *const f32,
        gamma: f32,
        lambda: f32,
        adv_out: *mut f32,
        ret_out: *mut f32,
    ) -> Result<(), MgymError> {
        check(unsafe { mgym_gae(self.env, k, reward, done, truncated, value, last_value, final_value, gamma, lambda, adv_out, ret_out) })
    }
    /// A critic's values over a rollout's buffers in the shapes `gae` takes (`mgym_value_mlp`, `include/mgym.h`).  `critic`: host floats in `nn.Linear` order, one
    /// hidden layer (`hidden2 == 0`) or two; the other pointers are device pointers.  `final_obs` / `final_value_out` / `truncated` are all set or the first two
    /// null; `done` may be null.  `final_value_out` is written only where `truncated && !done`, and `final_obs` is read only there.
    #[allow(clippy::too_many_arguments)]
    pub fn value_mlp(
        &mut self,
        critic: &[f32],
        hidden1: i32,
        hidden2: i32,
        activation: i32,
        k: i32,
        obs_first: *const f32,
        obs: *const f32,
        final_obs: *const f32,
        done: *const u8,
        truncated: *const u8,
        value_out: *mut f32,
        last_value_out: *mut f32,
        final_value_out: *mut f32,
    ) -> Result<(), MgymError> {
        check(unsafe {
            mgym_value_mlp(self.env, critic.as_ptr(), hidden1, hidden2, activation, k, obs_first, obs, final_obs, done, truncated, value_out, last_value_out, final_value_out)
        })
    }
    /// The actor's log-probabilities of a rollout's actions (`mgym_logprob_mlp`, `include/mgym.h`).  `policy`: host floats in `nn.Linear` order, one hidden layer
    /// (`hidden2 == 0`) or two; `head`: `MGYM_HEAD_SAMPLE` (1, the discrete families) or `MGYM_HEAD_GAUSS` (2, the continuous ones; `sigma` positive and normal);
    /// the other pointers are device pointers: `actions` the rollout's `actions_out` words, `logp_out` `[K][n]`.
    #[allow(clippy::too_many_arguments)]
    pub fn logprob_mlp(
        &mut self,
        policy: &[f32],
        hidden1: i32,
        hidden2: i32,
        activation: i32,
        head: i32,
        sigma: f32,
        k: i32,
        obs_first: *const f32,
        obs: *const f32,
        actions: *const c_void,
        logp_out: *mut f32,
    ) -> Result<(), MgymError> {
        check(unsafe { mgym_logprob_mlp(self.env, policy.as_ptr(), hidden1, hidden2, activation, head, sigma, k, obs_first, obs, actions, logp_out) })
    }
    /// `(min_bytes, best_bytes)` of the workspace of the gradient calls at this hidden width (`mgym_grad_workspace_bytes`).
    pub fn grad_workspace_bytes(kind: i32, hidden: i32) -> Result<(usize, usize), MgymError> {
        let (mut lo, mut hi) = (0usize, 0usize);
        check(unsafe { mgym_grad_workspace_bytes(kind, hidden, &mut lo, &mut hi) })?;
        Ok((lo, hi))
    }
    /// PPO's clipped loss and the actor's gradient over a rollout's buffers (`mgym_ppo_grad_mlp`, `include/mgym.h`).  `policy`: host floats in `nn.Linear`
    /// order, one hidden layer; the range is the environments `env_first .. env_first + env_count` over all `k` steps; the other pointers are device
    /// pointers: `workspace` 16-byte aligned, `grad_out` the parameters' gradient and one more word, `stats_out` 8 floats.
    #[allow(clippy::too_many_arguments)]
    pub fn ppo_grad_mlp(
        &mut self,
        policy: &[f32],
        hidden: i32,
        activation: i32,
        head: i32,
        sigma: f32,
        k: i32,
        env_first: u64,
        env_count: u64,
        obs_first: *const f32,
        obs: *const f32,
        actions: *const c_void,
        logp_old: *const f32,
        adv: *const f32,
        clip: f32,
        ent_coef: f32,
        workspace: *mut c_void,
        workspace_bytes: usize,
        grad_out: *mut f32,
        stats_out: *mut f32,
    ) -> Result<(), MgymError> {
        check(unsafe {
            mgym_ppo_grad_mlp(self.env, policy.as_ptr(), hidden, activation, head, sigma, k, env_first, env_count, obs_first, obs, actions, logp_old, adv, clip, ent_coef,
                              workspace, workspace_bytes, grad_out, stats_out)
        })
    }
    /// A one-hidden-layer critic's loss `1/2 mean((V - ret)^2)` and its gradient over the same range (`mgym_value_grad_mlp`).
    #[allow(clippy::too_many_arguments)]
    pub fn value_grad_mlp(
        &mut self,
        critic: &[f32],
        hidden: i32,
        activation: i32,
        k: i32,
        env_first: u64,
        env_count: u64,
        obs_first: *const f32,
        obs: *const f32,
        ret: *const f32,
        workspace: *mut c_void,
        workspace_bytes: usize,
        grad_out: *mut f32,
        stats_out: *mut f32,
    ) -> Result<(), MgymError> {
        check(unsafe {
            mgym_value_grad_mlp(self.env, critic.as_ptr(), hidden, activation, k, env_first, env_count, obs_first, obs, ret, workspace, workspace_bytes, grad_out, stats_out)
        })
    }
    /// `(min_bytes, best_bytes)` of the workspace of the two-layer gradient calls at these widths (`mgym_grad_workspace_bytes2`).
    pub fn grad_workspace_bytes2(kind: i32, hidden1: i32, hidden2: i32) -> Result<(usize, usize), MgymError> {
        let (mut lo, mut hi) = (0usize, 0usize);
        check(unsafe { mgym_grad_workspace_bytes2(kind, hidden1, hidden2, &mut lo, &mut hi) })?;
        Ok((lo, hi))
    }
    /// `ppo_grad_mlp` for the two-hidden-layer actor of `rollout_mlp2` (`mgym_ppo_grad_mlp2`): `policy` in that call's layout; `grad_out` receives
    /// `dW1, db1, dW2, db2, dW3, db3` and one more word.
    #[allow(clippy::too_many_arguments)]
    pub fn ppo_grad_mlp2(
        &mut self,
        policy: &[f32],
        hidden1: i32,
        hidden2: i32,
        activation: i32,
        head: i32,
        sigma: f32,
        k: i32,
        env_first: u64,
        env_count: u64,
        obs_first: *const f32,
        obs: *const f32,
        actions: *const c_void,
        logp_old: *const f32,
        adv: *const f32,
        clip: f32,
        ent_coef: f32,
        workspace: *mut c_void,
        workspace_bytes: usize,
        grad_out: *mut f32,
        stats_out: *mut f32,
    ) -> Result<(), MgymError> {
        check(unsafe {
            mgym_ppo_grad_mlp2(self.env, policy.as_ptr(), hidden1, hidden2, activation, head, sigma, k, env_first, env_count, obs_first, obs, actions, logp_old, adv, clip,
                               ent_coef, workspace, workspace_bytes, grad_out, stats_out)
        })
    }
    /// `value_grad_mlp` for a two-hidden-layer critic (`mgym_value_grad_mlp2`).
    #[allow(clippy::too_many_arguments)]
    pub fn value_grad_mlp2(
        &mut self,
        critic: &[f32],
        hidden1: i32,
        hidden2: i32,
        activation: i32,
        k: i32,
        env_first: u64,
        env_count: u64,
        obs_first: *const f32,
        obs: *const f32,
        ret: *const f32,
        workspace: *mut c_void,
        workspace_bytes: usize,
        grad_out: *mut f32,
        stats_out: *mut f32,
    ) -> Result<(), MgymError> {
        check(unsafe {
            mgym_value_grad_mlp2(self.env, critic.as_ptr(), hidden1, hidden2, activation, k, env_first, env_count, obs_first, obs, ret, workspace, workspace_bytes,
                                 grad_out, stats_out)
        })
    }
    /// The return and length of the episodes that end inside a rollout (`mgym_episode_returns`): `ep_return` / `ep_length` are the caller's carry of the
    /// running episodes (read and written); `return_out` / `length_out` (`[K][n]`, may be null) are written only where `done | truncated`.
    #[allow(clippy::too_many_arguments)]
    pub fn episode_returns(
        &mut self,
        k: i32,
        reward: *const f32,
        done: *const u8,
        truncated: *const u8,
        ep_return: &mut DeviceBuf<f32>,
        ep_length: &mut DeviceBuf<u32>,
        return_out: *mut f32,
        length_out: *mut u32,
    ) -> Result<(), MgymError> {
        check(unsafe { mgym_episode_returns(self.env, k, reward, done, truncated, ep_return.as_ptr(), ep_length.as_ptr(), return_out, length_out) })
    }
    pub fn reset_deterministic(&mut self, obs_out: &mut DeviceBuf<f32>) -> Result<(), MgymError> {
        check(unsafe { mgym_reset_deterministic(self.env, obs_out.as_ptr()) })
    }
    pub fn set_dispersion_override(&mut self, disp: Option<&DeviceBuf<f32>>) -> Result<(), MgymError> {
        check(unsafe { mgym_set_dispersion_override(self.env, disp.map_or(std::ptr::null(), |b| b.as_ptr() as *const f32)) })
    }
}

impl Drop for VecGym {
    fn drop(&mut self) {
        unsafe { mgym_destroy(self.env) };
    }
}
