"""Host-side mirror of the reference's environment interface over the libmgym C ABI.

Reference surface (ModuRL/ModuRL_Gym, `impl Gym for ...`):
    CartPoleV1::builder().sutton_barto_reward(..).is_euler(..).build()   cartpole.rs:34-44
    MountainCarV0::builder().goal_velocity(..).build()                   mountain_car.rs:25-34
    LunarLanderV3::builder().gravity(..).enable_wind(..)...build()       lunar_lander.rs:278-291
    reset() -> Tensor, step(action) -> StepInfo{state, reward, done, truncated}
The single-env classes below keep those names, argument meanings and error behaviour
(panics become exceptions).  `VecEnv` is the batched superset the GPU engine exists for:
n_envs environments, SoA buffers, one kernel launch per reset()/step().

Python is test/bench plumbing here (the reference is Rust; its toolchain is absent from this
image, INTEGRATION.md shows the Rust shim).  The compute path is HIP only: nothing in this
package falls back to a CPU implementation.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib as L

StepInfo = namedtuple("StepInfo", ["state", "reward", "done", "truncated"])  # modurl::gym::StepInfo

KIND_NAMES = {L.CARTPOLE: "CartPoleV1", L.MOUNTAINCAR: "MountainCarV0",
              L.MOUNTAINCAR_CONT: "MountainCarContinuousV0", L.LUNARLANDER: "LunarLanderV3", L.PENDULUM: "PendulumV1", L.ACROBOT: "AcrobotV1"}


class MgymError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"mgym status {status}: {msg}")
        self.status = status


class InvalidActionError(MgymError, ValueError):
    """assert!(self.action_space.contains(&action)) — cartpole.rs:252, mountain_car.rs:294"""


class NotResetError(MgymError):
    """assert!(self.lander.is_some(), "You forgot to call reset()") — lunar_lander.rs:920"""


class BadConfigError(MgymError, ValueError):
    """assert!(-12.0 < gravity && gravity < 0.0) — lunar_lander.rs:292-296"""


class PolicyShapeError(MgymError, ValueError):
    """rollout_linear_device: the policy does not hold the number of floats the family takes (status ERR_BAD_ARG)"""


_EXC = {L.ERR_INVALID_ACTION: InvalidActionError, L.ERR_NOT_RESET: NotResetError, L.ERR_BAD_CONFIG: BadConfigError}


def _check(st):
    if st != L.OK:
        msg = L.load().mgym_last_error().decode(errors="replace")
        raise _EXC.get(st, MgymError)(st, msg)


def device_count():
    n = C.c_int(0)
    st = L.load().mgym_device_count(C.byref(n))
    return n.value if st == L.OK else 0


def get_spec(kind):
    s = L.Spec()
    _check(L.load().mgym_get_spec(kind, C.byref(s)))
    return s


class DeviceArray:
    """A typed device allocation made through mgym_malloc (for callers without torch)."""

    def __init__(self, shape, dtype, device=0):
        self.shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.dtype = np.dtype(dtype)
        self.device = device
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        p = C.c_void_p()
        _check(L.load().mgym_malloc(device, self.nbytes, C.byref(p)))
        self.ptr = p.value

    def __del__(self):
        if getattr(self, "ptr", None):
            try:
                L.load().mgym_free(self.device, self.ptr)
            except Exception:
                pass
            self.ptr = None

    def data_ptr(self):
        return self.ptr

    def copy_from(self, host):
        a = np.ascontiguousarray(host, self.dtype)
        assert a.nbytes == self.nbytes, (a.shape, self.shape)
        _check(L.load().mgym_memcpy_h2d(self.device, self.ptr, a.ctypes.data, self.nbytes))
        return self

    def numpy(self):
        out = np.empty(self.shape, self.dtype)
        _check(L.load().mgym_memcpy_d2h(self.device, out.ctypes.data, self.ptr, self.nbytes))
        return out

    @classmethod
    def from_numpy(cls, a, device=0):
        a = np.ascontiguousarray(a)
        return cls(a.shape, a.dtype, device).copy_from(a)


def _ptr(x):
    """device pointer of None / int / DeviceArray / torch tensor"""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    return x.data_ptr()


# the names the policy entry points take for an MGYM_ACT_* / MGYM_HEAD_* value (the value itself passes through)
_ACTIVATIONS = {"relu": L.ACT_RELU, "tanh": L.ACT_TANH, "tanh_fast": L.ACT_TANH_FAST}
_HEADS = {"greedy": L.HEAD_GREEDY, "sample": L.HEAD_SAMPLE, "gauss": L.HEAD_GAUSS}


_ACT_WORDING = 'activation must be "relu", "tanh", "tanh_fast" or an MGYM_ACT_* value'
_DENSITY_HEAD_WORDING = 'head must be "sample", "gauss" or an MGYM_HEAD_* value'   # (the calls that need a density take no "greedy")


def _named(names, value, wording):
    """names[value], or the integer value itself; anything else raises PolicyShapeError with `wording`"""
    v = names.get(value, value)
    if not isinstance(v, (int, np.integer)):
        raise PolicyShapeError(L.ERR_BAD_ARG, f"{wording}, got {value!r}")
    return int(v)


def _mlp_floats(D, A, h1, h2=0):
    """the packed float32 words of a net D -> h1 (-> h2) -> A, h2 = 0 for one hidden layer; None when a width is out of range (the engine rejects the call for
    it first)"""
    if not (1 <= h1 <= 64 and 0 <= h2 <= 64):
        return None
    return h1 * (D + 1) + (h2 * (h1 + 1) + A * (h2 + 1) if h2 else A * (h1 + 1))


def _policy_floats(policy, want, what):
    """policy as the contiguous float32 words an entry point reads: `want` of them, or PolicyShapeError "policy must hold .. floats for `what`" (want None: not
    checked, the engine rejects the call for its hidden width first)"""
    pol = np.ascontiguousarray(np.asarray(policy, np.float32).ravel())
    if want is not None and pol.size != want:
        raise PolicyShapeError(L.ERR_BAD_ARG, f"policy must hold {want} floats for {what}, got {pol.size}")
    return pol


def _fptr(pol):
    """the const float* of a float32 array (None: NULL, which the engine rejects)"""
    return None if pol is None else pol.ctypes.data_as(C.POINTER(C.c_float))


def _draw(seed, call):
    """the policy seed and call word of the drawing entry points as the ABI takes them: 64 and 32 bits"""
    return int(seed) & (2**64 - 1), int(call) & 0xFFFFFFFF


class VecEnv:
    """n_envs environments of one family on one GPU (one mgym_env handle, one stream)."""

    def __init__(self, kind, n_envs=1, device=0, seed=0, env_id_base=0, auto_reset=False, stream=None,
                 sutton_barto_reward=False, is_euler=True, goal_velocity=0.0, gravity=None, enable_wind=False,
                 wind_power=15.0, turbulence_power=1.5, max_episode_steps=0):
        lib = L.load()
        cfg = L.Config()
        _check(lib.mgym_default_config(kind, C.byref(cfg)))
        cfg.device, cfg.n_envs, cfg.env_id_base, cfg.seed = device, int(n_envs), int(env_id_base), int(seed)
        cfg.flags = L.FLAG_AUTO_RESET if auto_reset else 0
        cfg.sutton_barto_reward, cfg.is_euler = int(sutton_barto_reward), int(is_euler)
        cfg.goal_velocity = goal_velocity
        if gravity is not None:   # None: the family's default (LunarLander -10, Pendulum 10)
            cfg.gravity = gravity
        cfg.enable_wind = int(enable_wind)
        cfg.wind_power, cfg.turbulence_power = wind_power, turbulence_power
        # episode time limit (include/mgym.h): 0 = off, the reference's behaviour; CartPole keeps the reference's 500
        if not 0 <= int(max_episode_steps) <= 0xFFFFFFFF:
            raise BadConfigError(L.ERR_BAD_CONFIG, f"max_episode_steps must be between 0 and 65535, got {max_episode_steps}")
        cfg.max_episode_steps = int(max_episode_steps)
        h = C.c_void_p()
        self._h = None
        _check(lib.mgym_create(C.byref(cfg), C.byref(h)))
        self._h, self._lib = h, lib
        self.kind, self.n, self.device = kind, int(n_envs), device
        self.max_episode_steps = int(max_episode_steps)
        spec = get_spec(kind)
        self.obs_dim, self.n_actions, self.action_is_float = spec.obs_dim, spec.n_actions, bool(spec.action_is_float)
        self.action_dtype = np.float32 if self.action_is_float else np.uint32
        if stream is not None:
            self.set_stream(stream)
        self._bufs = None
        self._disp = None

    # ---- lifetime -------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.mgym_destroy(self._h)
            self._h = None

    __del__ = close

    def set_stream(self, hip_stream):
        _check(self._lib.mgym_set_stream(self._h, C.c_void_p(int(hip_stream))))

    def sync(self):
        """hipStreamSynchronize + sticky device status (raises InvalidActionError / NotResetError)."""
        _check(self._lib.mgym_sync(self._h))

    def info(self):
        """mgym_get_info as a dict: kind, n_envs, GPU_MAX_HW_QUEUES as seen at creation; LunarLander adds its launch
        structure and how many of its streams were seen running at the same time (a probe launch on each)."""
        buf = C.create_string_buffer(1024)
        _check(self._lib.mgym_get_info(self._h, buf, len(buf)))
        return dict(line.split("=", 1) for line in buf.value.decode().splitlines() if "=" in line)

    # ---- raw device-pointer path (what bench.py and a Rust/C caller use) --------------
    def set_final_obs_out_device(self, final_obs_out, steps_cap=0):
        """mgym_set_final_obs_out: a device buffer [steps_cap][obs_dim][n] (pointer, DeviceArray or tensor) that every stepping call fills, where
        done | truncated is set, with the observation the step produced before the fused reset; None turns the channel off.  The caller keeps
        the buffer alive while it is set (auto-reset handles of CartPole, MountainCar(+Continuous) and Pendulum)."""
        _check(self._lib.mgym_set_final_obs_out(self._h, _ptr(final_obs_out), int(steps_cap)))
        self._final_obs = final_obs_out   # (keeps a DeviceArray / tensor alive)

    def reset_device(self, mask=None, obs_out=None):
        _check(self._lib.mgym_reset(self._h, _ptr(mask), _ptr(obs_out)))

    def reset_done_device(self, done, trunc, obs_out=None):
        _check(self._lib.mgym_reset_done(self._h, _ptr(done), _ptr(trunc), _ptr(obs_out)))

    def step_device(self, actions, obs_out=None, reward_out=None, done_out=None, trunc_out=None):
        _check(self._lib.mgym_step(self._h, _ptr(actions), _ptr(obs_out), _ptr(reward_out), _ptr(done_out),
                                   _ptr(trunc_out)))

    def rollout_device(self, actions, K, obs_out=None, reward_out=None, done_out=None, trunc_out=None):
        _check(self._lib.mgym_rollout(self._h, _ptr(actions), int(K), _ptr(obs_out), _ptr(reward_out), _ptr(done_out),
                                      _ptr(trunc_out)))

    def _policy_device(self, fn, lead, outs):
        """one policy entry point of the C ABI: fn(handle, its own leading arguments `lead`, already converted, K among them; the five output pointers)"""
        _check(fn(self._h, *lead, *(_ptr(x) for x in outs)))

    def rollout_uniform_device(self, policy_seed, K, actions_out=None, obs_out=None, reward_out=None, done_out=None, trunc_out=None):
        """K fused steps under the on-device uniform random policy (mgym_rollout_uniform; every family — include/mgym.h documents the draws)."""
        self._policy_device(self._lib.mgym_rollout_uniform, (int(policy_seed), int(K)), (actions_out, obs_out, reward_out, done_out, trunc_out))

    def rollout_linear_device(self, policy, K, actions_out=None, obs_out=None, reward_out=None, done_out=None, trunc_out=None):
        """K fused steps under the on-device linear policy (mgym_rollout_linear): policy = obs_dim weights + bias (CartPole: action 1 if the score is
        positive; MountainCarContinuous: the score is the force; Pendulum: (w_cos, w_sin, w_thdot, b), the score is the torque), or one such row per action (MountainCar: 3 rows, Acrobot: 3 rows of 6 weights + bias, LunarLander: 4 rows of 8 weights + bias;
        the index of the largest score, the first of equal ones).  Host floats.  A policy of the wrong length raises PolicyShapeError (an MgymError with
        status ERR_BAD_ARG and a ValueError)."""
        rows = {L.MOUNTAINCAR: 3, L.ACROBOT: 3, L.LUNARLANDER: 4}.get(self.kind, 1)   # a row of (weights, bias) per action for the argmax families
        pol = _policy_floats(policy, rows * (self.obs_dim + 1), "this family")
        self._policy_device(self._lib.mgym_rollout_linear, (_fptr(pol), int(K)), (actions_out, obs_out, reward_out, done_out, trunc_out))

    def _rollout_host(self, K, call, action_dtype=np.uint32):
        """The host-array form of every K-step call: allocate the [K, ..] outputs, run call(actions, obs, reward, done, trunc) on them, sync
        -> (actions [K, n], obs [K, obs_dim, n], reward [K, n], done, trunc) as host arrays; without the actions if action_dtype is None."""
        n = max(self.n, 1)
        shapes = [(K, self.n), (K, self.obs_dim, self.n), (K, self.n), (K, self.n), (K, self.n)]
        dtypes = [action_dtype, np.float32, np.float32, np.uint8, np.uint8]
        if action_dtype is None:
            shapes, dtypes = shapes[1:], dtypes[1:]
        outs = [DeviceArray(sh[:-1] + (n,), dt, self.device) for sh, dt in zip(shapes, dtypes)]
        call(*outs)
        self.sync()
        return tuple(x.numpy().reshape(-1)[: int(np.prod(sh))].reshape(sh) for x, sh in zip(outs, shapes))

    def rollout_linear(self, policy, K):
        """host-array form: -> (actions [K, n], obs [K, obs_dim, n], reward [K, n], done, trunc)"""
        return self._rollout_host(K, lambda *out: self.rollout_linear_device(policy, K, *out))

    def mlp_dims(self):
        """(D, A) of mgym_rollout_mlp for this family: obs_dim inputs; one score per action, or the one force / torque of MountainCarContinuous / Pendulum"""
        return self.obs_dim, (1 if self.action_is_float else self.n_actions)

    def pack_mlp(self, w1, b1, w2, b2):
        """nn.Linear-layout weights (w1 [H, D], b1 [H], w2 [A, H], b2 [A]; arrays or anything np.asarray takes) -> (policy, H): the H (D + 1) + A (H + 1)
        float32 words mgym_rollout_mlp reads.  Shapes are checked against the family (PolicyShapeError); H itself is checked by the engine."""
        D, A = self.mlp_dims()
        w1, b1, w2, b2 = (np.asarray(x, np.float32) for x in (w1, b1, w2, b2))
        H = w1.shape[0] if w1.ndim == 2 else -1
        if w1.shape != (H, D) or b1.shape != (H,) or w2.shape != (A, H) or b2.shape != (A,):
            raise PolicyShapeError(L.ERR_BAD_ARG, f"{KIND_NAMES[self.kind]} takes w1 [H, {D}], b1 [H], w2 [{A}, H], b2 [{A}]; got "
                                                  f"{w1.shape}, {b1.shape}, {w2.shape}, {b2.shape}")
        return np.concatenate([w1.ravel(), b1, w2.ravel(), b2]).astype(np.float32), H

    def _mlp_args(self, policy, hidden, activation):
        """(contiguous float32 policy or None, activation value) of the hidden-layer entry points, the policy's length checked against H and the family"""
        act = _named(_ACTIVATIONS, activation, _ACT_WORDING)
        return None if policy is None else _policy_floats(policy, _mlp_floats(*self.mlp_dims(), int(hidden)), f"hidden = {hidden}"), act

    def _family_head(self):
        """the head a family's actions have: the name a call takes where `head` is None"""
        return "gauss" if self.action_dtype == np.float32 else "sample"

    def rollout_mlp_device(self, policy, hidden, activation, K, actions_out=None, obs_out=None, reward_out=None, done_out=None, trunc_out=None):
        """K fused steps under the on-device one-hidden-layer policy (mgym_rollout_mlp): `policy` = the packed host floats of pack_mlp (or None, which the
        engine rejects), `hidden` = H, `activation` = "relu" / "tanh" / "tanh_fast" or the MGYM_ACT_* value ("tanh" is glibc's tanhf to the bit and most of the
        launch's time; "tanh_fast" is the cheap tanh include/mgym.h defines word for word, within 2.5 f32 spacings of tanh).  A policy of the wrong length for H raises PolicyShapeError."""
        pol, act = self._mlp_args(policy, hidden, activation)
        self._policy_device(self._lib.mgym_rollout_mlp, (_fptr(pol), int(hidden), act, int(K)), (actions_out, obs_out, reward_out, done_out, trunc_out))

    def rollout_mlp_sample_device(self, policy, hidden, activation, seed, call, K, actions_out=None, obs_out=None, reward_out=None, done_out=None, trunc_out=None):
        """rollout_mlp_device with the action drawn from the softmax of the scores (mgym_rollout_mlp_sample; the discrete families): the draw is a pure
        function of (seed, call, global env id, step) and the scores — include/mgym.h states it to the word.  The handle keeps no count: pass a new `call`
        (a 32-bit word) for each call that is to draw afresh."""
        pol, act = self._mlp_args(policy, hidden, activation)
        self._policy_device(self._lib.mgym_rollout_mlp_sample, (_fptr(pol), int(hidden), act, *_draw(seed, call), int(K)),
                            (actions_out, obs_out, reward_out, done_out, trunc_out))

    def rollout_mlp_gauss_device(self, policy, hidden, activation, sigma, seed, call, K, actions_out=None, obs_out=None, reward_out=None, done_out=None, trunc_out=None):
        """rollout_mlp_device for MountainCarContinuous and Pendulum with the action drawn from a Gaussian around the score (mgym_rollout_mlp_gauss):
        a = mu + sigma * z, `sigma` finite and >= 0, z a pure function of (seed, call, global env id, step) — include/mgym.h states it to the word.
        actions_out receives a before the step's clamp.  The handle keeps no count: pass a new `call` (a 32-bit word) for each call that is to draw afresh."""
        pol, act = self._mlp_args(policy, hidden, activation)
        self._policy_device(self._lib.mgym_rollout_mlp_gauss, (_fptr(pol), int(hidden), act, float(sigma), *_draw(seed, call), int(K)),
                            (actions_out, obs_out, reward_out, done_out, trunc_out))

    def rollout_mlp(self, w1, b1, w2, b2, K, activation="relu"):
        """host-array form: -> (actions [K, n], obs [K, obs_dim, n], reward [K, n], done, trunc); actions float32 for MountainCarContinuous"""
        policy, H = self.pack_mlp(w1, b1, w2, b2)
        return self._rollout_host(K, lambda *out: self.rollout_mlp_device(policy, H, activation, K, *out), self.action_dtype)

    def rollout_mlp_sample(self, w1, b1, w2, b2, K, seed, call=0, activation="relu"):
        """host-array form of rollout_mlp_sample_device: -> (actions [K, n], obs [K, obs_dim, n], reward [K, n], done, trunc)"""
        policy, H = self.pack_mlp(w1, b1, w2, b2)
        return self._rollout_host(K, lambda *out: self.rollout_mlp_sample_device(policy, H, activation, seed, call, K, *out), self.action_dtype)

    def rollout_mlp_gauss(self, w1, b1, w2, b2, K, sigma, seed, call=0, activation="relu"):
        """host-array form of rollout_mlp_gauss_device: -> (actions [K, n] float32, obs [K, obs_dim, n], reward [K, n], done, trunc)"""
        policy, H = self.pack_mlp(w1, b1, w2, b2)
        return self._rollout_host(K, lambda *out: self.rollout_mlp_gauss_device(policy, H, activation, sigma, seed, call, K, *out), np.float32)

    def pack_mlp2(self, w1, b1, w2, b2, w3, b3):
        """nn.Linear-layout weights of Linear(D, H1) - act - Linear(H1, H2) - act - Linear(H2, A) (w1 [H1, D], b1 [H1], w2 [H2, H1], b2 [H2], w3 [A, H2], b3 [A])
        -> (policy, H1, H2): the float32 words mgym_rollout_mlp2 reads.  Shapes are checked against the family (PolicyShapeError); H1 and H2 by the engine."""
        D, A = self.mlp_dims()
        w1, b1, w2, b2, w3, b3 = (np.asarray(x, np.float32) for x in (w1, b1, w2, b2, w3, b3))
        H1 = w1.shape[0] if w1.ndim == 2 else -1
        H2 = w2.shape[0] if w2.ndim == 2 else -1
        if w1.shape != (H1, D) or b1.shape != (H1,) or w2.shape != (H2, H1) or b2.shape != (H2,) or w3.shape != (A, H2) or b3.shape != (A,):
            raise PolicyShapeError(L.ERR_BAD_ARG, f"{KIND_NAMES[self.kind]} takes w1 [H1, {D}], b1 [H1], w2 [H2, H1], b2 [H2], w3 [{A}, H2], b3 [{A}]; got "
                                                  f"{w1.shape}, {b1.shape}, {w2.shape}, {b2.shape}, {w3.shape}, {b3.shape}")
        return np.concatenate([w1.ravel(), b1, w2.ravel(), b2, w3.ravel(), b3]).astype(np.float32), H1, H2

    def rollout_mlp2_device(self, policy, hidden1, hidden2, activation, head, sigma, seed, call, K, actions_out=None, obs_out=None, reward_out=None, done_out=None,
                            trunc_out=None):
        """K fused steps under the on-device two-hidden-layer policy (mgym_rollout_mlp2): `policy` = the packed host floats of pack_mlp2 (or None, which the
        engine rejects), `activation` = "relu" / "tanh_fast" or the MGYM_ACT_* value (the exact tanh is refused), `head` = "greedy" (argmax / the score), "sample"
        (the draw of rollout_mlp_sample; discrete families) or "gauss" (mu + sigma * z of rollout_mlp_gauss; MountainCarContinuous, Pendulum) or the MGYM_HEAD_*
        value.  sigma, seed and call are ignored by the heads that do not use them.  A policy of the wrong length for (H1, H2) raises PolicyShapeError."""
        act = _named(_ACTIVATIONS, activation, 'activation must be "relu", "tanh_fast" or an MGYM_ACT_* value')
        hd = _named(_HEADS, head, 'head must be "greedy", "sample", "gauss" or an MGYM_HEAD_* value')
        (D, A), h1, h2 = self.mlp_dims(), int(hidden1), int(hidden2)
        want = h1 * (D + 1) + h2 * (h1 + 1) + A * (h2 + 1) if 1 <= h1 <= 64 and 1 <= h2 <= 64 else None
        pol = None if policy is None else _policy_floats(policy, want, f"hidden1 = {h1}, hidden2 = {h2}")
        self._policy_device(self._lib.mgym_rollout_mlp2, (_fptr(pol), h1, h2, act, hd, float(sigma), *_draw(seed, call), int(K)),
                            (actions_out, obs_out, reward_out, done_out, trunc_out))

    def rollout_mlp2(self, w1, b1, w2, b2, w3, b3, K, activation="relu", head="greedy", sigma=0.0, seed=0, call=0):
        """host-array form of rollout_mlp2_device: -> (actions [K, n], obs [K, obs_dim, n], reward [K, n], done, trunc); actions float32 for the continuous families"""
        policy, H1, H2 = self.pack_mlp2(w1, b1, w2, b2, w3, b3)
        return self._rollout_host(K, lambda *out: self.rollout_mlp2_device(policy, H1, H2, activation, head, sigma, seed, call, K, *out), self.action_dtype)

    def rollout_uniform(self, policy_seed, K):
        """host-array form: -> (actions [K, n], obs [K, obs_dim, n], reward [K, n], done, trunc)"""
        return self._rollout_host(K, lambda *out: self.rollout_uniform_device(policy_seed, K, *out))

    def gae_device(self, K, reward, done, trunc, value, last_value, final_value, gamma, lam, adv_out=None, ret_out=None):
        """mgym_gae on device buffers (pointers, DeviceArrays or tensors): reward / value [K, n], done / trunc uint8 [K, n] or None, last_value [n], final_value
        [K, n] or None (read only where trunc && !done), adv_out / ret_out [K, n] (one may be None).  On the env's stream, nothing synchronised."""
        _check(self._lib.mgym_gae(self._h, int(K), _ptr(reward), _ptr(done), _ptr(trunc), _ptr(value), _ptr(last_value), _ptr(final_value), float(gamma),
                                  float(lam), _ptr(adv_out), _ptr(ret_out)))

    def episode_returns_device(self, K, reward, done, trunc, ep_return, ep_length, return_out=None, length_out=None):
        """mgym_episode_returns on device buffers: reward [K, n], done / trunc uint8 [K, n] or None, the caller's carry ep_return float32 [n] and ep_length
        uint32 [n] (read and written), return_out / length_out [K, n] or None, written only where done | trunc.  On the env's stream, nothing synchronised."""
        _check(self._lib.mgym_episode_returns(self._h, int(K), _ptr(reward), _ptr(done), _ptr(trunc), _ptr(ep_return), _ptr(ep_length), _ptr(return_out),
                                              _ptr(length_out)))

    def _dev(self, a, dtype, shape):
        """a host array as a DeviceArray of the given shape (None stays None)"""
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype)
        assert a.shape == shape, (a.shape, shape)
        return DeviceArray.from_numpy(a, self.device) if a.size else DeviceArray(1, dtype, self.device)

    def gae(self, reward, done, trunc, value, last_value, final_value=None, gamma=0.99, lam=0.95):
        """host-array form of gae_device: -> (adv [K, n], ret [K, n])"""
        K, n = np.shape(reward)[0], self.n
        r, v, fv = (self._dev(x, np.float32, (K, n)) for x in (reward, value, final_value))
        d, u = (self._dev(None if x is None else np.asarray(x) != 0, np.uint8, (K, n)) for x in (done, trunc))
        lv = self._dev(last_value, np.float32, (n,))
        adv, ret = DeviceArray((K, max(n, 1)), np.float32, self.device), DeviceArray((K, max(n, 1)), np.float32, self.device)
        self.gae_device(K, r, d, u, v, lv, fv, gamma, lam, adv, ret)
        self.sync()
        return tuple(x.numpy().reshape(-1)[: K * n].reshape(K, n) for x in (adv, ret))

    def pack_critic(self, weights):
        """nn.Linear-layout critic weights, (w1 [H1, D], b1 [H1], w2 [1, H1], b2 [1]) or (w1, b1, w2 [H2, H1], b2 [H2], w3 [1, H2], b3 [1]) -> (critic, H1, H2):
        the float32 words mgym_value_mlp reads, H2 = 0 for one hidden layer.  Shapes are checked against the family (PolicyShapeError); the widths by the engine."""
        D = self.obs_dim
        ws = [np.asarray(x, np.float32) for x in weights]
        if len(ws) not in (4, 6):
            raise PolicyShapeError(L.ERR_BAD_ARG, f"a critic is (w1, b1, w2, b2) or (w1, b1, w2, b2, w3, b3); got {len(ws)} arrays")
        H1 = ws[0].shape[0] if ws[0].ndim == 2 else -1
        H2 = (ws[2].shape[0] if ws[2].ndim == 2 else -1) if len(ws) == 6 else 0
        want = [(H1, D), (H1,), (1, H1), (1,)] if len(ws) == 4 else [(H1, D), (H1,), (H2, H1), (H2,), (1, H2), (1,)]
        if [w.shape for w in ws] != want:
            raise PolicyShapeError(L.ERR_BAD_ARG, f"{KIND_NAMES[self.kind]} takes a critic of shapes {want} (H1, H2 free); got {[w.shape for w in ws]}")
        return np.concatenate([w.ravel() for w in ws]).astype(np.float32), H1, H2

    def value_mlp_device(self, critic, hidden1, hidden2, activation, K, obs_first, obs, final_obs=None, done=None, trunc=None, value_out=None, last_value_out=None,
                         final_value_out=None):
        """mgym_value_mlp on device buffers (pointers, DeviceArrays or tensors): `critic` = the packed host floats of pack_critic (or None, which the engine
        rejects), hidden2 = 0 for one hidden layer; obs_first [D, n], obs [K, D, n], final_obs [K, D, n] or None, done / trunc uint8 [K, n] or None; value_out
        [K, n], last_value_out [n], final_value_out [K, n] or None — written only where trunc && !done, final_obs read only there.  The three outputs are
        gae_device's value, last_value and final_value.  On the env's stream, nothing synchronised.  A critic of the wrong length raises PolicyShapeError."""
        act = _named(_ACTIVATIONS, activation, _ACT_WORDING)
        h1, h2 = int(hidden1), int(hidden2)
        pol = None if critic is None else _policy_floats(critic, _mlp_floats(self.obs_dim, 1, h1, h2), f"hidden1 = {h1}, hidden2 = {h2}")
        _check(self._lib.mgym_value_mlp(self._h, _fptr(pol), h1, h2, act, int(K), _ptr(obs_first), _ptr(obs), _ptr(final_obs), _ptr(done), _ptr(trunc),
                                        _ptr(value_out), _ptr(last_value_out), _ptr(final_value_out)))

    def value_mlp(self, weights, obs_first, obs, final_obs=None, done=None, trunc=None, activation="relu"):
        """host-array form of value_mlp_device: weights as pack_critic takes them, obs_first [D, n], obs [K, D, n], final_obs [K, D, n] or None with done /
        trunc [K, n] -> (value [K, n], last_value [n], final_value [K, n] or None); final_value is 0 where the call does not write it"""
        critic, H1, H2 = self.pack_critic(weights)
        K, D, n = np.shape(obs)[0], self.obs_dim, self.n
        of, ob, fo = self._dev(obs_first, np.float32, (D, n)), self._dev(obs, np.float32, (K, D, n)), self._dev(final_obs, np.float32, (K, D, n))
        d, u = (self._dev(None if x is None else np.asarray(x) != 0, np.uint8, (K, n)) for x in (done, trunc))
        val, last = DeviceArray((K, max(n, 1)), np.float32, self.device), DeviceArray((max(n, 1),), np.float32, self.device)
        fv = None if fo is None else self._dev(np.zeros((K, n), np.float32), np.float32, (K, n))
        self.value_mlp_device(critic, H1, H2, activation, K, of, ob, fo, d, u, val, last, fv)
        self.sync()
        return (val.numpy().reshape(-1)[: K * n].reshape(K, n), last.numpy().reshape(-1)[:n], None if fv is None else fv.numpy().reshape(-1)[: K * n].reshape(K, n))

    def logprob_mlp_device(self, policy, hidden1, hidden2, activation, head, sigma, K, obs_first, obs, actions, logp_out):
        """mgym_logprob_mlp on device buffers (pointers, DeviceArrays or tensors): `policy` = the packed host floats of pack_mlp (hidden2 = 0) or pack_mlp2 (or
        None, which the engine rejects); head "sample" (the discrete families) or "gauss" (MountainCarContinuous, Pendulum; sigma a positive normal float, ignored
        by "sample"); obs_first [D, n], obs [K, D, n] and actions [K, n] (uint32 or float32 words) are a rollout's buffers, logp_out [K, n] receives the
        log-probability of each action under the distribution the rollout drew from.  On the env's stream, nothing synchronised.  A policy of the wrong length
        raises PolicyShapeError."""
        act = _named(_ACTIVATIONS, activation, _ACT_WORDING)
        hd = _named(_HEADS, head, _DENSITY_HEAD_WORDING)
        h1, h2 = int(hidden1), int(hidden2)
        pol = None if policy is None else _policy_floats(policy, _mlp_floats(*self.mlp_dims(), h1, h2), f"hidden1 = {h1}, hidden2 = {h2}")
        _check(self._lib.mgym_logprob_mlp(self._h, _fptr(pol), h1, h2, act, hd, float(sigma), int(K), _ptr(obs_first), _ptr(obs), _ptr(actions), _ptr(logp_out)))

    def logprob_mlp(self, weights, obs_first, obs, actions, activation="relu", head=None, sigma=0.0):
        """host-array form of logprob_mlp_device: weights (w1, b1, w2, b2) or (w1, b1, w2, b2, w3, b3) as pack_mlp / pack_mlp2 take them, obs_first [D, n],
        obs [K, D, n], actions [K, n] (this family's action dtype) -> logp [K, n] float32.  head: None takes the family's ("gauss" for a continuous one)."""
        if len(weights) not in (4, 6):
            raise PolicyShapeError(L.ERR_BAD_ARG, f"a policy is (w1, b1, w2, b2) or (w1, b1, w2, b2, w3, b3); got {len(weights)} arrays")
        policy, H1, H2 = (*self.pack_mlp(*weights), 0) if len(weights) == 4 else self.pack_mlp2(*weights)
        if head is None:
            head = self._family_head()
        K, D, n = np.shape(obs)[0], self.obs_dim, self.n
        of, ob = self._dev(obs_first, np.float32, (D, n)), self._dev(obs, np.float32, (K, D, n))
        ac = self._dev(actions, self.action_dtype, (K, n))
        out = DeviceArray((K, max(n, 1)), np.float32, self.device)
        self.logprob_mlp_device(policy, H1, H2, activation, head, sigma, K, of, ob, ac, out)
        self.sync()
        return out.numpy().reshape(-1)[: K * n].reshape(K, n)

    def grad_workspace_bytes(self, hidden):
        """(min_bytes, best_bytes) of the workspace of ppo_grad_mlp_device / value_grad_mlp_device at this hidden width (mgym_grad_workspace_bytes): one slab of
        partial sums, and the most a launch uses"""
        return self._grad_workspace(hidden)

    def grad_workspace_bytes2(self, hidden1, hidden2):
        """(min_bytes, best_bytes) of the workspace of ppo_grad_mlp2_device / value_grad_mlp2_device at these widths (mgym_grad_workspace_bytes2): one slab of
        partial sums, and the most a launch uses"""
        return self._grad_workspace(hidden1, hidden2)

    def _grad_workspace(self, *widths):
        """the workspace query of the gradient calls with as many hidden layers as there are widths"""
        query = self._lib.mgym_grad_workspace_bytes if len(widths) == 1 else self._lib.mgym_grad_workspace_bytes2
        lo, hi = C.c_size_t(), C.c_size_t()
        _check(query(self.kind, *(int(w) for w in widths), C.byref(lo), C.byref(hi)))
        return int(lo.value), int(hi.value)

    def _mlp2_grad_floats(self, weights, A, h1, h2):
        """the contiguous float32 words of a two-layer gradient call (None: NULL); the length is checked where the widths are ones the engine takes"""
        want = _mlp_floats(self.obs_dim, A, h1, h2) if h2 >= 1 else None
        return None if weights is None else _policy_floats(weights, want, f"hidden1 = {h1}, hidden2 = {h2}")

    def _ppo_grad_device(self, policy, widths, activation, head, sigma, K, env_first, env_count, obs_first, obs, actions, logp_old, adv, clip, ent_coef, workspace,
                         workspace_bytes, grad_out, stats_out):
        """the actor's gradient call of either depth, widths = (hidden,) or (hidden1, hidden2): each depth's entry point, and its checks in its order"""
        if len(widths) == 1:
            pol, act = self._mlp_args(policy, widths[0], activation)
            hd = _named(_HEADS, head, _DENSITY_HEAD_WORDING)
            call, widths = self._lib.mgym_ppo_grad_mlp, (int(widths[0]),)
        else:
            act = _named(_ACTIVATIONS, activation, _ACT_WORDING)
            hd = _named(_HEADS, head, _DENSITY_HEAD_WORDING)
            call, widths = self._lib.mgym_ppo_grad_mlp2, (int(widths[0]), int(widths[1]))
            pol = self._mlp2_grad_floats(policy, self.mlp_dims()[1], *widths)
        _check(call(self._h, _fptr(pol), *widths, act, hd, float(sigma), int(K), int(env_first), int(env_count), _ptr(obs_first), _ptr(obs), _ptr(actions),
                    _ptr(logp_old), _ptr(adv), float(clip), float(ent_coef), _ptr(workspace), int(workspace_bytes), _ptr(grad_out), _ptr(stats_out)))

    def _value_grad_device(self, critic, widths, activation, K, env_first, env_count, obs_first, obs, ret, workspace, workspace_bytes, grad_out, stats_out):
        """the critic's gradient call of either depth, as _ppo_grad_device"""
        act = _named(_ACTIVATIONS, activation, _ACT_WORDING)
        if len(widths) == 1:
            h = int(widths[0])
            cr = None if critic is None else _policy_floats(critic, _mlp_floats(self.obs_dim, 1, h), f"hidden = {widths[0]}")
            call, widths = self._lib.mgym_value_grad_mlp, (h,)
        else:
            call, widths = self._lib.mgym_value_grad_mlp2, (int(widths[0]), int(widths[1]))
            cr = self._mlp2_grad_floats(critic, 1, *widths)
        _check(call(self._h, _fptr(cr), *widths, act, int(K), int(env_first), int(env_count), _ptr(obs_first), _ptr(obs), _ptr(ret), _ptr(workspace),
                    int(workspace_bytes), _ptr(grad_out), _ptr(stats_out)))

    def ppo_grad_mlp_device(self, policy, hidden, activation, head, sigma, K, env_first, env_count, obs_first, obs, actions, logp_old, adv, clip, ent_coef,
                            workspace, workspace_bytes, grad_out, stats_out):
        """mgym_ppo_grad_mlp on device buffers (pointers, DeviceArrays or tensors): PPO's clipped loss and the actor's gradient over the env-steps of environments
        env_first .. env_first + env_count - 1 of a K-step rollout.  `policy` = the packed host floats of pack_mlp; obs_first, obs, actions as logprob_mlp_device
        takes them, logp_old [K, n] its output, adv [K, n] gae_device's; workspace: 16-byte aligned, workspace_bytes of it (grad_workspace_bytes); grad_out
        receives H (D + 1) + A (H + 1) + 1 floats (dW1, db1, dW2, db2 in nn.Linear order, d / d log sigma), stats_out 8.  On the env's stream, nothing
        synchronised, nothing allocated."""
        self._ppo_grad_device(policy, (hidden,), activation, head, sigma, K, env_first, env_count, obs_first, obs, actions, logp_old, adv, clip, ent_coef, workspace,
                              workspace_bytes, grad_out, stats_out)

    def value_grad_mlp_device(self, critic, hidden, activation, K, env_first, env_count, obs_first, obs, ret, workspace, workspace_bytes, grad_out, stats_out):
        """mgym_value_grad_mlp on device buffers: the loss 1/2 mean((V - ret)^2) of a one-hidden-layer critic (pack_critic's floats) and its gradient over the same
        range; grad_out receives H (D + 1) + (H + 1) + 1 floats (the last +0), stats_out 8."""
        self._value_grad_device(critic, (hidden,), activation, K, env_first, env_count, obs_first, obs, ret, workspace, workspace_bytes, grad_out, stats_out)

    def ppo_grad_mlp2_device(self, policy, hidden1, hidden2, activation, head, sigma, K, env_first, env_count, obs_first, obs, actions, logp_old, adv, clip,
                             ent_coef, workspace, workspace_bytes, grad_out, stats_out):
        """mgym_ppo_grad_mlp2 on device buffers: ppo_grad_mlp_device for the two-hidden-layer actor of pack_mlp2.  workspace_bytes of grad_workspace_bytes2;
        grad_out receives H1 (D + 1) + H2 (H1 + 1) + A (H2 + 1) + 1 floats (dW1, db1, dW2, db2, dW3, db3 in nn.Linear order, d / d log sigma), stats_out 8.
        On the env's stream, nothing synchronised, nothing allocated."""
        self._ppo_grad_device(policy, (hidden1, hidden2), activation, head, sigma, K, env_first, env_count, obs_first, obs, actions, logp_old, adv, clip, ent_coef,
                              workspace, workspace_bytes, grad_out, stats_out)

    def value_grad_mlp2_device(self, critic, hidden1, hidden2, activation, K, env_first, env_count, obs_first, obs, ret, workspace, workspace_bytes, grad_out,
                               stats_out):
        """mgym_value_grad_mlp2 on device buffers: value_grad_mlp_device for a two-hidden-layer critic (pack_critic's floats); grad_out receives
        H1 (D + 1) + H2 (H1 + 1) + (H2 + 1) + 1 floats (the last +0), stats_out 8."""
        self._value_grad_device(critic, (hidden1, hidden2), activation, K, env_first, env_count, obs_first, obs, ret, workspace, workspace_bytes, grad_out, stats_out)

    def _grad_host(self, A, widths, env_slice, workspace_bytes, call):
        """the workspace and the outputs of a host-array gradient call -> (grad [P + 1], stats [8])"""
        first, count = (0, self.n) if env_slice is None else env_slice
        lo, hi = self._grad_workspace(*widths)
        nbytes = hi if workspace_bytes is None else int(workspace_bytes)
        ws = DeviceArray(max(nbytes, lo) // 8, np.float64, self.device)
        grad, stats = DeviceArray(_mlp_floats(self.obs_dim, A, *widths) + 1, np.float32, self.device), DeviceArray(8, np.float32, self.device)
        call(first, count, ws, nbytes, grad, stats)
        self.sync()
        return grad.numpy().copy(), stats.numpy().copy()

    def _ppo_grad_host(self, policy, widths, obs_first, obs, actions, logp_old, adv, activation, head, sigma, clip, ent_coef, env_slice, workspace_bytes):
        """the host-array form of _ppo_grad_device on packed weights: the inputs staged on the device"""
        if head is None:
            head = self._family_head()
        K, D, n = np.shape(obs)[0], self.obs_dim, self.n
        of, ob = self._dev(obs_first, np.float32, (D, n)), self._dev(obs, np.float32, (K, D, n))
        ac, lp, ad = self._dev(actions, self.action_dtype, (K, n)), self._dev(logp_old, np.float32, (K, n)), self._dev(adv, np.float32, (K, n))
        return self._grad_host(self.mlp_dims()[1], widths, env_slice, workspace_bytes, lambda first, count, *out: self._ppo_grad_device(
            policy, widths, activation, head, sigma, K, first, count, of, ob, ac, lp, ad, clip, ent_coef, *out))

    def _value_grad_host(self, critic, widths, obs_first, obs, ret, activation, env_slice, workspace_bytes):
        """the host-array form of _value_grad_device on packed weights"""
        K, D, n = np.shape(obs)[0], self.obs_dim, self.n
        of, ob, rt = self._dev(obs_first, np.float32, (D, n)), self._dev(obs, np.float32, (K, D, n)), self._dev(ret, np.float32, (K, n))
        return self._grad_host(1, widths, env_slice, workspace_bytes, lambda first, count, *out: self._value_grad_device(
            critic, widths, activation, K, first, count, of, ob, rt, *out))

    def ppo_grad_mlp(self, weights, obs_first, obs, actions, logp_old, adv, activation="relu", head=None, sigma=0.0, clip=0.2, ent_coef=0.0, env_slice=None,
                     workspace_bytes=None):
        """host-array form of ppo_grad_mlp_device: weights (w1, b1, w2, b2), obs_first [D, n], obs [K, D, n], actions, logp_old and adv [K, n] -> (grad [P + 1]
        float32, stats [8] float32).  head: None takes the family's; env_slice: (first, count), None the full range; workspace_bytes: None takes best_bytes."""
        policy, *widths = self.pack_mlp(*weights)
        return self._ppo_grad_host(policy, widths, obs_first, obs, actions, logp_old, adv, activation, head, sigma, clip, ent_coef, env_slice, workspace_bytes)

    def ppo_grad_mlp2(self, weights, obs_first, obs, actions, logp_old, adv, activation="relu", head=None, sigma=0.0, clip=0.2, ent_coef=0.0, env_slice=None,
                      workspace_bytes=None):
        """host-array form of ppo_grad_mlp2_device: weights (w1, b1, w2, b2, w3, b3), the other arguments as ppo_grad_mlp -> (grad [P2 + 1] float32,
        stats [8] float32)"""
        policy, *widths = self.pack_mlp2(*weights)
        return self._ppo_grad_host(policy, widths, obs_first, obs, actions, logp_old, adv, activation, head, sigma, clip, ent_coef, env_slice, workspace_bytes)

    def value_grad_mlp(self, weights, obs_first, obs, ret, activation="relu", env_slice=None, workspace_bytes=None):
        """host-array form of value_grad_mlp_device: a one-hidden-layer critic (w1, b1, w2 [1, H], b2 [1]) -> (grad [P + 1] float32, stats [8] float32)"""
        critic, H, H2 = self.pack_critic(weights)
        if H2:
            raise PolicyShapeError(L.ERR_BAD_ARG, "value_grad_mlp takes a critic with one hidden layer")
        return self._value_grad_host(critic, (H,), obs_first, obs, ret, activation, env_slice, workspace_bytes)

    def value_grad_mlp2(self, weights, obs_first, obs, ret, activation="relu", env_slice=None, workspace_bytes=None):
        """host-array form of value_grad_mlp2_device: a two-hidden-layer critic (w1, b1, w2, b2, w3 [1, H2], b3 [1]) -> (grad [P2 + 1] float32, stats [8] float32)"""
        critic, H1, H2 = self.pack_critic(weights)
        if not H2:
            raise PolicyShapeError(L.ERR_BAD_ARG, "value_grad_mlp2 takes a critic with two hidden layers")
        return self._value_grad_host(critic, (H1, H2), obs_first, obs, ret, activation, env_slice, workspace_bytes)

    def episode_returns(self, reward, done, trunc, ep_return=None, ep_length=None):
        """host-array form of episode_returns_device: the carry in (None: zeros) -> (return_out [K, n] float32, length_out [K, n] uint32, both 0 where no
        episode ended, and the carry out: ep_return [n], ep_length [n])"""
        K, n = np.shape(reward)[0], self.n
        r = self._dev(reward, np.float32, (K, n))
        d, u = (self._dev(None if x is None else np.asarray(x) != 0, np.uint8, (K, n)) for x in (done, trunc))
        acc = self._dev(np.zeros(n, np.float32) if ep_return is None else ep_return, np.float32, (n,))
        length = self._dev(np.zeros(n, np.uint32) if ep_length is None else ep_length, np.uint32, (n,))
        ret, ln = self._dev(np.zeros((K, n), np.float32), np.float32, (K, n)), self._dev(np.zeros((K, n), np.uint32), np.uint32, (K, n))
        self.episode_returns_device(K, r, d, u, acc, length, ret, ln)
        self.sync()
        return (ret.numpy().reshape(-1)[: K * n].reshape(K, n), ln.numpy().reshape(-1)[: K * n].reshape(K, n), acc.numpy()[:n], length.numpy()[:n])

    def episode_count(self):
        """env-steps of this handle that returned done or truncated since creation (mgym_episode_count; synchronises)"""
        c = C.c_uint64()
        _check(self._lib.mgym_episode_count(self._h, C.byref(c)))
        return c.value

    def _coerce_actions(self, actions):
        """Discrete envs take integer actions only (reference: `action_space.contains(&action)` needs a u32 tensor,
        cartpole.rs:252,377): floats and bools are rejected instead of being truncated; negative integers become
        out-of-range u32 values and fail on the device like any invalid action."""
        a = np.asarray(actions)
        if not self.action_is_float and a.dtype.kind not in "iu":
            raise InvalidActionError(L.ERR_INVALID_ACTION, f"discrete actions must be integers, got dtype {a.dtype}")
        return np.ascontiguousarray(a, self.action_dtype)

    def rollout(self, actions):
        """K fused steps on host arrays: actions [K, n] -> (obs [K, obs_dim, n], reward [K, n], done, trunc)."""
        a = self._coerce_actions(actions)
        K = a.shape[0]
        assert a.shape == (K, self.n)
        da = DeviceArray.from_numpy(a, self.device) if a.size else DeviceArray(1, self.action_dtype, self.device)
        return self._rollout_host(K, lambda *out: self.rollout_device(da, K, *out), None)

    def observation_device(self):
        p, stride = C.c_void_p(), C.c_uint64()
        _check(self._lib.mgym_observation(self._h, C.byref(p), C.byref(stride)))
        return p.value, stride.value

    def timer_start(self):
        _check(self._lib.mgym_timer_start(self._h))

    def timer_stop(self):
        ms = C.c_float()
        _check(self._lib.mgym_timer_stop(self._h, C.byref(ms)))
        return ms.value

    def graph_capture(self, fn):
        """Capture the launches fn() issues on this env's stream into a hipGraphExec."""
        _check(self._lib.mgym_graph_begin(self._h))
        try:
            fn()
        finally:
            g = C.c_void_p()
            st = self._lib.mgym_graph_end(self._h, C.byref(g))
        _check(st)
        return g

    def graph_launch(self, g):
        _check(self._lib.mgym_graph_launch(self._h, g))

    def graph_destroy(self, g):
        _check(self._lib.mgym_graph_destroy(g))

    # ---- host-array convenience path (tests) ----------------------------------------
    def _buffers(self):
        if self._bufs is None:
            n = max(self.n, 1)
            self._bufs = dict(act=DeviceArray(n, self.action_dtype, self.device),
                              obs=DeviceArray((self.obs_dim, n), np.float32, self.device),
                              rew=DeviceArray(n, np.float32, self.device), done=DeviceArray(n, np.uint8, self.device),
                              trunc=DeviceArray(n, np.uint8, self.device), mask=DeviceArray(n, np.uint8, self.device))
        return self._bufs

    def _host(self, key, shape):
        return self._bufs[key].numpy().reshape(-1)[: int(np.prod(shape))].reshape(shape)

    def reset(self, mask=None):
        b = self._buffers()
        if mask is not None:
            m = np.ascontiguousarray(mask, np.uint8)
            assert m.shape == (self.n,)
            if self.n:
                b["mask"].copy_from(m)
            self.reset_device(b["mask"], b["obs"])
        else:
            self.reset_device(None, b["obs"])
        self.sync()
        return self._host("obs", (self.obs_dim, self.n))

    def reset_deterministic(self):
        """Testable::reset_deterministic of the reference's test modules, on every env."""
        b = self._buffers()
        _check(self._lib.mgym_reset_deterministic(self._h, b["obs"].ptr))
        self.sync()
        return self._host("obs", (self.obs_dim, self.n))

    def step(self, actions):
        b = self._buffers()
        a = self._coerce_actions(actions)
        assert a.shape == (self.n,), f"actions must be [{self.n}], got {a.shape}"
        if self.n:
            b["act"].copy_from(a)
        self.step_device(b["act"], b["obs"], b["rew"], b["done"], b["trunc"])
        self.sync()
        return (self._host("obs", (self.obs_dim, self.n)), self._host("rew", (self.n,)),
                self._host("done", (self.n,)), self._host("trunc", (self.n,)))

    def observation(self):
        """copy of the engine-owned observation (zero-copy pointer: observation_device())"""
        p, stride = self.observation_device()
        out = np.empty((self.obs_dim, self.n), np.float32)
        for k in range(self.obs_dim):
            if self.n:
                _check(self._lib.mgym_memcpy_d2h(self.device, out[k].ctypes.data, p + 4 * k * stride, 4 * self.n))
        return out

    def observation_aos(self):
        """row-major [n, obs_dim] copy of the current observation (mgym_observation_aos)"""
        d = DeviceArray((max(self.n, 1), self.obs_dim), np.float32, self.device)
        _check(self._lib.mgym_observation_aos(self._h, d.ptr))
        self.sync()
        return d.numpy()[: self.n]

    @property
    def state_cols(self):
        return get_spec(self.kind).state_cols

    def get_state(self):
        cols = self.state_cols
        d = DeviceArray((cols, max(self.n, 1)), np.float32, self.device)
        _check(self._lib.mgym_get_state(self._h, d.ptr))
        self.sync()
        return d.numpy().reshape(-1)[: cols * self.n].reshape(cols, self.n)

    def set_state(self, blob):
        b = np.ascontiguousarray(blob, np.float32)
        assert b.shape == (self.state_cols, self.n)
        if self.n == 0:
            return
        d = DeviceArray.from_numpy(b, self.device)
        _check(self._lib.mgym_set_state(self._h, d.ptr))
        self.sync()

    def elapsed_steps_device(self, out):
        """mgym_get_elapsed_steps: caller-visible steps since each env's last reset into a device uint32[n] (on the env's stream)"""
        _check(self._lib.mgym_get_elapsed_steps(self._h, _ptr(out)))

    def set_elapsed_steps_device(self, src):
        _check(self._lib.mgym_set_elapsed_steps(self._h, _ptr(src)))

    def elapsed_steps(self):
        d = DeviceArray(max(self.n, 1), np.uint32, self.device)
        self.elapsed_steps_device(d)
        self.sync()
        return d.numpy()[: self.n]

    def set_elapsed_steps(self, elapsed):
        a = np.ascontiguousarray(elapsed, np.uint32)
        assert a.shape == (self.n,)
        if self.n == 0:
            return
        d = DeviceArray.from_numpy(a, self.device)
        self.set_elapsed_steps_device(d)
        self.sync()

    def set_dispersion(self, disp):
        if disp is None:
            self._disp = None
            _check(self._lib.mgym_set_dispersion_override(self._h, None))
        else:
            a = np.ascontiguousarray(disp, np.float32)
            assert a.shape == (2, self.n)
            self._disp = DeviceArray.from_numpy(a, self.device)
            _check(self._lib.mgym_set_dispersion_override(self._h, self._disp.ptr))


class _SingleEnv:
    """n_envs = 1 view with the reference's scalar signature: reset() -> state, step(a) -> StepInfo."""

    KIND = None

    def __init__(self, device=0, seed=0, **builder_args):
        self.vec = VecEnv(self.KIND, 1, device=device, seed=seed, **builder_args)

    def reset(self):
        return self.vec.reset()[:, 0].copy()

    def step(self, action):
        a = np.asarray(action)
        if a.ndim != 0:  # cartpole.rs:392-403: a [1]-shaped action tensor is rejected (rank-0 required)
            raise InvalidActionError(L.ERR_INVALID_ACTION, f"action must be a scalar, got shape {a.shape}")
        obs, rew, done, trunc = self.vec.step(a.reshape(1))
        return StepInfo(obs[:, 0].copy(), float(rew[0]), bool(done[0]), bool(trunc[0]))

    def observation_space(self):
        s = get_spec(self.KIND)
        return np.array(s.obs_low[: s.obs_dim], np.float32), np.array(s.obs_high[: s.obs_dim], np.float32)

    def action_space(self):
        s = get_spec(self.KIND)
        return ("Box", s.action_low, s.action_high) if s.action_is_float else ("Discrete", s.n_actions)

    def close(self):
        self.vec.close()


class CartPoleV1(_SingleEnv):
    """cartpole.rs:13-357"""
    KIND = L.CARTPOLE

    def __init__(self, device=0, sutton_barto_reward=False, is_euler=True, seed=0):
        super().__init__(device, seed, sutton_barto_reward=sutton_barto_reward, is_euler=is_euler)


class MountainCarV0(_SingleEnv):
    """mountain_car.rs:10-339"""
    KIND = L.MOUNTAINCAR

    def __init__(self, device=0, goal_velocity=0.0, seed=0, max_episode_steps=0):
        super().__init__(device, seed, goal_velocity=goal_velocity, max_episode_steps=max_episode_steps)


class MountainCarContinuousV0(_SingleEnv):
    """Not in the reference (BASELINE config 3); gymnasium semantics, parity unpinned."""
    KIND = L.MOUNTAINCAR_CONT

    def __init__(self, device=0, goal_velocity=0.0, seed=0, max_episode_steps=0):
        super().__init__(device, seed, goal_velocity=goal_velocity, max_episode_steps=max_episode_steps)


class PendulumV1(_SingleEnv):
    """Not in the reference; gymnasium's Pendulum-v1 in f32 as include/mgym.h defines it, parity unpinned.  gymnasium registers it with
    max_episode_steps = 200; here the limit is off unless asked for, as for every family."""
    KIND = L.PENDULUM

    def __init__(self, device=0, g=10.0, seed=0, max_episode_steps=0):
        super().__init__(device, seed, gravity=g, max_episode_steps=max_episode_steps)


class AcrobotV1(_SingleEnv):
    """Not in the reference; gymnasium's Acrobot-v1 ("book" dynamics, RK4, no torque noise) in f32 as include/mgym.h defines it, parity unpinned.
    gymnasium registers it with max_episode_steps = 500; here the limit is off unless asked for, as for every family."""
    KIND = L.ACROBOT

    def __init__(self, device=0, seed=0, max_episode_steps=0):
        super().__init__(device, seed, max_episode_steps=max_episode_steps)


class LunarLanderV3(_SingleEnv):
    """lunar_lander.rs:232-1201"""
    KIND = L.LUNARLANDER

    def __init__(self, device=0, gravity=-10.0, enable_wind=False, wind_power=15.0, turbulence_power=1.5, seed=0,
                 max_episode_steps=0):
        super().__init__(device, seed, gravity=gravity, enable_wind=enable_wind, wind_power=wind_power,
                         turbulence_power=turbulence_power, max_episode_steps=max_episode_steps)
