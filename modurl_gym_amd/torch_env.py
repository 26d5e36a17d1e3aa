"""Torch-ROCm interop for the batched engine (the step either side of the path).

A policy network consumes observations and produces `action[n]`; this module lets that loop run
without leaving the GPU or the torch stream:

    env = TorchVecEnv(mg.CARTPOLE, 1 << 20, auto_reset=True)
    obs = env.reset()                                  # torch.float32 [obs_dim, n]  (SoA, like the engine)
    for _ in range(T):
        actions = policy(obs)                          # torch.int32 [n]  (float32 for MountainCarContinuous and Pendulum)
        obs, reward, done, truncated = env.step(actions)
    env.check()                                        # surfaces the sticky device status (invalid action ...)

Nothing here computes environment physics: tensors are handed to the C ABI by `data_ptr()` and
the engine's launches are enqueued on torch's *current* stream, so they order with the policy's
kernels exactly like torch ops do (no host synchronisation in `step`).  Torch is plumbing (device
memory + streams), as in bench.py.  The reference has no counterpart: its `Gym::step` takes and
returns host `candle` tensors one environment at a time (cartpole.rs:251-305).

Layouts: `obs_layout="soa"` returns `[obs_dim, n]` (the engine's native column layout, what
`mgym_step` writes); `"aos"` additionally runs `mgym_observation_aos` and returns `[n, obs_dim]`
row-major, the shape an `nn.Linear` policy wants.  `observation_view()` is a zero-copy tensor
over the engine-owned columns (`mgym_observation`): valid until the next call that advances them.
"""
import numpy as np

from . import envs as E


class _DeviceSpan:
    """Engine-owned device memory exposed through __cuda_array_interface__ (torch reads it under ROCm too)."""

    def __init__(self, ptr, shape, strides_bytes, owner):
        self._owner = owner  # keep the env alive while views exist
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f4", "data": (int(ptr), False),
                                         "version": 2, "strides": tuple(strides_bytes)}


class TorchVecEnv:
    """`VecEnv` whose inputs/outputs are torch tensors on the env's GPU, stream-ordered with torch."""

    def __init__(self, kind, n_envs, device=None, seed=0, env_id_base=0, auto_reset=True, obs_layout="soa", final_obs_steps=0, **params):
        import torch
        if not torch.cuda.is_available():
            raise E.MgymError(E.L.ERR_NO_DEVICE, "TorchVecEnv needs a GPU (there is no CPU path)")
        if obs_layout not in ("soa", "aos"):
            raise ValueError("obs_layout must be 'soa' or 'aos'")
        if int(final_obs_steps) > 0 and obs_layout != "soa":
            raise ValueError("final_obs_steps needs obs_layout='soa' (the final observations are delivered in the engine's column layout only)")
        self._torch = torch
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.env = E.VecEnv(kind, n_envs, device=self.device.index, seed=seed, env_id_base=env_id_base,
                            auto_reset=auto_reset, **params)
        self.kind, self.n, self.obs_dim = kind, self.env.n, self.env.obs_dim
        self.n_actions, self.action_is_float = self.env.n_actions, self.env.action_is_float
        self.obs_layout = obs_layout
        self._stream = None
        f32, u8 = torch.float32, torch.uint8
        self._obs = torch.empty((self.obs_dim, self.n), dtype=f32, device=self.device)
        self._obs_aos = torch.empty((self.n, self.obs_dim), dtype=f32, device=self.device) if obs_layout == "aos" else None
        self._rew = torch.empty(self.n, dtype=f32, device=self.device)
        self._done = torch.empty(self.n, dtype=u8, device=self.device)
        self._trunc = torch.empty(self.n, dtype=u8, device=self.device)
        # final observations of auto-reset episodes (mgym_set_final_obs_out): [final_obs_steps, obs_dim, n], written where done | truncated is set
        self.final_obs = None
        if int(final_obs_steps) > 0:
            self.final_obs = torch.zeros((int(final_obs_steps), self.obs_dim, self.n), dtype=f32, device=self.device)
            self.env.set_final_obs_out_device(self.final_obs, int(final_obs_steps))
        self._ep_return = self._ep_length = None   # the carry of episode_returns(), created by its first call
        self._grad_ws = {}   # the workspaces of the gradient calls, one per (hidden widths, stream), created by the first call that needs one

    # ---- plumbing -----------------------------------------------------------------------
    def _bind_stream(self):
        s = self._torch.cuda.current_stream(self.device).cuda_stream
        if s != self._stream:
            self.env.set_stream(s)
            self._stream = s

    def _actions(self, a, lead=()):
        torch = self._torch
        if not isinstance(a, torch.Tensor):
            raise TypeError("actions must be a torch tensor on the env's device")
        if a.device != self.device:
            raise ValueError(f"actions are on {a.device}, the env is on {self.device}")
        if tuple(a.shape) != tuple(lead) + (self.n,):
            raise ValueError(f"actions must have shape {tuple(lead) + (self.n,)}, got {tuple(a.shape)}")
        if self.action_is_float:
            if a.dtype != torch.float32:
                a = a.to(torch.float32)
        elif a.dtype not in (torch.int32, torch.uint32):
            if a.dtype.is_floating_point or a.dtype == torch.bool:
                raise TypeError(f"discrete actions must be an integer tensor, got {a.dtype}")
            a = a.to(torch.int32)  # one extra elementwise kernel; pass int32 to avoid it
        return a.contiguous()

    def _obs_out(self):
        if self._obs_aos is None:
            return self._obs
        E._check(self.env._lib.mgym_observation_aos(self.env._h, self._obs_aos.data_ptr()))
        return self._obs_aos

    def _flags(self):
        return self._done.view(self._torch.bool), self._trunc.view(self._torch.bool)

    # ---- the Gym-shaped surface ---------------------------------------------------------
    def reset(self, mask=None):
        """Reset all envs, or those with mask != 0 (torch.uint8/bool [n]); returns the observation tensor."""
        self._bind_stream()
        if mask is not None:
            torch = self._torch
            if mask.dtype == torch.bool:
                mask = mask.view(torch.uint8)
            if mask.dtype != torch.uint8 or tuple(mask.shape) != (self.n,) or mask.device != self.device:
                raise ValueError("mask must be a uint8/bool tensor of shape [n] on the env's device")
            mask = mask.contiguous()
        if self._ep_return is not None:   # (episode_returns() has been used: the episodes that are reset start from nothing)
            if mask is None:
                self._ep_return.zero_(), self._ep_length.zero_()
            else:
                self._ep_return.masked_fill_(mask != 0, 0.0), self._ep_length.masked_fill_(mask != 0, 0)
        self.env.reset_device(mask, self._obs)
        return self._obs_out()

    def step(self, actions, check=False):
        """One step of every env.  Returns (obs, reward, done, truncated); the tensors are reused by the
        next call (clone what must outlive it).  check=True synchronises and raises on invalid actions."""
        self._bind_stream()
        a = self._actions(actions)
        self.env.step_device(a, self._obs, self._rew, self._done, self._trunc)
        if check:
            self.check()
        d, t = self._flags()
        return self._obs_out(), self._rew, d, t

    def rollout(self, actions):
        """K fused steps for a caller-supplied action tensor [K, n] (mgym_rollout): returns
        (obs [K, obs_dim, n], reward [K, n], done [K, n], truncated [K, n]) as fresh tensors."""
        self._bind_stream()
        K = int(actions.shape[0])
        a = self._actions(actions, (K,))
        obs, rew, done, trunc = self._policy_outputs(K, actions=False)
        self.env.rollout_device(a, K, obs, rew, done, trunc)
        return obs, rew, done.view(self._torch.bool), trunc.view(self._torch.bool)

    def _policy_outputs(self, K, actions=True):
        """fresh [K, ..] tensors for a K-step call to fill: (actions if asked for,) obs, reward, done, truncated — the flags as uint8"""
        torch = self._torch

        def new(dtype, *mid):
            return torch.empty((K, *mid, self.n), dtype=dtype, device=self.device)

        out = new(torch.float32, self.obs_dim), new(torch.float32), new(torch.uint8), new(torch.uint8)
        return (new(torch.float32 if self.action_is_float else torch.int32),) + out if actions else out

    def _rollout_policy(self, weights, K, call):
        """The tensor form of every policy call: on torch's current stream, the weights as host arrays (they are read on the host, during the call), fresh
        [K, ..] outputs, call(host weights, K, outputs) — a VecEnv.*_device call — -> (actions, obs, reward, done, truncated), the flags as bool."""
        torch = self._torch
        self._bind_stream()
        host = [x.detach().to("cpu", torch.float32).numpy() if isinstance(x, torch.Tensor) else x for x in weights]
        K = int(K)
        act, obs, rew, done, trunc = out = self._policy_outputs(K)
        call(host, K, out)
        return act, obs, rew, done.view(torch.bool), trunc.view(torch.bool)

    def rollout_linear(self, policy, K):
        """K fused steps under the on-device linear policy (mgym_rollout_linear; `policy`: host floats or a tensor, the layout
        VecEnv.rollout_linear_device documents): returns (actions [K, n], obs [K, obs_dim, n], reward [K, n], done [K, n], truncated [K, n])
        as fresh tensors, stream-ordered on torch's current stream (actions int32, float32 for MountainCarContinuous and Pendulum)."""
        return self._rollout_policy((policy,), K, lambda host, K, out: self.env.rollout_linear_device(host[0], K, *out))

    def rollout_mlp(self, w1, b1, w2, b2, K, activation="relu"):
        """K fused steps under the on-device one-hidden-layer policy (mgym_rollout_mlp): w1 [H, D], b1 [H], w2 [A, H], b2 [A] are tensors (or arrays) in
        nn.Linear layout — `rollout_mlp(net[0].weight, net[0].bias, net[2].weight, net[2].bias, K)` for nn.Sequential(Linear, ReLU / Tanh, Linear) — read on the
        host during the call; activation "relu", "tanh" or "tanh_fast" (the cheap tanh of include/mgym.h: what a collector wants).  Returns (actions, obs, reward, done, truncated) like rollout_linear."""
        return self._rollout_policy((w1, b1, w2, b2), K, lambda host, K, out: self.env.rollout_mlp_device(*self.env.pack_mlp(*host), activation, K, *out))

    def rollout_mlp_sample(self, w1, b1, w2, b2, K, seed, call=0, activation="relu"):
        """rollout_mlp with the action drawn from the softmax of the scores (mgym_rollout_mlp_sample; the discrete families) — the collector of an on-policy
        trainer.  The draw is a pure function of (seed, call, global env id, step) and the scores: pass a new `call` for each call that is to draw afresh.
        Returns (actions, obs, reward, done, truncated) like rollout_mlp; logprob_mlp gives the log-probabilities of these actions over obs and actions."""
        return self._rollout_policy((w1, b1, w2, b2), K,
                                    lambda host, K, out: self.env.rollout_mlp_sample_device(*self.env.pack_mlp(*host), activation, seed, call, K, *out))

    def rollout_mlp_gauss(self, w1, b1, w2, b2, K, sigma, seed, call=0, activation="relu"):
        """rollout_mlp for MountainCarContinuous and Pendulum with the action drawn from a Gaussian around the score, a = mu + sigma * z with a
        state-independent `sigma` >= 0 (mgym_rollout_mlp_gauss) — the collector of a continuous-control on-policy trainer.  z is a pure function of (seed,
        call, global env id, step): pass a new `call` for each call that is to draw afresh.  Returns (actions, obs, reward, done, truncated) like rollout_mlp;
        the actions are float32 and not clamped (the step clamps): logprob_mlp over obs and these actions gives their log-probabilities."""
        return self._rollout_policy((w1, b1, w2, b2), K,
                                    lambda host, K, out: self.env.rollout_mlp_gauss_device(*self.env.pack_mlp(*host), activation, float(sigma), seed, call, K, *out))

    def rollout_mlp2(self, w1, b1, w2, b2, w3, b3, K, activation="relu", head="greedy", sigma=0.0, seed=0, call=0):
        """K fused steps under the on-device two-hidden-layer policy (mgym_rollout_mlp2): the six tensors (or arrays) of nn.Sequential(Linear(D, H1), act,
        Linear(H1, H2), act, Linear(H2, A)) in nn.Linear layout, read on the host during the call; activation "relu" or "tanh_fast"; head "greedy", "sample" (the
        discrete families: the draw of rollout_mlp_sample) or "gauss" (MountainCarContinuous, Pendulum: mu + sigma * z of rollout_mlp_gauss).  Pass a new `call`
        for each call that is to draw afresh.  Returns (actions, obs, reward, done, truncated) like rollout_mlp."""
        return self._rollout_policy((w1, b1, w2, b2, w3, b3), K,
                                    lambda host, K, out: self.env.rollout_mlp2_device(*self.env.pack_mlp2(*host), activation, head, float(sigma), seed, call, K, *out))

    def rollout_uniform(self, seed, K):
        """K fused steps under the on-device uniform random policy (mgym_rollout_uniform, include/mgym.h): returns (actions, obs, reward,
        done, truncated) like rollout_linear."""
        return self._rollout_policy((), K, lambda host, K, out: self.env.rollout_uniform_device(int(seed), K, *out))

    def bootstrap_obs(self, obs, done, truncated):
        """The observation a learner evaluates V on after each env-step of the last call: `obs` ([K, obs_dim, n], or [obs_dim, n] from step) with the final
        observation in the place of the reset one wherever the episode ended (needs final_obs_steps >= K at construction)."""
        if self.final_obs is None:
            raise ValueError("bootstrap_obs needs final_obs_steps > 0 at construction")
        fin = done | truncated
        if obs.dim() == 2:
            return self._torch.where(fin[None, :], self.final_obs[0], obs)
        return self._torch.where(fin[:, None, :], self.final_obs[: obs.shape[0]], obs)

    def _kn(self, x, dtype, name, lead):
        """x as a contiguous tensor of shape lead + (n,) and the given dtype on the env's device (bool flags are viewed as uint8); None stays None"""
        torch = self._torch
        if x is None:
            return None
        if x.dtype == torch.bool and dtype == torch.uint8:
            x = x.view(torch.uint8)
        if x.device != self.device or tuple(x.shape) != tuple(lead) + (self.n,):
            raise ValueError(f"{name} must have shape {tuple(lead) + (self.n,)} on {self.device}, got {tuple(x.shape)} on {x.device}")
        return x.to(dtype).contiguous()

    def gae(self, reward, done, truncated, value, last_value, final_value=None, gamma=0.99, lam=0.95):
        """Generalised advantage estimation over a rollout's outputs in one launch (mgym_gae, include/mgym.h, defined to the f32 word): reward / value [K, n],
        done / truncated [K, n] bool or uint8 (or None), last_value [n] = V(obs[-1]), final_value [K, n] = V(final_obs[:K]) or None (truncation then counts as
        termination); value[t] is V of the observation the policy acted on at step t.  final_value is read only where truncated & ~done, so the values of a
        final-observation buffer's unwritten words never matter.  Returns fresh (adv, ret) [K, n] tensors on torch's current stream."""
        torch = self._torch
        self._bind_stream()
        K = int(reward.shape[0])
        f32, u8 = torch.float32, torch.uint8
        r, v, fv = (self._kn(x, f32, nm, (K,)) for x, nm in ((reward, "reward"), (value, "value"), (final_value, "final_value")))
        d, u = self._kn(done, u8, "done", (K,)), self._kn(truncated, u8, "truncated", (K,))
        lv = self._kn(last_value, f32, "last_value", ())
        adv, ret = torch.empty((K, self.n), dtype=f32, device=self.device), torch.empty((K, self.n), dtype=f32, device=self.device)
        self.env.gae_device(K, r, d, u, v, lv, fv, gamma, lam, adv, ret)
        return adv, ret

    def value_mlp(self, weights, obs_first, obs, done=None, truncated=None, activation="relu"):
        """A critic's values over a rollout's buffers in one call (mgym_value_mlp, include/mgym.h), in place of three passes of a torch MLP.  weights: (w1, b1,
        w2, b2) or (w1, b1, w2, b2, w3, b3), tensors (or arrays) in nn.Linear layout with one output, as in rollout_mlp / rollout_mlp2, read on the host during
        the call; obs_first [obs_dim, n]: the observation held before the rollout's step 0 (clone it: reset() and step() reuse their tensor); obs [K, obs_dim, n]:
        the rollout's obs.  Returns (value [K, n], last_value [n], final_value): value[t] is V of the observation the policy acted on at step t, last_value is
        V(obs[-1]), and final_value [K, n] is V(final_obs[t]) where truncated & ~done and 0 elsewhere — or None unless the env was built with
        final_obs_steps >= K and `truncated` is given.  The three are shaped for gae().  Fresh tensors on torch's current stream."""
        torch = self._torch
        self._bind_stream()
        f32, u8 = torch.float32, torch.uint8
        host = [x.detach().to("cpu", f32).numpy() if isinstance(x, torch.Tensor) else x for x in weights]
        critic, h1, h2 = self.env.pack_critic(host)
        K = int(obs.shape[0])
        of, ob = self._kn(obs_first, f32, "obs_first", (self.obs_dim,)), self._kn(obs, f32, "obs", (K, self.obs_dim))
        value, last = torch.empty((K, self.n), dtype=f32, device=self.device), torch.empty(self.n, dtype=f32, device=self.device)
        fo = d = u = fv = None
        if self.final_obs is not None and self.final_obs.shape[0] >= K and truncated is not None:
            fo, fv = self.final_obs, torch.zeros((K, self.n), dtype=f32, device=self.device)
            d, u = self._kn(done, u8, "done", (K,)), self._kn(truncated, u8, "truncated", (K,))
        self.env.value_mlp_device(critic, h1, h2, activation, K, of, ob, fo, d, u, value, last, fv)
        return value, last, fv

    def logprob_mlp(self, weights, obs_first, obs, actions, activation="relu", head=None, sigma=0.0):
        """log pi(a | o) of every env-step of a rollout in one call (mgym_logprob_mlp, include/mgym.h): PPO's old log-probabilities under the distribution the
        rollout drew from, in its own arithmetic, in place of a torch forward pass of the actor.  weights: (w1, b1, w2, b2) or (w1, b1, w2, b2, w3, b3), the
        tensors (or arrays) given to rollout_mlp_sample / rollout_mlp_gauss / rollout_mlp2, read on the host during the call; obs_first [obs_dim, n]: the
        observation held before the rollout's step 0 (clone it: reset() and step() reuse their tensor); obs [K, obs_dim, n] and actions [K, n]: the rollout's
        (int32 for the discrete families, float32 and unclamped for the continuous ones).  head "sample" or "gauss" (None: the family's); sigma: the Gaussian
        head's, the one the rollout drew with.  Returns a fresh [K, n] float32 tensor on torch's current stream; no entropy (the learner's own pass has it)."""
        torch = self._torch
        self._bind_stream()
        host = [x.detach().to("cpu", torch.float32).numpy() if isinstance(x, torch.Tensor) else x for x in weights]
        if len(host) not in (4, 6):
            raise ValueError(f"a policy is (w1, b1, w2, b2) or (w1, b1, w2, b2, w3, b3); got {len(host)} arrays")
        policy, h1, h2 = (*self.env.pack_mlp(*host), 0) if len(host) == 4 else self.env.pack_mlp2(*host)
        if head is None:
            head = self.env._family_head()
        K = int(obs.shape[0])
        of, ob = self._kn(obs_first, torch.float32, "obs_first", (self.obs_dim,)), self._kn(obs, torch.float32, "obs", (K, self.obs_dim))
        ac = self._kn(actions, torch.float32 if self.action_is_float else torch.int32, "actions", (K,))
        logp = torch.empty((K, self.n), dtype=torch.float32, device=self.device)
        self.env.logprob_mlp_device(policy, h1, h2, activation, head, float(sigma), K, of, ob, ac, logp)
        return logp

    def _grad_buffers(self, widths, P):
        """the cached workspace of these hidden widths, (H,) or (H1, H2), on torch's current stream — best_bytes of mgym_grad_workspace_bytes /
        mgym_grad_workspace_bytes2, 16-byte aligned; one per stream, so that calls issued on two streams never share the slabs — and fresh outputs"""
        torch = self._torch
        key = (widths, self._stream)   # (_bind_stream has made the engine's stream torch's current one)
        if key not in self._grad_ws:
            self._grad_ws[key] = torch.empty(self.env._grad_workspace(*widths)[1] // 8, dtype=torch.float64, device=self.device)
        ws = self._grad_ws[key]
        return ws, ws.numel() * 8, torch.empty(P + 1, dtype=torch.float32, device=self.device), torch.empty(8, dtype=torch.float32, device=self.device)

    def _grad_views(self, grad, D, A, widths, log_sigma):
        """(dw, db) of every layer in nn.Linear order as views of grad — and the log-sigma word"""
        views, at = [], 0
        for rows, cols in zip((*widths, A), (D, *widths)):
            views += [grad[at: at + rows * cols].view(rows, cols), grad[at + rows * cols: at + rows * cols + rows]]
            at += rows * (cols + 1)
        return tuple(views) + ((grad[at:],) if log_sigma else ())

    def _ppo_grad(self, policy, widths, obs_first, obs, actions, logp_old, adv, activation, head, sigma, clip, ent_coef, env_slice):
        """ppo_grad_mlp / ppo_grad_mlp2 on packed weights"""
        torch = self._torch
        if head is None:
            head = self.env._family_head()
        K = int(obs.shape[0])
        D, A = self.env.mlp_dims()
        of, ob = self._kn(obs_first, torch.float32, "obs_first", (self.obs_dim,)), self._kn(obs, torch.float32, "obs", (K, self.obs_dim))
        ac = self._kn(actions, torch.float32 if self.action_is_float else torch.int32, "actions", (K,))
        lp, ad = self._kn(logp_old, torch.float32, "logp_old", (K,)), self._kn(adv, torch.float32, "adv", (K,))
        first, count = (0, self.n) if env_slice is None else env_slice
        ws, nbytes, grad, stats = self._grad_buffers(widths, E._mlp_floats(D, A, *widths))
        self.env._ppo_grad_device(policy, widths, activation, head, float(sigma), K, first, count, of, ob, ac, lp, ad, clip, ent_coef, ws, nbytes, grad, stats)
        return self._grad_views(grad, D, A, widths, head in ("gauss", E.L.HEAD_GAUSS)), stats

    def _value_grad(self, packed, widths, obs_first, obs, ret, activation, env_slice):
        """value_grad_mlp / value_grad_mlp2 on packed weights"""
        torch = self._torch
        K, D = int(obs.shape[0]), self.obs_dim
        of, ob = self._kn(obs_first, torch.float32, "obs_first", (D,)), self._kn(obs, torch.float32, "obs", (K, D))
        rt = self._kn(ret, torch.float32, "ret", (K,))
        first, count = (0, self.n) if env_slice is None else env_slice
        ws, nbytes, grad, stats = self._grad_buffers(widths, E._mlp_floats(D, 1, *widths))
        self.env._value_grad_device(packed, widths, activation, K, first, count, of, ob, rt, ws, nbytes, grad, stats)
        return self._grad_views(grad, D, 1, widths, False), stats

    def ppo_grad_mlp(self, weights, obs_first, obs, actions, logp_old, adv, activation="relu", head=None, sigma=0.0, clip=0.2, ent_coef=0.0, env_slice=None):
        """PPO's clipped loss and the actor's gradient in one call (mgym_ppo_grad_mlp, include/mgym.h) in place of a torch forward pass, the surrogate and
        autograd's backward pass.  weights: (w1, b1, w2, b2) of a one-hidden-layer actor, read on the host during the call; obs_first, obs, actions as
        logprob_mlp takes them; logp_old [K, n]: logprob_mlp's output under the behaviour policy; adv [K, n]: gae's (normalise it yourself if you do);
        env_slice = (first, count): the minibatch, the environments first .. first + count - 1 over all K steps (None: all of them).  Returns (grads, stats):
        grads = (dw1, db1, dw2, db2) as views of one tensor, shaped like the weights — and d / d log sigma [1] under the Gaussian head; stats [8] float32:
        policy loss, mean entropy, approximate KL, clipped fraction, mean ratio, the batch size, 0, 0.  Fresh tensors on torch's current stream; the workspace is
        cached per (hidden, stream) of this object, which lives on one device."""
        torch = self._torch
        self._bind_stream()
        host = [x.detach().to("cpu", torch.float32).numpy() if isinstance(x, torch.Tensor) else x for x in weights]
        policy, *widths = self.env.pack_mlp(*host)
        return self._ppo_grad(policy, tuple(widths), obs_first, obs, actions, logp_old, adv, activation, head, sigma, clip, ent_coef, env_slice)

    def value_grad_mlp(self, critic, obs_first, obs, ret, activation="relu", env_slice=None):
        """The loss 1/2 mean((V - ret)^2) of a one-hidden-layer critic (w1, b1, w2 [1, H], b2 [1]) and its gradient in one call (mgym_value_grad_mlp): ret
        [K, n] is gae's.  Returns (grads, stats): grads = (dw1, db1, dw2, db2) views shaped like the weights, stats [8] float32: the loss at [0], the batch size
        at [5].  env_slice as in ppo_grad_mlp."""
        torch = self._torch
        self._bind_stream()
        host = [x.detach().to("cpu", torch.float32).numpy() if isinstance(x, torch.Tensor) else x for x in critic]
        packed, H, H2 = self.env.pack_critic(host)
        if H2:
            raise ValueError("value_grad_mlp takes a critic with one hidden layer")
        return self._value_grad(packed, (H,), obs_first, obs, ret, activation, env_slice)

    def ppo_grad_mlp2(self, weights, obs_first, obs, actions, logp_old, adv, activation="relu", head=None, sigma=0.0, clip=0.2, ent_coef=0.0, env_slice=None):
        """ppo_grad_mlp for the two-hidden-layer actor (mgym_ppo_grad_mlp2): weights (w1, b1, w2, b2, w3, b3); activation "relu" or "tanh_fast".  Returns
        (grads, stats): grads = (dw1, db1, dw2, db2, dw3, db3) as views of one tensor, shaped like the weights — and d / d log sigma [1] under the Gaussian
        head; stats as ppo_grad_mlp's.  The workspace is cached per ((H1, H2), stream)."""
        torch = self._torch
        self._bind_stream()
        host = [x.detach().to("cpu", torch.float32).numpy() if isinstance(x, torch.Tensor) else x for x in weights]
        policy, *widths = self.env.pack_mlp2(*host)
        return self._ppo_grad(policy, tuple(widths), obs_first, obs, actions, logp_old, adv, activation, head, sigma, clip, ent_coef, env_slice)

    def value_grad_mlp2(self, critic, obs_first, obs, ret, activation="relu", env_slice=None):
        """value_grad_mlp for a two-hidden-layer critic (w1, b1, w2, b2, w3 [1, H2], b3 [1]) (mgym_value_grad_mlp2).  Returns (grads, stats): grads = (dw1, db1,
        dw2, db2, dw3, db3) views shaped like the weights, stats [8] float32."""
        torch = self._torch
        self._bind_stream()
        host = [x.detach().to("cpu", torch.float32).numpy() if isinstance(x, torch.Tensor) else x for x in critic]
        packed, H1, H2 = self.env.pack_critic(host)
        if not H2:
            raise ValueError("value_grad_mlp2 takes a critic with two hidden layers")
        return self._value_grad(packed, (H1, H2), obs_first, obs, ret, activation, env_slice)

    def episode_returns(self, reward, done, truncated):
        """The return and length of every episode that ended inside the rollout (mgym_episode_returns): (return_out float32 [K, n], length_out int32 [K, n]),
        fresh tensors that are 0 except where done | truncated — `length_out > 0` is that mask.  The running episodes' carry lives in this object, created
        zeroed by the first call, so episodes span calls; reset() zeroes it (reset(mask): where the mask is set)."""
        torch = self._torch
        self._bind_stream()
        K = int(reward.shape[0])
        r = self._kn(reward, torch.float32, "reward", (K,))
        d, u = self._kn(done, torch.uint8, "done", (K,)), self._kn(truncated, torch.uint8, "truncated", (K,))
        if self._ep_return is None:
            self._ep_return = torch.zeros(self.n, dtype=torch.float32, device=self.device)
            self._ep_length = torch.zeros(self.n, dtype=torch.int32, device=self.device)
        ret = torch.zeros((K, self.n), dtype=torch.float32, device=self.device)
        length = torch.zeros((K, self.n), dtype=torch.int32, device=self.device)
        self.env.episode_returns_device(K, r, d, u, self._ep_return, self._ep_length, ret, length)
        return ret, length

    def elapsed_steps(self):
        """Caller-visible steps since each env's last reset (mgym_get_elapsed_steps; the count of `max_episode_steps`, which is passed
        through `**params`): a fresh int32 [n] tensor, stream-ordered on torch's current stream."""
        self._bind_stream()
        out = self._torch.empty(self.n, dtype=self._torch.int32, device=self.device)
        self.env.elapsed_steps_device(out)
        return out

    def set_elapsed_steps(self, elapsed):
        """mgym_set_elapsed_steps from an int32 [n] tensor on the env's device (MountainCar clamps to 65535)."""
        self._bind_stream()
        torch = self._torch
        if elapsed.device != self.device or tuple(elapsed.shape) != (self.n,):
            raise ValueError("elapsed must be a tensor of shape [n] on the env's device")
        self.env.set_elapsed_steps_device(elapsed.to(torch.int32).contiguous())

    def observation_view(self):
        """Zero-copy [obs_dim, n] tensor over the engine-owned observation columns (column stride n_pad)."""
        ptr, stride = self.env.observation_device()
        span = _DeviceSpan(ptr, (self.obs_dim, self.n), (4 * stride, 4), self)
        return self._torch.as_tensor(span, device=self.device)

    def check(self):
        """hipStreamSynchronize + sticky device status (raises InvalidActionError / NotResetError)."""
        self.env.sync()

    def close(self):
        self.env.close()

    def state_numpy(self):
        return np.array(self.env.get_state())
