"""The device memory a GPU test hands to the engine, once: a slab between guard words that shows what a kernel did not write (Guarded), the refusal of a call's bad argument (bad_arg), the caller's
final-observation buffer on it (FinalBuf), the five buffers of a call (CallBuffers), the call of a named action source (policy_call) and the twin loop
that shows what a step produced before the fused reset (twin_steps).  tests/test_support.py checks the checkers on host memory.  No test here."""
import numpy as np
import pytest

import modurl_gym_amd as mg
from modurl_gym_amd import _lib
from words import bits, same

F = np.float32
FILL = 0x7FC0DEAD   # a NaN word no step produces


class Guarded:
    """`words` 32-bit words of device memory between two guards of four words each, everything filled with `fill`; mis = 1: 4 bytes off a 16-byte boundary"""

    def __init__(self, words, mis=0, host=None, fill=FILL, alloc=mg.DeviceArray):
        self.words, self.off, self.word = int(words), 4 + mis, fill   # (the allocation is 256-byte aligned)
        self.dev = alloc(self.words + 8 + mis, np.uint32)
        self.ptr = self.dev.ptr + 4 * self.off
        self.fill(host)

    def fill(self, host=None):
        """the fill word everywhere, then `host` (float32 or uint32, any shape of `words` elements) in the payload"""
        a = np.full(self.words + 8 + self.off - 4, self.word, np.uint32)
        if host is not None:
            h = np.ascontiguousarray(host)
            assert h.size == self.words and h.dtype.itemsize == 4
            a[self.off: self.off + self.words] = h.reshape(-1).view(np.uint32)
        self.dev.copy_from(a)
        self.initial = a

    def data_ptr(self):
        return self.ptr

    def payload(self, shape, dtype=np.uint32):
        return self.dev.numpy()[self.off: self.off + self.words].view(dtype).reshape(shape)

    def guards_hold(self):
        a = self.dev.numpy()
        return bool((a[: self.off] == self.word).all() and (a[self.off + self.words:] == self.word).all())

    def untouched(self):
        return bool(np.array_equal(self.dev.numpy(), self.initial))


def bad_arg(fn, name, *needles):
    """fn() is refused as a bad argument, in one message of entry point `name` that holds every needle"""
    with pytest.raises(mg.MgymError) as ei:
        fn()
    assert ei.value.status == _lib.ERR_BAD_ARG and str(ei.value).count(name + ":") == 1 and all(s in str(ei.value) for s in needles), str(ei.value)


class FinalBuf(Guarded):
    """the caller's [cap][obs_dim][n] buffer of mgym_set_final_obs_out"""

    def __init__(self, cap, obs_dim, n, mis=0, alloc=mg.DeviceArray):
        self.shape = (cap, obs_dim, n)
        super().__init__(cap * obs_dim * n, mis, alloc=alloc)

    def check(self, finals, finished, what, eq=same):
        """finals [T][obs_dim][n], finished [T][n], T <= cap: finished env-steps hold `finals` under eq, every other word the fill, and the guards hold"""
        got = self.payload(self.shape)
        mask = np.zeros(self.shape, bool)
        mask[: len(finished)] = np.asarray(finished, bool)[:, None, :]
        exp = np.zeros(self.shape, np.uint32)
        exp[: len(finals)] = bits(np.asarray(finals, F))
        assert self.guards_hold(), f"{what}: a guard word was written"
        assert eq(got[mask], exp[mask].view(F)), f"{what}: {int((got[mask] != exp[mask]).sum())} of {int(mask.sum())} final words differ from the reference's"
        assert np.all(got[~mask] == self.word), f"{what}: {int((got[~mask] != self.word).sum())} words outside the finished env-steps were written"


class CallBuffers:
    """the caller's buffers of a step or K-step call: actions [K][n], obs [K][obs_dim][n], reward, done and truncated [K][n], each 16 bytes longer than
    its payload.  mis: a byte offset off the 16-byte alignment per buffer (an int: the reward's); with_obs = False: no observation buffer, a null pointer"""

    def __init__(self, n, obs_dim, action_dtype, K=1, mis=(0, 0, 0, 0, 0), with_obs=True, alloc=mg.DeviceArray):
        mis = (0, 0, mis, 0, 0) if isinstance(mis, int) else tuple(mis)
        self.n, self.K, self.mis = n, K, mis
        self.dtypes = [np.dtype(d) for d in (action_dtype, F, F, np.uint8, np.uint8)]
        self.shapes = [(K, n), (K, obs_dim, n), (K, n), (K, n), (K, n)]
        self.nbytes = [int(np.prod(s)) * d.itemsize for s, d in zip(self.shapes, self.dtypes)]
        self.arr = [alloc(b + 16, np.uint8) if with_obs or i != 1 else None for i, b in enumerate(self.nbytes)]
        self.ptr = [None if a is None else a.ptr + m for a, m in zip(self.arr, mis)]
        assert all(p is None or (p % 16 != 0) == (m != 0) for p, m in zip(self.ptr, mis)), "a pointer's alignment is not what was asked for"
        self.put_actions(np.zeros((K, n), action_dtype))

    def put_actions(self, a):
        raw = np.zeros(self.nbytes[0] + 16, np.uint8)
        raw[self.mis[0]: self.mis[0] + self.nbytes[0]] = np.ascontiguousarray(a, self.dtypes[0]).reshape(-1).view(np.uint8)
        self.arr[0].copy_from(raw)

    def pointers(self, k=None):
        """(actions, obs, reward, done, truncated) of the call, or of the slabs of step k"""
        return tuple(p if p is None or k is None else p + k * (b // self.K) for p, b in zip(self.ptr, self.nbytes))

    def _get(self, i):
        if self.arr[i] is None:
            return None
        return self.arr[i].numpy()[self.mis[i]: self.mis[i] + self.nbytes[i]].copy().view(self.dtypes[i]).reshape(self.shapes[i])

    def actions(self):
        return self._get(0)

    def read(self):
        """-> (obs, reward, done, truncated), each [K, ..]; obs None without an observation buffer: the caller reads the engine's view"""
        return tuple(self._get(i) for i in range(1, 5))

    def host(self):
        """-> dict(act, obs, rew, done, trunc) of the buffers there are, each [K, ..]"""
        return {k: self._get(i) for i, k in enumerate(("act", "obs", "rew", "done", "trunc")) if self.arr[i] is not None}

    def step(self, env, a):
        """one mgym_step on the buffers -> (obs, reward, done, truncated) of the step"""
        self.put_actions(a)
        env.step_device(*self.pointers())
        env.sync()
        o, r, d, t = self.read()
        return (o[0] if o is not None else env.observation()), r[0], d[0], t[0]


def policy_call(env, src, K, b, linear=None, mlp=None, seed=0, call=0, sigma=0.5):
    """the K-step call of the action source `src` on the buffers b, then a sync.  step and table read b's actions, the others write them: uniform, linear,
    mlp_ / sample_ / gauss_<activation> (mlp = (packed policy, H)), mlp2_<activation>_<head> (mlp = (packed policy, H1, H2)); seed, call, sigma: the draw's"""
    act, *outs = b.pointers()
    form, _, rest = src.partition("_")
    if src == "step":
        assert K == 1
        env.step_device(act, *outs)
    elif src == "table":
        env.rollout_device(act, K, *outs)
    elif src == "uniform":
        env.rollout_uniform_device(seed, K, act, *outs)
    elif src == "linear":
        env.rollout_linear_device(linear, K, act, *outs)
    elif form == "mlp":
        env.rollout_mlp_device(*mlp, rest, K, act, *outs)
    elif form == "sample":
        env.rollout_mlp_sample_device(*mlp, rest, seed, call, K, act, *outs)
    elif form == "gauss":
        env.rollout_mlp_gauss_device(*mlp, rest, sigma, seed, call, K, act, *outs)
    else:
        assert form == "mlp2", src
        activation, _, head = rest.rpartition("_")
        env.rollout_mlp2_device(*mlp, activation, head, sigma, seed, call, K, act, *outs)
    env.sync()


def copy_state(src, twin):
    """the state blob of src into twin, and the elapsed counts where the family keeps them outside the blob and a limit is set"""
    twin.set_state(src.get_state())
    if src.max_episode_steps and src.kind != mg.CARTPOLE:
        twin.set_elapsed_steps(src.elapsed_steps())


def twin_steps(stepper, twin, actions, step=lambda env, a: env.step(a)):
    """K single steps of the auto-reset handle `stepper`, its state copied before each into `twin`, a handle of the same configuration without auto-reset
    that takes the same action through step(twin, a); the flags of the two agree.  -> (the stepper's outputs per step, the twin's obs [K, D, n]: what
    each step produced before any reset, and its done and truncated [K, n] as bool)"""
    outs, tobs, tdone, ttrunc = [], [], [], []
    for a in actions:
        copy_state(stepper, twin)
        outs.append([x.copy() for x in stepper.step(a)])
        o, _, d, t = step(twin, a)
        assert same(outs[-1][2], d) and same(outs[-1][3], t), "the twin's flags are the stepping handle's"
        tobs.append(o.copy()), tdone.append(d.astype(bool)), ttrunc.append(t.astype(bool))
    return outs, np.array(tobs), np.array(tdone), np.array(ttrunc)
