"""The host dispatch of the classic families' fused rollouts, walked as a product: kind x handle mode x time limit x action source.  The other files go
source by source or feature by feature; here every combination the host wrappers turn into a kernel instantiation is launched once.

Each case is one K-step call on a handle against K mgym_step calls on a second handle of the same kind, seed and mode, fed the call's actions_out (or the
given table), its final-observation pointer moved to slab k before step k.  n = 8 is two lanes; K = 5 is above the limit of 3, so every limited environment
is truncated at step 3 and, with auto-reset, restarted inside the launch.  No CartPole episode ends in 5 steps from a reset, so both CartPole handles
first import a state that puts environments 0..3 on the pole-angle threshold with the pole moving outwards: they finish in the first step.
Compared word for word: obs, reward, done, truncated, the whole final-observation buffer (pre-filled with one sentinel word on both sides), the state
blob, the elapsed counts (not CartPole: its counter is in the blob) and the episode count."""
import numpy as np
import pytest

import modurl_gym_amd as mg
from classic_edge_cases import CP_THETA_THR
from modurl_gym_amd.envs import DeviceArray
from words import same

pytestmark = pytest.mark.gpu

N, K, LIMIT = 8, 5, 3
SEED, PSEED, CALL, SIGMA = 31, 77, 3, 0.5
FILL = 0x7FC0DEAD   # a NaN word no step produces
KINDS = {"cartpole": mg.CARTPOLE, "mountain_car": mg.MOUNTAINCAR, "mountain_car_cont": mg.MOUNTAINCAR_CONT, "pendulum": mg.PENDULUM, "acrobot": mg.ACROBOT}
BOX = (mg.MOUNTAINCAR_CONT, mg.PENDULUM)
MODES = ("plain", "auto_reset", "final")
SOURCES = ("table", "uniform", "linear", "mlp_relu", "mlp_tanh_fast_draw", "mlp2_relu", "mlp2_tanh_fast_draw")
CASES = [pytest.param(kind, mode, limit, src, id=f"{fam}-{mode}-limit{limit}-{src}")
         for fam, kind in KINDS.items() for mode in MODES for limit in ((0,) if kind == mg.CARTPOLE else (0, LIMIT)) for src in SOURCES]


def make(kind, mode, limit):
    """a handle of the case, reset; CartPole: environments 0..3 one step from the pole-angle threshold"""
    env = mg.VecEnv(kind, N, seed=SEED, auto_reset=mode != "plain", max_episode_steps=limit)
    env.reset()
    if kind == mg.CARTPOLE:
        blob = env.get_state().copy()
        blob[2, :4], blob[3, :4] = CP_THETA_THR, 1.0
        env.set_state(blob)
    return env


class Bufs:
    """the [K, ..] device outputs of a case and its final-observation buffer, filled with FILL"""

    def __init__(self, env):
        self.D = env.obs_dim
        self.act = DeviceArray((K, N), np.uint32)
        self.obs, self.rew = DeviceArray((K, self.D, N), np.float32), DeviceArray((K, N), np.float32)
        self.done, self.trunc = DeviceArray((K, N), np.uint8), DeviceArray((K, N), np.uint8)
        self.fin = DeviceArray.from_numpy(np.full((K, self.D, N), FILL, np.uint32))

    def outs(self, k=0):
        """the pointers of step k's slabs: obs, reward, done, truncated"""
        return self.obs.ptr + 4 * k * self.D * N, self.rew.ptr + 4 * k * N, self.done.ptr + k * N, self.trunc.ptr + k * N

    def host(self, env):
        res = dict(obs=self.obs.numpy(), rew=self.rew.numpy(), done=self.done.numpy(), trunc=self.trunc.numpy(), final=self.fin.numpy(),
                   state=env.get_state(), count=np.array([env.episode_count()]))
        if env.kind != mg.CARTPOLE:
            res["elapsed"] = env.elapsed_steps()
        return res


def table_actions(kind):
    rng = np.random.default_rng(3)
    if kind in BOX:
        return rng.uniform(-2.5, 2.5, (K, N)).astype(np.float32).view(np.uint32)   # beyond the action bounds: the step clamps
    return rng.integers(0, 2 if kind == mg.CARTPOLE else 3, (K, N)).astype(np.uint32)


def fused_call(env, src, b):
    """the K-step call of the source, its actions into b.act (the table's are there already)"""
    rng = np.random.default_rng(9)
    D, A = env.mlp_dims()
    draw = "gauss" if env.kind in BOX else "sample"
    if src == "table":
        env.rollout_device(b.act, K, *b.outs())
    elif src == "uniform":
        env.rollout_uniform_device(PSEED, K, b.act, *b.outs())
    elif src == "linear":
        rows = 3 if env.kind in (mg.MOUNTAINCAR, mg.ACROBOT) else 1
        env.rollout_linear_device(rng.normal(0, 1, rows * (D + 1)).astype(np.float32), K, b.act, *b.outs())
    elif src.startswith("mlp2"):
        pol, h1, h2 = env.pack_mlp2(*(rng.normal(0, 1, s) for s in ((3, D), (3,), (5, 3), (5,), (A, 5), (A,))))
        activation, head = ("relu", "greedy") if src == "mlp2_relu" else ("tanh_fast", draw)
        env.rollout_mlp2_device(pol, h1, h2, activation, head, SIGMA, PSEED, CALL, K, b.act, *b.outs())
    else:
        pol, h = env.pack_mlp(*(rng.normal(0, 1, s) for s in ((2, D), (2,), (A, 2), (A,))))
        if src == "mlp_relu":
            env.rollout_mlp_device(pol, h, "relu", K, b.act, *b.outs())
        elif draw == "sample":
            env.rollout_mlp_sample_device(pol, h, "tanh_fast", PSEED, CALL, K, b.act, *b.outs())
        else:
            env.rollout_mlp_gauss_device(pol, h, "tanh_fast", SIGMA, PSEED, CALL, K, b.act, *b.outs())
    env.sync()


@pytest.mark.parametrize("kind,mode,limit,src", CASES)
def test_fused_call_is_k_steps(kind, mode, limit, src):
    env, ref = make(kind, mode, limit), make(kind, mode, limit)
    b, rb = Bufs(env), Bufs(ref)
    if src == "table":
        b.act.copy_from(table_actions(kind))
    if mode == "final":
        env.set_final_obs_out_device(b.fin, K)
    fused_call(env, src, b)
    got = b.host(env)

    rb.act.copy_from(b.act.numpy())
    for k in range(K):
        if mode == "final":
            ref.set_final_obs_out_device(rb.fin.ptr + 4 * k * rb.D * N, 1)
        ref.step_device(rb.act.ptr + 4 * k * N, *rb.outs(k))
    ref.sync()
    exp = rb.host(ref)
    env.close(), ref.close()

    for key in exp:
        assert same(got[key], exp[key]), f"{key} differs from K steps on the call's actions"
    fin = (exp["done"] | exp["trunc"]).astype(bool)
    if limit:
        assert fin[LIMIT - 1].all() and exp["trunc"][LIMIT - 1].all(), "every environment is truncated at the limit"
    if kind == mg.CARTPOLE and mode != "plain":
        assert exp["done"].any(), "a CartPole episode ends inside the launch"
    if mode == "final":
        assert ((exp["final"] != FILL).any(axis=1) == fin).all(), "a final observation for each finished env-step, and for no other"
    else:
        assert (exp["final"] == FILL).all()
