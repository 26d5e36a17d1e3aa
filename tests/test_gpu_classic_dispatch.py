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
from device_buffers import FILL, CallBuffers, FinalBuf, policy_call
from families import BY_KIND, CLASSIC, FAMILIES
from words import same

pytestmark = pytest.mark.gpu

N, K, LIMIT = 8, 5, 3
SEED, PSEED, CALL, SIGMA = 31, 77, 3, 0.5
MODES = ("plain", "auto_reset", "final")
SOURCES = ("table", "uniform", "linear", "mlp_relu", "mlp_tanh_fast_draw", "mlp2_relu", "mlp2_tanh_fast_draw")
CASE_ID = {"mountain_car_continuous": "mountain_car_cont"}   # the cases keep the ids they have had
CASES = [pytest.param(FAMILIES[fam].kind, mode, limit, src, id=f"{CASE_ID.get(fam, fam)}-{mode}-limit{limit}-{src}")
         for fam in CLASSIC for mode in MODES for limit in ((0, LIMIT) if FAMILIES[fam].limit_ok else (0,)) for src in SOURCES]


def make(kind, mode, limit):
    """a handle of the case, reset; CartPole: environments 0..3 one step from the pole-angle threshold"""
    env = mg.VecEnv(kind, N, seed=SEED, auto_reset=mode != "plain", max_episode_steps=limit)
    env.reset()
    if kind == mg.CARTPOLE:
        blob = env.get_state().copy()
        blob[2, :4], blob[3, :4] = CP_THETA_THR, 1.0
        env.set_state(blob)
    return env


def buffers(env):
    """the [K, ..] device buffers of a case and its final-observation buffer"""
    return CallBuffers(N, env.obs_dim, np.uint32, K), FinalBuf(K, env.obs_dim, N)


def host(env, b, fb):
    assert fb.guards_hold()
    res = dict(b.host(), final=fb.payload(fb.shape), state=env.get_state(), count=np.array([env.episode_count()]))
    if env.kind != mg.CARTPOLE:
        res["elapsed"] = env.elapsed_steps()
    return res


def table_actions(kind):
    rng = np.random.default_rng(3)
    if BY_KIND[kind].box is not None:
        return rng.uniform(-2.5, 2.5, (K, N)).astype(np.float32).view(np.uint32)   # beyond the action bounds: the step clamps
    return rng.integers(0, 2 if kind == mg.CARTPOLE else 3, (K, N)).astype(np.uint32)


def fused_call(env, src, b):
    """the K-step call of the source, its actions into b's (the table's are there already)"""
    rng = np.random.default_rng(9)
    D, A = env.mlp_dims()
    draw = "sample" if BY_KIND[env.kind].box is None else "gauss"
    linear = mlp = None
    if src == "linear":
        linear = rng.normal(0, 1, BY_KIND[env.kind].lin).astype(np.float32)
    elif src.startswith("mlp2"):
        mlp = env.pack_mlp2(*(rng.normal(0, 1, s) for s in ((3, D), (3,), (5, 3), (5,), (A, 5), (A,))))
    elif src.startswith("mlp"):
        mlp = env.pack_mlp(*(rng.normal(0, 1, s) for s in ((2, D), (2,), (A, 2), (A,))))
    name = {"mlp_tanh_fast_draw": f"{draw}_tanh_fast", "mlp2_relu": "mlp2_relu_greedy", "mlp2_tanh_fast_draw": f"mlp2_tanh_fast_{draw}"}.get(src, src)
    policy_call(env, name, K, b, linear, mlp, PSEED, CALL, SIGMA)


@pytest.mark.parametrize("kind,mode,limit,src", CASES)
def test_fused_call_is_k_steps(kind, mode, limit, src):
    env, ref = make(kind, mode, limit), make(kind, mode, limit)
    (b, fb), (rb, rfb) = buffers(env), buffers(ref)
    if src == "table":
        b.put_actions(table_actions(kind))
    if mode == "final":
        env.set_final_obs_out_device(fb.ptr, K)
    fused_call(env, src, b)
    got = host(env, b, fb)

    rb.put_actions(b.actions())
    for k in range(K):
        if mode == "final":
            ref.set_final_obs_out_device(rfb.ptr + 4 * k * ref.obs_dim * N, 1)
        ref.step_device(*rb.pointers(k))
    ref.sync()
    exp = host(ref, rb, rfb)
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
