"""mgym_gae on the device against the numpy restatement of its text (tests/gae_ref.py), word for word (words.same: exact words, NaNs included).

Inputs are synthetic, from seeded generators: rewards in [-16, 1], values in +-100, flag bytes of any non-zero value at rates of 0.08 with the first lanes
patched by hand (gae_ref.flags); each case first asserts the classes of endings it claims (gae_ref.check_coverage).  final_value holds a NaN word wherever the
text does not read it, and the outputs are pre-filled with that NaN word between two guards: every output word must have been written, the guards not.

Shapes: n = 2052 is two 1024-environment tiles of the four-per-lane kernel plus one lane; n = 1030 (not a multiple of 4) and a reward buffer 4 bytes off a
16-byte boundary take the one-environment-per-lane kernel; K = 1, 2, 17 and B - 1, B, B + 1 for the kernel's load batch B (a partial batch alone, full batches
alone, both)."""
import functools

import numpy as np
import pytest

import device_buffers
import gae_ref as R
import modurl_gym_amd as mg
from modurl_gym_amd import _lib
from words import same

pytestmark = pytest.mark.gpu

F = np.float32
N = 2052
B = R.batch()
KS = sorted({1, 2, 17, B - 1, B, B + 1})
Guarded = functools.partial(device_buffers.Guarded, fill=R.NAN_WORD)   # the word the inputs are built round
GAMMA, LAM = 0.99, 0.95


@functools.lru_cache(maxsize=None)
def case(K, n):
    """the inputs of one shape (computed once, never modified); fvals: finite values for final_value() to place where a call reads them"""
    rng = np.random.default_rng(4000 + 10 * K + n)
    r, v = rng.uniform(-16, 1, (K, n)).astype(F), rng.uniform(-100, 100, (K, n)).astype(F)
    lv = rng.uniform(-100, 100, n).astype(F)
    d, u = R.flags(rng, K, n)
    R.check_coverage(d, u)
    d, u = (d * rng.integers(1, 256, (K, n))).astype(np.uint8), (u * rng.integers(1, 256, (K, n))).astype(np.uint8)   # any non-zero byte is a set flag
    fvals = rng.uniform(-100, 100, (K, n)).astype(F)
    for a in (r, v, lv, d, u, fvals):
        a.setflags(write=False)
    return dict(r=r, v=v, lv=lv, d=d, u=u, fvals=fvals)


@functools.lru_cache(maxsize=None)
def final_value(K, n, with_d=True, with_u=True):
    """finite where the call reads it — trunc && !done under the flags the call passes — and the NaN word everywhere else"""
    c = case(K, n)
    sel = ((c["u"] != 0) if with_u else np.zeros((K, n), bool)) & ~((c["d"] != 0) if with_d else np.zeros((K, n), bool))
    fv = np.where(sel, c["fvals"], np.full((K, n), R.NAN_WORD, np.uint32).view(F))
    fv.setflags(write=False)
    return fv


@functools.lru_cache(maxsize=None)
def expected(K, n, with_d=True, with_u=True, with_fv=True):
    c = case(K, n)
    return R.gae(c["r"], c["d"] if with_d else None, c["u"] if with_u else None, c["v"], c["lv"], final_value(K, n, with_d, with_u) if with_fv else None, GAMMA, LAM)


class Slabs:
    def __init__(self, K, n, mis_rew=0, with_d=True, with_u=True, with_fv=True, with_adv=True, with_ret=True):
        c = case(K, n)
        self.K, self.n = K, n
        self.r, self.v, self.lv = Guarded(K * n, mis_rew, c["r"]), Guarded(K * n, 0, c["v"]), Guarded(n, 0, c["lv"])
        self.d = mg.DeviceArray.from_numpy(c["d"]) if with_d else None
        self.u = mg.DeviceArray.from_numpy(c["u"]) if with_u else None
        self.fv = Guarded(K * n, 0, final_value(K, n, with_d, with_u)) if with_fv else None
        self.adv = Guarded(K * n) if with_adv else None
        self.ret = Guarded(K * n) if with_ret else None

    def args(self):
        return (self.K, self.r, self.d, self.u, self.v, self.lv, self.fv, GAMMA, LAM, self.adv, self.ret)

    def check(self, exp, what):
        for name, buf, e in (("adv", self.adv, exp[0]), ("ret", self.ret, exp[1])):
            if buf is None:
                continue
            got = buf.payload((self.K, self.n), F)
            assert (got.view(np.uint32) != R.NAN_WORD).all(), f"{what}: {name} has words that were not written"
            assert same(got, e), f"{what}: {int((got.view(np.uint32) != e.view(np.uint32)).sum())} words of {name} differ from the restatement"
            assert buf.guards_hold(), f"{what}: a guard word of {name} was written"
        assert self.inputs_untouched()

    def inputs_untouched(self):
        c = case(self.K, self.n)
        return (all(b.untouched() for b in (self.r, self.v, self.lv, self.fv) if b is not None)
                and (self.d is None or same(self.d.numpy(), c["d"])) and (self.u is None or same(self.u.numpy(), c["u"])))


@pytest.fixture(scope="module")
def env():
    e = mg.VecEnv(mg.CARTPOLE, N)
    yield e
    e.close()


def run(env, K, n=N, **kw):
    b = Slabs(K, n, **kw)
    env.gae_device(*b.args())
    env.sync()
    exp = expected(K, n, kw.get("with_d", True), kw.get("with_u", True), kw.get("with_fv", True))
    b.check(exp, f"K={K} n={n} {kw}")
    return exp


@pytest.mark.parametrize("K", KS)
def test_four_per_lane(env, K):
    adv, ret = run(env, K)
    assert np.isfinite(adv).all() and np.isfinite(ret).all()   # the NaN words of final_value reach nothing


@pytest.mark.parametrize("nulls", [dict(with_d=False), dict(with_u=False), dict(with_fv=False), dict(with_d=False, with_u=False, with_fv=False),
                                   dict(with_d=False, with_u=False), dict(with_adv=False), dict(with_ret=False)], ids=lambda d: "-".join(d))
def test_null_arguments(env, nulls):
    for K in (B - 1, 17):
        run(env, K, **nulls)


@pytest.mark.parametrize("K", [1, B + 1, 17])
def test_one_per_lane(K):
    e = mg.VecEnv(mg.MOUNTAINCAR, 1030)
    run(e, K, 1030)
    run(e, K, 1030, with_d=False, with_fv=False, with_adv=False)
    e.close()


@pytest.mark.parametrize("K", [2, 17])
def test_misaligned_reward(env, K):
    run(env, K, mis_rew=1)


def test_a_nan_beyond_an_episode_end_stays_there(env):
    """value, reward and last_value NaN in the odd environments: the even ones give the words of the clean run"""
    K = 17
    c = case(K, N)
    b = Slabs(K, N)
    r, v, lv = c["r"].copy(), c["v"].copy(), c["lv"].copy()
    r[:, 1::2], v[:, 1::2], lv[1::2] = np.nan, np.nan, np.nan
    b.r.fill(r), b.v.fill(v), b.lv.fill(lv)
    env.gae_device(*b.args())
    env.sync()
    exp = expected(K, N)
    for buf, e in ((b.adv, exp[0]), (b.ret, exp[1])):
        got = buf.payload((K, N), F)
        assert same(got[:, 0::2], e[:, 0::2]) and np.isnan(got[:, 1::2]).all()


def test_graph_replay_equals_the_eager_call(env):
    K = B + 1
    b = Slabs(K, N)
    g = env.graph_capture(lambda: env.gae_device(*b.args()))
    try:
        env.sync()
        assert b.adv.untouched() and b.ret.untouched()   # capture launches nothing
        env.graph_launch(g)
        env.sync()
        b.check(expected(K, N), "graph replay")
    finally:
        env.graph_destroy(g)


def test_host_array_forms(env):
    """VecEnv.gae / VecEnv.episode_returns: numpy in, numpy out, the same words; episode_returns' outputs are 0 where no episode ended"""
    K = B + 1
    c = case(K, N)
    adv, ret = env.gae(c["r"], c["d"], c["u"], c["v"], c["lv"], final_value(K, N), GAMMA, LAM)
    exp = expected(K, N)
    assert same(adv, exp[0]) and same(ret, exp[1])
    acc0, len0 = np.full(N, -2.5, F), np.full(N, 3, np.uint32)
    for carry in ((None, None), (acc0, len0)):
        ret_out, len_out, acc, length = env.episode_returns(c["r"], c["d"], c["u"], *carry)
        e = R.episode_returns(c["r"], c["d"], c["u"], np.zeros(N, F) if carry[0] is None else acc0, np.zeros(N, np.uint32) if carry[1] is None else len0, fill=0)
        assert same(acc, e[0]) and same(length, e[1]) and same(ret_out.view(np.uint32), e[2]) and same(len_out, e[3])


def test_lunar_lander_handle_never_reset():
    e = mg.VecEnv(mg.LUNARLANDER, 8)
    c = dict(r=np.arange(24, dtype=F).reshape(3, 8), v=np.ones((3, 8), F), lv=np.full(8, 2, F), d=np.zeros((3, 8), np.uint8), u=np.zeros((3, 8), np.uint8))
    c["d"][1, :4], c["u"][2, 2:6] = 1, 1
    dev = {k: mg.DeviceArray.from_numpy(a) for k, a in c.items()}
    adv, ret = Guarded(24), Guarded(24)
    e.gae_device(3, dev["r"], dev["d"], dev["u"], dev["v"], dev["lv"], None, GAMMA, LAM, adv, ret)
    e.sync()   # (no sticky status: no state of the handle was stepped)
    exp = R.gae(c["r"], c["d"], c["u"], c["v"], c["lv"], None, GAMMA, LAM)
    assert same(adv.payload((3, 8), F), exp[0]) and same(ret.payload((3, 8), F), exp[1]) and adv.guards_hold() and ret.guards_hold()
    assert e.episode_count() == 0
    with pytest.raises(mg.NotResetError):   # ... and the handle is still one that was never reset
        e.step(np.zeros(8, np.uint32))
    e.close()


def test_no_environments():
    e = mg.VecEnv(mg.CARTPOLE, 0)
    x = mg.DeviceArray(4, F)
    e.gae_device(3, x, None, None, x.ptr, x.ptr, None, GAMMA, LAM, Guarded(4), None)   # MGYM_OK without a launch
    with pytest.raises(mg.MgymError):
        e.gae_device(0, x, None, None, x, x, None, GAMMA, LAM, Guarded(4), None)          # ... after the argument checks
    e.close()


def bad_arg(fn, *needles):
    with pytest.raises(mg.MgymError) as ei:
        fn()
    assert ei.value.status == _lib.ERR_BAD_ARG and all(s in str(ei.value) for s in ("mgym_gae:",) + needles), str(ei.value)


def test_errors(env):
    K = 2
    b = Slabs(K, N)
    a = list(b.args())
    IK, IR, ID, IU, IV, ILV, IFV, IG, IL, IADV, IRET = range(11)

    def call(repl):
        args = list(a)
        for k, v in repl.items():
            args[k] = v
        return lambda: env.gae_device(*args)

    rows = [({IK: 0}, "K"), ({IK: -1}, "K"), ({IR: None}, "reward"), ({IV: None}, "value"), ({ILV: None}, "last_value"), ({IADV: None, IRET: None}, "adv_out", "ret_out"),
            ({IG: float("nan")}, "gamma"), ({IG: -0.01}, "gamma"), ({IG: 1.01}, "gamma"), ({IL: float("nan")}, "lambda"), ({IL: -0.5}, "lambda"), ({IL: 1.5}, "lambda"),
            ({IR: b.r.ptr + 2}, "reward", "4-byte aligned"), ({IV: b.v.ptr + 1}, "value", "4-byte aligned"), ({ILV: b.lv.ptr + 2}, "last_value", "4-byte aligned"),
            ({IFV: b.fv.ptr + 2}, "final_value", "4-byte aligned"), ({IADV: b.adv.ptr + 2}, "adv_out", "4-byte aligned"), ({IRET: b.ret.ptr + 3}, "ret_out", "4-byte aligned"),
            ({IADV: b.r.ptr}, "adv_out", "reward"), ({IRET: b.v.ptr}, "ret_out", "value"), ({IADV: b.lv.ptr}, "adv_out", "last_value"), ({IRET: b.fv.ptr}, "ret_out", "final_value"),
            ({IADV: b.d.ptr}, "adv_out", "done"), ({IRET: b.u.ptr}, "ret_out", "trunc")]
    for repl, *needles in rows:
        bad_arg(call(repl), *needles)
    env.sync()
    assert b.inputs_untouched() and b.adv.untouched() and b.ret.untouched()
    call({IG: 0.0, IL: 1.0})()   # the ends of [0, 1] are accepted
    call({IG: 1.0, IL: 0.0})()
    env.gae_device(*a)
    env.sync()
    b.check(expected(K, N), "after the refused calls")


def test_torch_env_integration():
    """Pendulum under a 7-step limit, a Gaussian MLP collector, V = a fixed random linear function of the observation: TorchVecEnv.gae on the rollout's own
    tensors equals the restatement on the downloaded arrays, and episode_returns over two rollouts reports length 7 for every episode that started in them"""
    torch = pytest.importorskip("torch")
    from modurl_gym_amd.torch_env import TorchVecEnv
    K, LIMIT, H = 16, 7, 8
    env = TorchVecEnv(mg.PENDULUM, N, seed=2024, final_obs_steps=K, max_episode_steps=LIMIT)
    obs0 = env.reset().clone()
    el0 = (np.random.default_rng(11).permutation(N) % LIMIT).astype(np.int32)   # staggered: a lane's environments are truncated on different steps
    env.set_elapsed_steps(torch.from_numpy(el0).to(env.device))
    rng = np.random.default_rng(9)
    w1, b1, w2, b2 = (rng.normal(0, 1, s).astype(F) for s in ((H, 3), (H,), (1, H), (1,)))
    vw, vb = torch.from_numpy(rng.normal(0, 30, 3).astype(F)).to(env.device), 5.0
    value = lambda o: torch.einsum("d,...dn->...n", vw, o) + vb   # [.., 3, n] -> [.., n]
    lengths, first_end = [], np.full(N, -1)
    for call in range(2):
        act, obs, rew, done, trunc = env.rollout_mlp_gauss(w1, b1, w2, b2, K, 0.5, 77, call)
        v = value(torch.cat([obs0[None], obs[:-1]]))
        last, fv = value(obs[-1]), value(env.final_obs[:K])
        adv, ret = env.gae(rew, done, trunc, v, last, fv, GAMMA, LAM)
        ep_ret, ep_len = env.episode_returns(rew, done, trunc)
        env.check()
        h = {k: x.cpu().numpy() for k, x in dict(rew=rew, done=done, trunc=trunc, v=v, last=last, fv=fv, adv=adv, ret=ret, ep_ret=ep_ret, ep_len=ep_len).items()}
        assert h["trunc"].sum() >= 2 * N and not h["done"].any()   # Pendulum only ever truncates: V(final observation) is what every ending reads
        exp = R.gae(h["rew"], h["done"], h["trunc"], h["v"], h["last"], h["fv"], GAMMA, LAM)
        assert same(h["adv"], exp[0]) and same(h["ret"], exp[1])
        assert not same(exp[0], R.gae(h["rew"], h["done"], h["trunc"], h["v"], h["last"], None, GAMMA, LAM)[0])   # final_value matters here
        fin = h["trunc"] | h["done"]
        assert np.array_equal(h["ep_len"] > 0, fin) and (h["ep_ret"][~fin] == 0).all()
        lengths.append((fin, h["ep_len"], h["ep_ret"], h["rew"]))
        obs0 = obs[-1].clone()
    fin, ln, er, rw = (np.concatenate([a[i] for a in lengths]) for i in range(4))
    assert fin[: LIMIT].any(axis=0).all()   # every environment's first ending lies within the limit ...
    first = fin.argmax(axis=0)
    assert np.array_equal(ln[first, np.arange(N)], LIMIT - el0)   # ... and is that of the episode running since the reset, counted from the carry's 0
    later = fin.copy()
    later[first, np.arange(N)] = False
    assert later.sum() >= 3 * N and (ln[later] == LIMIT).all()   # every episode that started inside the two rollouts
    i = int(np.argmax(el0 == 3))   # one environment by hand: its second episode's return is the f32 sum of its 7 rewards in step order
    t0 = int(first[i])
    acc = F(0)
    for t in range(t0 + 1, t0 + 1 + LIMIT):
        acc = F(acc + rw[t, i])
    assert later[t0 + LIMIT, i] and er[t0 + LIMIT, i] == acc
    mask = torch.zeros(N, dtype=torch.uint8, device=env.device)
    mask[::2] = 1
    before = env._ep_length.clone()
    assert before[::2].any().item()
    env.reset(mask)   # reset(mask) zeroes the carry where the mask is set, and only there
    assert not env._ep_length[::2].any().item() and not env._ep_return[::2].any().item() and torch.equal(env._ep_length[1::2], before[1::2])
    env.reset()
    assert not env._ep_length.any().item() and not env._ep_return.any().item()   # reset() zeroes the carry
    env.close()
