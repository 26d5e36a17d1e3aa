"""mgym_episode_returns on the device against the numpy restatement of its text (tests/gae_ref.py), word for word.

return_out and length_out are pre-filled with a NaN word between two guards: the words under done | trunc equal the restatement's, and EVERY other word and
both guards still hold the fill.  The carry (ep_return, ep_length) starts from non-zero values, so that an episode begun before the call is counted.  Inputs,
shapes and coverage as in test_gpu_gae.py: n = 2052 four per lane; n = 1030 and a misaligned reward buffer one per lane; K = 1, 2, 17, B - 1, B, B + 1."""
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


@functools.lru_cache(maxsize=None)
def case(K, n):
    rng = np.random.default_rng(6000 + 10 * K + n)
    r = rng.uniform(-16, 1, (K, n)).astype(F)
    d, u = R.flags(rng, K, n)
    R.check_coverage(d, u)
    d, u = (d * rng.integers(1, 256, (K, n))).astype(np.uint8), (u * rng.integers(1, 256, (K, n))).astype(np.uint8)   # any non-zero byte is a set flag
    acc, length = rng.uniform(-300, 0, n).astype(F), rng.integers(0, 500, n).astype(np.uint32)
    length[0] = 0xFFFFFFFF   # env 0 never ends: its count wraps as a u32
    for a in (r, d, u, acc, length):
        a.setflags(write=False)
    return dict(r=r, d=d, u=u, acc=acc, len=length)


@functools.lru_cache(maxsize=None)
def expected(K, n, with_d=True, with_u=True):
    c = case(K, n)
    return R.episode_returns(c["r"], c["d"] if with_d else None, c["u"] if with_u else None, c["acc"], c["len"])


class Slabs:
    def __init__(self, K, n, mis_rew=0, with_d=True, with_u=True, with_ret=True, with_len=True):
        c = case(K, n)
        self.K, self.n = K, n
        self.r = Guarded(K * n, mis_rew, c["r"])
        self.d = mg.DeviceArray.from_numpy(c["d"]) if with_d else None
        self.u = mg.DeviceArray.from_numpy(c["u"]) if with_u else None
        self.acc, self.len = Guarded(n, 0, c["acc"]), Guarded(n, 0, c["len"])
        self.ret_out = Guarded(K * n) if with_ret else None
        self.len_out = Guarded(K * n) if with_len else None

    def args(self):
        return (self.K, self.r, self.d, self.u, self.acc, self.len, self.ret_out, self.len_out)

    def check(self, exp, what):
        acc, length, ret_out, len_out = exp
        assert same(self.acc.payload((self.n,)), acc.view(np.uint32)) and same(self.len.payload((self.n,)), length), f"{what}: the carry"
        assert self.acc.guards_hold() and self.len.guards_hold()
        for name, buf, e in (("return_out", self.ret_out, ret_out), ("length_out", self.len_out, len_out)):
            if buf is None:
                continue
            got = buf.payload((self.K, self.n))
            written = e != R.NAN_WORD
            assert np.array_equal(got[written], e[written]), f"{what}: {name} differs from the restatement where an episode ended"
            assert (got[~written] == R.NAN_WORD).all(), f"{what}: {int((got[~written] != R.NAN_WORD).sum())} words of {name} outside done | trunc were written"
            assert buf.guards_hold(), f"{what}: a guard word of {name} was written"
        assert self.inputs_untouched()

    def inputs_untouched(self):
        c = case(self.K, self.n)
        return self.r.untouched() and (self.d is None or same(self.d.numpy(), c["d"])) and (self.u is None or same(self.u.numpy(), c["u"]))


@pytest.fixture(scope="module")
def env():
    e = mg.VecEnv(mg.ACROBOT, N)
    yield e
    e.close()


def run(env, K, n=N, **kw):
    b = Slabs(K, n, **kw)
    env.episode_returns_device(*b.args())
    env.sync()
    b.check(expected(K, n, kw.get("with_d", True), kw.get("with_u", True)), f"K={K} n={n} {kw}")


@pytest.mark.parametrize("K", KS)
def test_four_per_lane(env, K):
    run(env, K)


@pytest.mark.parametrize("nulls", [dict(with_d=False), dict(with_u=False), dict(with_d=False, with_u=False), dict(with_ret=False), dict(with_len=False),
                                   dict(with_ret=False, with_len=False)], ids=lambda d: "-".join(d))
def test_null_arguments(env, nulls):
    for K in (B - 1, 17):
        run(env, K, **nulls)


@pytest.mark.parametrize("K", [1, B + 1, 17])
def test_one_per_lane(K):
    e = mg.VecEnv(mg.PENDULUM, 1030)
    run(e, K, 1030)
    run(e, K, 1030, with_u=False, with_len=False)
    e.close()


@pytest.mark.parametrize("K", [2, 17])
def test_misaligned_reward(env, K):
    run(env, K, mis_rew=1)


@pytest.mark.parametrize("K1,K2", [(1, B), (B - 1, B + 2), (17, 2)])
def test_two_calls_leave_the_words_of_one(env, K1, K2):
    K = K1 + K2
    c = case(K, N)
    one = expected(K, N)
    acc, length = Guarded(N, 0, c["acc"]), Guarded(N, 0, c["len"])
    ret_out, len_out = Guarded(K * N), Guarded(K * N)
    r, d, u = mg.DeviceArray.from_numpy(c["r"]), mg.DeviceArray.from_numpy(c["d"]), mg.DeviceArray.from_numpy(c["u"])
    env.episode_returns_device(K1, r, d, u, acc, length, ret_out, len_out)
    env.episode_returns_device(K2, r.ptr + 4 * K1 * N, d.ptr + K1 * N, u.ptr + K1 * N, acc, length, ret_out.ptr + 4 * K1 * N, len_out.ptr + 4 * K1 * N)
    env.sync()
    assert same(acc.payload((N,)), one[0].view(np.uint32)) and same(length.payload((N,)), one[1])
    assert same(ret_out.payload((K, N)), one[2]) and same(len_out.payload((K, N)), one[3]) and ret_out.guards_hold() and len_out.guards_hold()


def test_graph_replay_equals_the_eager_call(env):
    K = B + 1
    b = Slabs(K, N)
    g = env.graph_capture(lambda: env.episode_returns_device(*b.args()))
    try:
        env.sync()
        assert b.acc.untouched() and b.ret_out.untouched()   # capture launches nothing
        env.graph_launch(g)
        env.sync()
        b.check(expected(K, N), "graph replay")
    finally:
        env.graph_destroy(g)


def test_lunar_lander_handle_never_reset():
    e = mg.VecEnv(mg.LUNARLANDER, 8)
    r, d = np.arange(24, dtype=F).reshape(3, 8), np.zeros((3, 8), np.uint8)
    d[1, :4], d[2, 2:6] = 1, 1
    acc, length, ret_out, len_out = Guarded(8, 0, np.zeros(8, F)), Guarded(8, 0, np.zeros(8, np.uint32)), Guarded(24), Guarded(24)
    e.episode_returns_device(3, mg.DeviceArray.from_numpy(r), mg.DeviceArray.from_numpy(d), None, acc, length, ret_out, len_out)
    e.sync()
    exp = R.episode_returns(r, d, None, np.zeros(8, F), np.zeros(8, np.uint32))
    assert same(acc.payload((8,), F), exp[0]) and same(length.payload((8,)), exp[1]) and same(ret_out.payload((3, 8)), exp[2]) and same(len_out.payload((3, 8)), exp[3])
    assert e.episode_count() == 0
    with pytest.raises(mg.NotResetError):   # the handle is still one that was never reset
        e.step(np.zeros(8, np.uint32))
    e.close()


def bad_arg(fn, *needles):
    with pytest.raises(mg.MgymError) as ei:
        fn()
    assert ei.value.status == _lib.ERR_BAD_ARG and all(s in str(ei.value) for s in ("mgym_episode_returns:",) + needles), str(ei.value)


def test_errors(env):
    K = 2
    b = Slabs(K, N)
    a = list(b.args())
    IK, IR, ID, IU, IACC, ILEN, IRO, ILO = range(8)

    def call(repl):
        args = list(a)
        for k, v in repl.items():
            args[k] = v
        return lambda: env.episode_returns_device(*args)

    rows = [({IK: 0}, "K"), ({IK: -2}, "K"), ({IR: None}, "reward"), ({IACC: None}, "ep_return"), ({ILEN: None}, "ep_length"),
            ({IR: b.r.ptr + 2}, "reward", "4-byte aligned"), ({IACC: b.acc.ptr + 1}, "ep_return", "4-byte aligned"), ({ILEN: b.len.ptr + 2}, "ep_length", "4-byte aligned"),
            ({IRO: b.ret_out.ptr + 2}, "return_out", "4-byte aligned"), ({ILO: b.len_out.ptr + 3}, "length_out", "4-byte aligned")]
    for repl, *needles in rows:
        bad_arg(call(repl), *needles)
    env.sync()
    assert b.inputs_untouched() and all(x.untouched() for x in (b.acc, b.len, b.ret_out, b.len_out))
    env.episode_returns_device(*a)
    env.sync()
    b.check(expected(K, N), "after the refused calls")
    e0 = mg.VecEnv(mg.CARTPOLE, 0)
    e0.episode_returns_device(3, b.r, None, None, b.acc, b.len, None, None)   # no environments: MGYM_OK without a launch
    e0.close()
