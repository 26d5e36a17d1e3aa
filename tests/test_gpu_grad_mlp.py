"""mgym_ppo_grad_mlp and mgym_value_grad_mlp on the device against the float64 restatement (tests/grad_ref.py: grad64), every gradient word within
GRAD_BOUND x S_w and every statistic within STAT_BOUND x S_w — S_w the word's mean absolute per-env-step term, the bounds 4 x what the f32 text itself is from
float64 (test_grad_host.py) — and a word whose terms are all zero exactly zero.  One case per family of test_one_per_lane is a batch of 10 env-steps
(one partly filled wave), which is compared with the f32 text summed in float64 (grad_ref.grad32) under the same bounds: the text's own distance from float64
does not average out over 10 terms as it does at the batch sizes the bounds were measured at.

grad_out, stats_out and the workspace are poisoned slabs between guards: every output word must have been written, no guard and no word at or beyond
workspace_bytes may have been, and the inputs are untouched.  Shapes: n = 2052 is two 1024-environment tiles of the four-per-lane kernel plus one lane; n = 1030,
env_first = 1 and an obs buffer 4 bytes off a 16-byte boundary take the one-environment-per-lane kernel; K = 1, 2 and 17 leave a partial group of steps, K = 254 and 255 at n = 1028 stand on the two sides of the tile count at which the
four-per-lane kernel goes from one step per lane to two; a workspace of one, two or three slabs makes the blocks stride over the tiles."""
import functools

import numpy as np
import pytest

import device_buffers
import families
import grad_ref as G
import logprob_ref as R
import modurl_gym_amd as mg
from modurl_gym_amd import _lib
from words import same

pytestmark = pytest.mark.gpu

F = np.float32
N = 2052
KS = (1, 2, 17)
HS = (1, 17, 64)
Guarded = functools.partial(device_buffers.Guarded, fill=R.POISON)
bad_arg = device_buffers.bad_arg


@functools.lru_cache(maxsize=None)
def _env(family, n):
    return mg.VecEnv(families.KIND[family], n)


def env_of(family, n=N):
    """the one handle of a family and a population (its stream is the one every call on it is ordered on)"""
    return _env(family, n)


class Call:
    """the device buffers of one gradient call on the inputs of a grad_ref case"""

    def __init__(self, c, first=None, count=None, slabs=None, mis_obs=0, poison_outside=False):
        self.c, self.env = c, env_of(c.family, c.n)
        self.first, self.count = (0, c.n) if first is None else (first, count)
        D, K, n = c.D, c.K, c.n
        ins = dict(obs_first=c.obs_first, obs=c.obs, actions=c.actions, x0=c.x0, x1=c.x1)
        if poison_outside:   # a NaN in every input word outside the range
            ins = {k: None if v is None else self._poisoned(v) for k, v in ins.items()}
        self.obs_first, self.obs = Guarded(D * n, 0, ins["obs_first"]), Guarded(K * D * n, mis_obs, ins["obs"])
        self.actions = None if c.actions is None else Guarded(K * n, 0, ins["actions"])
        self.x0 = Guarded(K * n, 0, ins["x0"])
        self.x1 = None if c.x1 is None else Guarded(K * n, 0, ins["x1"])
        self.P = G.n_params(c.D, c.A, c.H)
        lo, hi = self.env.grad_workspace_bytes(c.H)
        self.ws_bytes = hi if slabs is None else slabs * lo + 8   # (the 8 bytes are no slab: they are never written)
        self.ws, self.grad, self.stats = Guarded((self.ws_bytes + 3) // 4), Guarded(self.P + 1), Guarded(8)

    def _poisoned(self, a):
        a = np.array(a)
        keep = np.zeros(a.shape[-1], bool)
        keep[self.first: self.first + self.count] = True
        nan = np.uint32(0x7FC00001) if a.dtype == np.uint32 else F(np.nan)
        return np.where(keep, a, nan).astype(a.dtype)

    def launch(self, **kw):
        c, e = self.c, self.env
        if c.head == G.VALUE:
            e.value_grad_mlp_device(c.pol, c.H, c.act, c.K, self.first, self.count, self.obs_first, self.obs, self.x0, self.ws, self.ws_bytes, self.grad, self.stats)
        else:
            a = dict(x0=self.x0, x1=self.x1, clip=c.clip, ent_coef=c.ent_coef)
            a.update(kw)
            e.ppo_grad_mlp_device(c.pol, c.H, c.act, "gauss" if c.gauss else "sample", c.sigma, c.K, self.first, self.count, self.obs_first, self.obs, self.actions,
                                  a["x0"], a["x1"], a["clip"], a["ent_coef"], self.ws, self.ws_bytes, self.grad, self.stats)

    def result(self, what):
        self.env.sync()
        grad, stats = self.grad.payload((self.P + 1,)), self.stats.payload((8,))
        assert (grad != R.POISON).all() and (stats != R.POISON).all(), f"{what}: an output word was not written"
        assert self.grad.guards_hold() and self.stats.guards_hold() and self.ws.guards_hold(), f"{what}: a guard word was written"
        assert all(b is None or b.untouched() for b in (self.obs_first, self.obs, self.actions, self.x0, self.x1)), f"{what}: an input was written"
        return grad.view(F).copy(), stats.view(F).copy()

    def check(self, what, ref=None, extra=0.0):
        grad, stats = self.result(what)
        ref = G.grad64(self.c, self.first, self.count) if ref is None else ref
        ok, (wg, ws) = G.within(grad, stats, ref, extra)
        print(f"{what}: largest |device - grad64| / S: gradient {wg:.3g} (bound {G.GRAD_BOUND:.3g}), statistics {ws:.3g} (bound {G.STAT_BOUND:.3g})")
        assert ok, f"{what}: gradient {wg:.3g} of {G.GRAD_BOUND:.3g}, statistics {ws:.3g} of {G.STAT_BOUND:.3g}, or a word that must be exact is not"
        return grad, stats


def run(family, K, n, H, act, head=G.PPO, text=False, **kw):
    """text: the yardstick is the f32 text summed in float64 (grad_ref.grad32) with grad64's S — for a batch of a few env-steps, where the text's own distance
    from float64 does not average out as it does at the batch sizes the bounds were measured at, and the device differs from the text by the order of its sums only"""
    c = G.case(family, K, n, H, act, head)
    b = Call(c, **kw)
    b.launch()
    ref = None
    if text:
        ref = G.grad64(c, b.first, b.count)
        ref.grad, ref.stats = (x.astype(np.float64) for x in G.grad32(c, b.first, b.count))
    return b.check(f"{family} {head} K={K} n={n} H={H} act={act} {kw}", ref)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("family", R.ALL)
def test_four_per_lane(family, K):
    for H in HS:
        for act in G.ACTS:
            run(family, K, N, H, act)


@pytest.mark.parametrize("K", (254, 255))
def test_both_step_counts_of_the_four_per_lane_form(K):
    """the four-per-lane kernel takes two steps per lane when that gives at least 256 tiles and one step otherwise: n = 1028 is 2 tiles wide, so K = 255 (128
    groups of two, the last one half filled: 256 tiles) takes two and K = 254 (127 groups: 254 tiles) takes one; every shape above is below the threshold.
    With three slabs the blocks of both stride over their tiles"""
    for family, head, act in (("cartpole", G.PPO, G.TANH_FAST), ("pendulum", G.PPO, G.TANH), ("lunar_lander", G.VALUE, G.TANH_FAST)):
        run(family, K, 1028, 17, act, head)
    run("acrobot", K, 1028, 17, G.TANH_FAST, slabs=3)


@pytest.mark.parametrize("family", ("cartpole", "pendulum", "lunar_lander"))
def test_one_per_lane(family):
    """n = 1030 is no multiple of 4; env_first = 1; an obs buffer 4 bytes off a 16-byte boundary"""
    for K in (1, 17):
        run(family, K, 1030, 17, G.TANH_FAST)
    run(family, 2, N, 17, G.RELU, first=1, count=N - 1)
    run(family, 2, N, 64, G.TANH, text=True, first=1, count=5)   # B = 10: one partly filled wave
    run(family, 17, N, 17, G.TANH_FAST, mis_obs=1)


@pytest.mark.parametrize("family,head", (("cartpole", G.PPO), ("pendulum", G.PPO), ("lunar_lander", G.VALUE)))
def test_slices(family, head):
    """(4, 1024) and (1028, 1024) of n = 2052, weighted by B, give the gradient of (4, 2048); with a NaN in every input word outside the slice the words are the same"""
    c = G.case(family, 2, N, 17, G.TANH_FAST, head)
    parts = []
    for first in (4, 1028):
        b = Call(c, first, 1024)
        b.launch()
        plain = b.check(f"{family} slice {first}")
        p = Call(c, first, 1024, poison_outside=True)
        p.launch()
        got = p.result(f"{family} poisoned slice {first}")
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and same(got[0], plain[0]) and same(got[1], plain[1])
        parts.append(plain)
    whole = G.grad64(c, 4, 2048)
    grad = (parts[0][0].astype(np.float64) + parts[1][0]) / 2
    stats = (parts[0][1].astype(np.float64) + parts[1][1]) / 2 * np.array([1, 1, 1, 1, 1, 2, 1, 1])
    assert G.within(grad, stats, whole)[0]
    one = Call(c, 4, 2048)
    one.launch()
    one.check(f"{family} (4, 2048)", whole)


@pytest.mark.parametrize("slabs", (1, 2, 3, None), ids=("1", "2", "3", "best"))
def test_workspace_sizes(slabs):
    """a workspace of one, two and three slabs (the blocks stride over the 9 x 5 tiles of K = 17) and best_bytes; nothing at or beyond workspace_bytes is written"""
    for family, head, H in (("cartpole", G.PPO, 64), ("pendulum", G.PPO, 17), ("cartpole", G.VALUE, 17), ("lunar_lander", G.PPO, 64)):
        run(family, 17, N, H, G.TANH_FAST, head, slabs=slabs)
    run("cartpole", 17, 1030, 17, G.RELU, slabs=slabs)


def test_workspace_query():
    for family in R.ALL:
        D, A = R.dims(family)
        for H in (1, 64):
            lo, hi = env_of(family).grad_workspace_bytes(H)
            assert lo == 8 * (G.n_params(D, A, H) + 8) and hi == 1024 * lo and lo == G.check_lib().grad_slab_bytes_of(D, A, H)
    lib, a, b = _lib.load(), _lib.C.c_size_t(), _lib.C.c_size_t()
    for kind, hidden, pa, pb, needle in ((99, 8, a, b, "kind"), (mg.CARTPOLE, 0, a, b, "hidden"), (mg.CARTPOLE, 65, a, b, "hidden"), (mg.CARTPOLE, 8, None, b, "min_bytes"),
                                         (mg.CARTPOLE, 8, a, None, "best_bytes")):
        st = lib.mgym_grad_workspace_bytes(kind, hidden, None if pa is None else _lib.C.byref(pa), None if pb is None else _lib.C.byref(pb))
        msg = lib.mgym_last_error().decode()
        assert st == _lib.ERR_BAD_ARG and msg.startswith("mgym_grad_workspace_bytes:") and needle in msg, msg


@pytest.mark.parametrize("family,head", (("cartpole", G.PPO), ("pendulum", G.PPO), ("acrobot", G.VALUE)))
def test_determinism(family, head):
    """the same call twice, and once through a captured graph: identical words"""
    c = G.case(family, 17, N, 64, G.TANH_FAST, head)
    out = []
    for mode in ("eager", "eager", "graph"):
        b = Call(c, slabs=3 if mode == "graph" else None)
        if mode == "graph":
            e = b.env
            g = e.graph_capture(b.launch)
            try:
                e.sync()
                assert b.grad.untouched() and b.stats.untouched() and b.ws.untouched()   # capture launches nothing
                e.graph_launch(g)
                first = b.result("graph replay")
                e.graph_launch(g)
                assert all(same(x, y) for x, y in zip(first, b.result("second replay")))
            finally:
                e.graph_destroy(g)
            eager = Call(c, slabs=3)
            eager.launch()
            assert all(same(x, y) for x, y in zip(first, eager.result("eager, three slabs")))
        else:
            b.launch()
            out.append(b.result(mode))
    assert same(out[0][0], out[1][0]) and same(out[0][1], out[1][1])


@pytest.mark.parametrize("family", ("cartpole", "acrobot", "pendulum"))
def test_exact_identities(family):
    for act in (G.TANH_FAST, G.RELU):
        c = G.case(family, 17, N, 17, act)
        b = Call(c)
        # logp_old from the device's own log-probability call with the same weights: the ratio is exactly 1
        old = Guarded(c.K * c.n)
        b.env.logprob_mlp_device(c.pol, c.H, 0, act, "gauss" if c.gauss else "sample", c.sigma, c.K, b.obs_first, b.obs, b.actions, old)
        b.launch(x0=old)
        grad, stats = b.result("unchanged weights")
        assert same(stats[2:5], np.array([0.0, 0.0, 1.0], F)) and np.isfinite(grad).all() and np.abs(grad).max() > 0
        assert same(old.payload((c.K, c.n)), R.logprob_mlp(c.pol, c.D, c.A, (c.H,), act, c.obs_first, c.obs, c.actions, c.sigma))
        # no advantage, no entropy bonus: no gradient
        b = Call(c)
        b.launch(x1=Guarded(c.K * c.n, 0, np.zeros((c.K, c.n), F)), ent_coef=0.0)
        grad, stats = b.result("adv = 0")
        assert (grad == 0).all() and stats[0] == 0
        # every env-step clipped
        cc = G.case(family, 17, N, 17, act, all_clipped=True)
        b = Call(cc)
        b.launch(ent_coef=0.0)
        grad, stats = b.result("all clipped")
        assert (grad == 0).all() and stats[3] == F(1.0)
        b = Call(cc)   # and with the bonus the gradient is the entropy term alone: grad64 with g = 0
        b.launch()
        b.check("all clipped, entropy bonus")


@pytest.mark.parametrize("family", ("cartpole", "lunar_lander"))
def test_critic(family):
    for K in KS:
        for H in HS:
            for act in G.ACTS:
                run(family, K, N, H, act, G.VALUE)
    run(family, 17, 1030, 17, G.TANH_FAST, G.VALUE)
    run(family, 2, N, 17, G.RELU, G.VALUE, first=1, count=N - 1)
    run(family, 2, N, 17, G.TANH, G.VALUE, mis_obs=1)


def test_host_array_forms():
    c = G.case("cartpole", 2, N, 17, G.TANH_FAST)
    w = R.actor("cartpole", (17,))[1]
    grad, stats = env_of("cartpole").ppo_grad_mlp(w, c.obs_first, c.obs, c.actions, c.x0, c.x1, "tanh_fast", clip=c.clip, ent_coef=c.ent_coef, env_slice=(4, 1024))
    assert G.within(grad, stats, G.grad64(c, 4, 1024))[0]
    v = G.case("cartpole", 2, N, 17, G.RELU, G.VALUE)
    import value_ref
    grad, stats = env_of("cartpole").value_grad_mlp(value_ref.critic("cartpole", (17,))[1], v.obs_first, v.obs, v.x0, "relu", workspace_bytes=2 * 8 * (G.n_params(4, 1, 17) + 8))
    assert G.within(grad, stats, G.grad64(v))[0]


def test_torch():
    """TorchVecEnv.ppo_grad_mlp / value_grad_mlp against torch's f32 device autograd of the textbook loss: within (GRAD_BOUND + TORCH32_BOUND) S_w, the second the
    measured distance of torch's own f32 pass from float64 (test_grad_host.py)"""
    torch = pytest.importorskip("torch")
    from modurl_gym_amd.torch_env import TorchVecEnv
    from test_grad_host import textbook_loss
    import mlp_ref
    for family, head, act in (("cartpole", G.PPO, G.TANH), ("pendulum", G.PPO, G.RELU), ("lunar_lander", G.VALUE, G.TANH)):
        c = G.case(family, 17, N, 64, act, head)
        env = TorchVecEnv(families.KIND[family], N)
        dev = env.device
        w = [torch.from_numpy(np.array(x)).to(dev) for x in mlp_ref.split(c.pol, c.D, c.A, c.H)]
        t = lambda a, dt=torch.float32: torch.from_numpy(np.array(a)).to(dev).to(dt)
        name = R.ACT_NAMES[act]
        if head == G.VALUE:
            grads, stats = env.value_grad_mlp(w, t(c.obs_first), t(c.obs), t(c.x0), activation=name)
        else:
            acts = t(c.actions) if c.gauss else t(c.actions.astype(np.int32), torch.int32)
            grads, stats = env.ppo_grad_mlp(w, t(c.obs_first), t(c.obs), acts, t(c.x0), t(c.x1), activation=name, sigma=c.sigma, clip=c.clip, ent_coef=c.ent_coef)
        assert [tuple(g.shape) for g in grads[:4]] == [tuple(x.shape) for x in w] and len(grads) == (5 if c.gauss else 4) and stats.shape == (8,)
        params = [x.clone().requires_grad_(True) for x in w] + [torch.tensor([np.log(c.sigma)], dtype=torch.float32, device=dev, requires_grad=True)]

        class OnDevice:   # textbook_loss with its inputs moved to the device
            def __getattr__(self, k):
                return getattr(torch, k)

            @staticmethod
            def from_numpy(a):
                return torch.from_numpy(a).to(dev)
        loss = textbook_loss(OnDevice(), c, params, torch.float32)
        loss.backward()
        ref = G.grad64(c)
        auto = np.concatenate([(p.grad if p.grad is not None else torch.zeros_like(p)).detach().cpu().double().numpy().ravel() for p in params])
        if not c.gauss:
            auto[-1] = 0.0
        got = np.concatenate([g.detach().cpu().double().numpy().ravel() for g in grads] + ([] if c.gauss else [np.zeros(1)]))
        worst, exact = G.worst(got, auto, ref.S_grad)
        print(f"{family} {head}: largest |device - torch f32 autograd| / S = {worst:.3g}, bound {G.GRAD_BOUND + G.TORCH32_BOUND:.3g}")
        assert worst <= G.GRAD_BOUND + G.TORCH32_BOUND
        assert G.within(got, stats.cpu().numpy(), ref)[0]
        env.close()


def test_errors():
    """every refusal names its entry point and its argument, launches nothing and leaves the handle usable"""
    c, v = G.case("cartpole", 2, N, 17, G.RELU), G.case("cartpole", 2, N, 17, G.RELU, G.VALUE)
    b, e = Call(c), env_of("cartpole")
    lo, _ = e.grad_workspace_bytes(17)
    nan, inf = float("nan"), float("inf")
    IPOL, IH, IACT, IHEAD, ISIG, IK, IFIRST, ICOUNT, IOF, IOBS, IA, IOLD, IADV, ICLIP, IENT, IWS, IWB, IG, IS = range(19)
    good = [c.pol, 17, _lib.ACT_RELU, _lib.HEAD_SAMPLE, nan, 2, 0, N, b.obs_first, b.obs, b.actions, b.x0, b.x1, 0.2, 0.01, b.ws, b.ws_bytes, b.grad, b.stats]
    ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.data_ptr())

    def ppo(repl):
        a = list(good)
        for k, val in repl.items():
            a[k] = val
        fp = None if a[IPOL] is None else np.ascontiguousarray(a[IPOL], F).ctypes.data_as(_lib.C.POINTER(_lib.C.c_float))
        return lambda: mg.envs._check(e._lib.mgym_ppo_grad_mlp(e._h, fp, *a[IH: ICOUNT + 1], *(ptr(x) for x in a[IOF: IADV + 1]), a[ICLIP], a[IENT], ptr(a[IWS]), a[IWB],
                                                               ptr(a[IG]), ptr(a[IS])))
    rows = [({IK: 0}, "K"), ({IK: -3}, "K"), ({IPOL: None}, "policy"), ({IOF: None}, "obs_first"), ({IOBS: None}, "obs"), ({IA: None}, "actions"),
            ({IOLD: None}, "logp_old"), ({IADV: None}, "adv"), ({IWS: None}, "workspace"), ({IG: None}, "grad_out"), ({IS: None}, "stats_out"),
            ({IH: 0}, "hidden"), ({IH: 65}, "hidden"), ({IACT: 2}, "activation"), ({IACT: 4}, "activation"), ({IACT: -1}, "activation"),
            ({IHEAD: _lib.HEAD_GREEDY}, "head", "MGYM_HEAD_GREEDY"), ({IHEAD: 3}, "head"), ({IHEAD: _lib.HEAD_GAUSS, ISIG: 0.5}, "head", "MGYM_HEAD_GAUSS", "CartPole"),
            ({ICOUNT: 0}, "env_count"), ({IFIRST: 1}, "env_first", "env_count", "n_envs"), ({IFIRST: N, ICOUNT: 1}, "n_envs"), ({IFIRST: 2 ** 64 - 1, ICOUNT: 2}, "n_envs"),
            ({ICLIP: nan}, "clip"), ({ICLIP: -0.1}, "clip"), ({ICLIP: 1.0}, "clip"), ({ICLIP: inf}, "clip"), ({IENT: nan}, "ent_coef"), ({IENT: inf}, "ent_coef"),
            ({IENT: -inf}, "ent_coef"), ({IWB: lo - 1}, "workspace_bytes", "min_bytes"), ({IWB: 0}, "workspace_bytes"), ({IWS: b.ws.ptr + 8}, "workspace", "16-byte aligned"),
            ({IOF: b.obs_first.ptr + 2}, "obs_first", "4-byte aligned"), ({IOBS: b.obs.ptr + 1}, "obs", "4-byte aligned"), ({IA: b.actions.ptr + 2}, "actions", "4-byte"),
            ({IOLD: b.x0.ptr + 3}, "logp_old", "4-byte aligned"), ({IADV: b.x1.ptr + 1}, "adv", "4-byte aligned"), ({IG: b.grad.ptr + 2}, "grad_out", "4-byte aligned"),
            ({IS: b.stats.ptr + 1}, "stats_out", "4-byte aligned"), ({IG: b.obs.ptr}, "grad_out", "obs"), ({IS: b.x1.ptr}, "stats_out", "adv"),
            ({IS: b.x0.ptr}, "stats_out", "logp_old"), ({IWS: b.obs_first.ptr}, "workspace", "obs_first"), ({IG: b.actions.ptr}, "grad_out", "actions"),
            ({IS: b.grad.ptr}, "stats_out", "grad_out"), ({IG: b.ws.ptr}, "grad_out", "workspace"), ({IS: b.ws.ptr}, "stats_out", "workspace"),
            # two faults: the earlier group's is the one reported — K, the NULLs, width and activation, head and sigma, the call's own checks, alignment, aliasing
            ({IK: 0, IPOL: None}, "K must be"), ({IG: None, IH: 0}, "grad_out is NULL"), ({IH: 0, IHEAD: 3}, "hidden must be"),
            ({IHEAD: 3, IOBS: b.obs.ptr + 1}, "head must be"), ({IHEAD: 3, ICOUNT: 0}, "head must be"), ({IWB: lo - 1, IOBS: b.obs.ptr + 1}, "workspace_bytes is below"),
            ({IOBS: b.obs.ptr + 1, IG: b.actions.ptr}, "obs must be 4-byte aligned")]
    state = e.get_state()
    for repl, *needles in rows:
        bad_arg(ppo(repl), "mgym_ppo_grad_mlp", *needles)
    e.sync()
    assert b.grad.untouched() and b.stats.untouched() and b.ws.untouched() and same(e.get_state(), state)
    ppo({})()
    b.check("after the refused calls")
    # the continuous side: the sample head, and every sigma that has no density
    p = Call(G.case("pendulum", 2, N, 17, G.RELU))
    for repl, *needles in (({"head": "sample"}, "head", "MGYM_HEAD_SAMPLE", "Pendulum"), ({"sigma": 0.0}, "sigma"), ({"sigma": -1.0}, "sigma"), ({"sigma": nan}, "sigma"),
                           ({"sigma": inf}, "sigma"), ({"sigma": 1e-45}, "sigma")):
        a = dict(head="gauss", sigma=0.5)
        a.update(repl)
        bad_arg(lambda: p.env.ppo_grad_mlp_device(p.c.pol, 17, "relu", a["head"], a["sigma"], 2, 0, N, p.obs_first, p.obs, p.actions, p.x0, p.x1, 0.2, 0.0, p.ws, p.ws_bytes,
                                                  p.grad, p.stats), "mgym_ppo_grad_mlp", *needles)
    assert p.grad.untouched()
    # the critic's call
    q = Call(v)
    vgood = [v.pol, 17, _lib.ACT_RELU, 2, 0, N, q.obs_first, q.obs, q.x0, q.ws, q.ws_bytes, q.grad, q.stats]

    def val(repl):
        a = list(vgood)
        for k, x in repl.items():
            a[k] = x
        fp = None if a[0] is None else np.ascontiguousarray(a[0], F).ctypes.data_as(_lib.C.POINTER(_lib.C.c_float))
        return lambda: mg.envs._check(e._lib.mgym_value_grad_mlp(e._h, fp, *a[1:6], *(ptr(x) for x in a[6:10]), a[10], ptr(a[11]), ptr(a[12])))
    for repl, *needles in (({3: 0}, "K"), ({0: None}, "critic"), ({6: None}, "obs_first"), ({7: None}, "obs"), ({8: None}, "ret"), ({9: None}, "workspace"),
                           ({11: None}, "grad_out"), ({12: None}, "stats_out"), ({1: 65}, "hidden"), ({2: 2}, "activation"), ({5: 0}, "env_count"), ({4: 5}, "n_envs"),
                           ({10: 8}, "workspace_bytes"), ({9: q.ws.ptr + 4}, "workspace", "16-byte"), ({8: q.x0.ptr + 2}, "ret", "4-byte aligned"),
                           ({11: q.x0.ptr}, "grad_out", "ret"), ({12: q.grad.ptr}, "stats_out", "grad_out"), ({9: q.obs.ptr}, "workspace", "obs"),
                           ({3: 0, 0: None}, "K must be"), ({11: None, 1: 0}, "grad_out is NULL"), ({1: 0, 5: 0}, "hidden must be"),   # two faults, as above
                           ({10: 8, 7: q.obs.ptr + 1}, "workspace_bytes is below"), ({7: q.obs.ptr + 1, 11: q.x0.ptr}, "obs must be 4-byte aligned")):
        bad_arg(val(repl), "mgym_value_grad_mlp", *needles)
    e.sync()
    assert q.grad.untouched() and q.ws.untouched()
    val({})()
    q.check("the critic after the refused calls")


def test_no_environments():
    e = mg.VecEnv(mg.CARTPOLE, 0)
    x, pol = mg.DeviceArray(4096, F), R.actor("cartpole", (17,))[0]
    p = [x.ptr + 256 * k for k in range(8)]
    e.ppo_grad_mlp_device(pol, 17, "relu", "sample", 0.0, 3, 0, 0, p[0], p[1], p[2], p[3], p[4], 0.2, 0.0, p[5], 4096, p[6], p[7])   # MGYM_OK without a launch
    with pytest.raises(mg.MgymError):
        e.ppo_grad_mlp_device(pol, 17, "relu", "sample", 0.0, 0, 0, 0, p[0], p[1], p[2], p[3], p[4], 0.2, 0.0, p[5], 4096, p[6], p[7])   # ... after the argument checks
    e.close()
