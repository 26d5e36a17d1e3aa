"""mgym_ppo_grad_mlp2 and mgym_value_grad_mlp2 on the device against the float64 restatement (tests/grad2_ref.py: grad64), every gradient word within
GRAD2_BOUND x S_w and every statistic within STAT2_BOUND x S_w — S_w the word's mean absolute per-env-step term, the bounds 4 x what the f32 text itself is
from float64 (test_grad2_host.py) — and a word whose terms are all zero exactly zero.  Those bounds are wide (a second layer behind a ReLU makes words of one
near-kink term), so the K = 1 and K = 2 cases, the one-per-lane batch of 10 env-steps and the slices are also held against the f32 text summed in float64
(grad2_ref.grad32) under grad2_ref.SUM_BOUND, which the number formats give: the device differs from that text by its sums alone.

grad_out, stats_out and the workspace are poisoned slabs between guards: every output word must have been written, no guard and no word at or beyond
workspace_bytes may have been, and the inputs are untouched.  Shapes: the kernels' tile is 256 lanes x 4 env-steps (four environments of one step, or one
environment at four steps) for every K and n — the launch has no threshold between forms — so n = 2052 is two tiles plus one lane of the four-per-lane form;
K = 1, 2 and 17 give one tile row, and in the one-per-lane form (n = 1030, env_first = 1, an obs buffer 4 bytes off a 16-byte boundary) a partly filled group
of four steps (K = 1, 2: 1 and 2 of 4; K = 17: four whole groups and 1 of 4).  Widths: (64, 64) the whole of every chain and tile; (17, 9) one whole 16-block
plus one unit, and a partial block; (1, 1); (8, 64) and (64, 17) the pack's chunk-of-8 tail and uneven block counts in both operands of the products.  A
workspace of one, two or three slabs makes the blocks stride over the tiles."""
import functools

import numpy as np
import pytest

import device_buffers
import families
import grad2_ref as G2
import logprob_ref as R
import mlp2_ref
import modurl_gym_amd as mg
import value_ref
from modurl_gym_amd import _lib
from words import same

pytestmark = pytest.mark.gpu

F = np.float32
N = 2052
KS = (1, 2, 17)
Guarded = functools.partial(device_buffers.Guarded, fill=R.POISON)
bad_arg = device_buffers.bad_arg


@functools.lru_cache(maxsize=None)
def _env(family, n):
    return mg.VecEnv(families.KIND[family], n)


def env_of(family, n=N):
    """the one handle of a family and a population (its stream is the one every call on it is ordered on)"""
    return _env(family, n)


class Call:
    """the device buffers of one two-layer gradient call on the inputs of a grad2_ref case"""

    def __init__(self, c, first=None, count=None, slabs=None, mis_obs=0, poison_outside=False, ws_bytes=None):
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
        self.P = G2.n_params(c.D, c.A, c.H1, c.H2)
        lo, hi = self.env.grad_workspace_bytes2(c.H1, c.H2)
        self.ws_bytes = (hi if slabs is None else slabs * lo + 8) if ws_bytes is None else ws_bytes   # (the 8 bytes are no slab: they are never written)
        self.ws, self.grad, self.stats = Guarded((self.ws_bytes + 3) // 4), Guarded(self.P + 1), Guarded(8)

    def _poisoned(self, a):
        a = np.array(a)
        keep = np.zeros(a.shape[-1], bool)
        keep[self.first: self.first + self.count] = True
        nan = np.uint32(0x7FC00001) if a.dtype == np.uint32 else F(np.nan)
        return np.where(keep, a, nan).astype(a.dtype)

    def launch(self, **kw):
        c, e = self.c, self.env
        a = dict(pol=c.pol, x0=self.x0, x1=self.x1, clip=c.clip, ent_coef=c.ent_coef)
        a.update(kw)
        if c.head == G2.VALUE:
            e.value_grad_mlp2_device(a["pol"], c.H1, c.H2, c.act, c.K, self.first, self.count, self.obs_first, self.obs, a["x0"], self.ws, self.ws_bytes, self.grad,
                                     self.stats)
        else:
            e.ppo_grad_mlp2_device(a["pol"], c.H1, c.H2, c.act, "gauss" if c.gauss else "sample", c.sigma, c.K, self.first, self.count, self.obs_first, self.obs,
                                   self.actions, a["x0"], a["x1"], a["clip"], a["ent_coef"], self.ws, self.ws_bytes, self.grad, self.stats)

    def result(self, what):
        self.env.sync()
        grad, stats = self.grad.payload((self.P + 1,)), self.stats.payload((8,))
        assert (grad != R.POISON).all() and (stats != R.POISON).all(), f"{what}: an output word was not written"
        assert self.grad.guards_hold() and self.stats.guards_hold() and self.ws.guards_hold(), f"{what}: a guard word was written"
        assert all(b is None or b.untouched() for b in (self.obs_first, self.obs, self.actions, self.x0, self.x1)), f"{what}: an input was written"
        return grad.view(F).copy(), stats.view(F).copy()

    def check(self, what, ref=None, text=False):
        """within the bounds of grad64; text: also within SUM_BOUND of the f32 text summed in float64"""
        grad, stats = self.result(what)
        ref = G2.grad64(self.c, self.first, self.count) if ref is None else ref
        ok, (wg, ws) = G2.within(grad, stats, ref)
        print(f"{what}: largest |device - grad64| / S: gradient {wg:.3g} (bound {G2.GRAD2_BOUND:.3g}), statistics {ws:.3g} (bound {G2.STAT2_BOUND:.3g})")
        assert ok, f"{what}: gradient {wg:.3g} of {G2.GRAD2_BOUND:.3g}, statistics {ws:.3g} of {G2.STAT2_BOUND:.3g}, or a word that must be exact is not"
        if text:
            tg, ts = G2.grad32(self.c, self.first, self.count)
            wg, zg = G2.worst(grad, tg, ref.S_grad)
            ws, zs = G2.worst(stats[:5], ts[:5], ref.S_stats[:5])
            print(f"{what}: largest |device - grad32| / S: gradient {wg:.3g}, statistics {ws:.3g} (bound {G2.SUM_BOUND:.3g})")
            assert wg <= G2.SUM_BOUND and ws <= G2.SUM_BOUND and zg and zs, f"{what}: the sums: gradient {wg:.3g}, statistics {ws:.3g} of {G2.SUM_BOUND:.3g}"
        return grad, stats


def run(family, K, n, widths, act, head=G2.PPO, text=False, **kw):
    c = G2.case2(family, K, n, widths[0], widths[1], act, head)
    b = Call(c, **kw)
    b.launch()
    return b.check(f"{family} {head} K={K} n={n} widths={widths} act={act} {kw}", text=text)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("family", R.ALL)
def test_four_per_lane(family, K):
    for widths in G2.WIDTHS:
        for act in G2.ACTS:
            run(family, K, N, widths, act, text=K <= 2)


@pytest.mark.parametrize("family", ("cartpole", "lunar_lander"))
def test_critic(family):
    for K in KS:
        for widths in G2.WIDTHS:
            for act in G2.ACTS:
                run(family, K, N, widths, act, G2.VALUE, text=K == 2 and widths != (64, 64))
    run(family, 17, 1030, (17, 9), G2.TANH_FAST, G2.VALUE)
    run(family, 2, N, (64, 17), G2.RELU, G2.VALUE, first=1, count=N - 1)
    run(family, 2, N, (8, 64), G2.TANH_FAST, G2.VALUE, mis_obs=1)


@pytest.mark.parametrize("family", ("cartpole", "pendulum", "lunar_lander"))
def test_one_per_lane(family):
    """n = 1030 is no multiple of 4; env_first = 1; an obs buffer 4 bytes off a 16-byte boundary; one batch of 10 env-steps (one partly filled wave) against
    the f32 text summed in float64 — the text's own distance from float64 does not average out over 10 terms"""
    for K in (1, 2, 17):
        run(family, K, 1030, (17, 9), G2.TANH_FAST)
    run(family, 17, 1030, (64, 64), G2.RELU)
    run(family, 2, N, (64, 17), G2.RELU, first=1, count=N - 1)
    c = G2.case2(family, 2, N, 64, 64, G2.TANH_FAST)
    b = Call(c, 1, 5)   # B = 10
    b.launch()
    ref = G2.grad64(c, 1, 5)
    ref.grad, ref.stats = (x.astype(np.float64) for x in G2.grad32(c, 1, 5))
    b.check(f"{family} B = 10", ref, text=True)
    run(family, 17, N, (8, 64), G2.TANH_FAST, mis_obs=1)


@pytest.mark.parametrize("family,head", (("cartpole", G2.PPO), ("pendulum", G2.PPO), ("lunar_lander", G2.VALUE)))
def test_slices(family, head):
    """(4, 1024) and (1028, 1024) of n = 2052, weighted by B, give the gradient of (4, 2048); with a NaN in every input word outside the slice the words are the same"""
    c = G2.case2(family, 2, N, 17, 9, G2.TANH_FAST, head)
    parts = []
    for first in (4, 1028):
        b = Call(c, first, 1024)
        b.launch()
        plain = b.check(f"{family} slice {first}", text=True)
        p = Call(c, first, 1024, poison_outside=True)
        p.launch()
        got = p.result(f"{family} poisoned slice {first}")
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and same(got[0], plain[0]) and same(got[1], plain[1])
        parts.append(plain)
    whole = G2.grad64(c, 4, 2048)
    grad = (parts[0][0].astype(np.float64) + parts[1][0]) / 2
    stats = (parts[0][1].astype(np.float64) + parts[1][1]) / 2 * np.array([1, 1, 1, 1, 1, 2, 1, 1])
    assert G2.within(grad, stats, whole)[0]
    one = Call(c, 4, 2048)
    one.launch()
    one.check(f"{family} (4, 2048)", whole, text=True)


@pytest.mark.parametrize("slabs", (1, 2, 3, None), ids=("1", "2", "3", "best"))
def test_workspace_sizes(slabs):
    """a workspace of one, two and three slabs (the blocks stride over the 17 x 3 tiles of K = 17, or the 5 x 5 of the one-per-lane form) and best_bytes;
    nothing at or beyond workspace_bytes is written"""
    for family, head, widths in (("cartpole", G2.PPO, (64, 64)), ("pendulum", G2.PPO, (17, 9)), ("cartpole", G2.VALUE, (8, 64)), ("lunar_lander", G2.PPO, (64, 64))):
        run(family, 17, N, widths, G2.TANH_FAST, head, slabs=slabs)
    run("cartpole", 17, 1030, (64, 17), G2.RELU, slabs=slabs)


def test_workspace_query():
    for family in R.ALL:
        D, A = R.dims(family)
        for H1, H2 in ((1, 1), (17, 9), (64, 64)):
            lo, hi = env_of(family).grad_workspace_bytes2(H1, H2)
            assert lo == 8 * (G2.n_params(D, A, H1, H2) + 8) and hi == G2.SLAB_CAP * lo and lo == G2.check_lib().grad2_slab_bytes_of(D, A, H1, H2)


@pytest.mark.parametrize("family,head", (("cartpole", G2.PPO), ("pendulum", G2.PPO), ("acrobot", G2.VALUE)))
def test_determinism(family, head):
    """the same call twice, and once through a captured graph: identical words"""
    c = G2.case2(family, 17, N, 64, 64, G2.TANH_FAST, head)
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


def test_a_graph_replays_each_call_with_its_own_weights():
    """one captured graph holds mgym_logprob_mlp (two layers), mgym_ppo_grad_mlp2 and mgym_value_grad_mlp2, each with other weights (seeds 0, 1 and the
    critic's): every replay gives what the three eager calls give, so no call found another's pack"""
    family, K, widths = "cartpole", 2, (17, 9)
    c, v = G2.case2(family, K, N, *widths, G2.TANH_FAST, G2.PPO, 1), G2.case2(family, K, N, *widths, G2.TANH_FAST, G2.VALUE)
    other = R.actor(family, widths, 0)[0]
    assert not np.array_equal(other, c.pol)
    e = env_of(family)

    def three(b, q, logp):
        e.logprob_mlp_device(other, *widths, c.act, "sample", c.sigma, K, b.obs_first, b.obs, b.actions, logp)
        b.launch()
        q.launch()
    eager = (Call(c), Call(v), Guarded(K * N))
    three(*eager)
    want = (eager[0].result("eager actor"), eager[1].result("eager critic"), eager[2].payload((K, N)).copy())
    assert same(want[2], R.logprob_mlp(other, c.D, c.A, widths, c.act, c.obs_first, c.obs, c.actions, c.sigma))
    held = (Call(c), Call(v), Guarded(K * N))
    g = e.graph_capture(lambda: three(*held))
    try:
        for _ in range(2):
            e.graph_launch(g)
            got = (held[0].result("replayed actor"), held[1].result("replayed critic"), held[2].payload((K, N)).copy())
            assert all(same(x, y) for x, y in zip(got[0], want[0])) and all(same(x, y) for x, y in zip(got[1], want[1])) and same(got[2], want[2])
    finally:
        e.graph_destroy(g)
    held[0].check("the replayed actor's call")
    held[1].check("the replayed critic's call")


@pytest.mark.parametrize("family", ("cartpole", "acrobot", "pendulum"))
def test_the_exact_ratio(family):
    """logp_old from mgym_logprob_mlp (hidden2 >= 1) on the same weights: the mean ratio is exactly 1, the approximate KL and the clipped fraction exactly 0 —
    the gradient kernels' own forward pass makes the words of the forward kernels"""
    for widths in ((64, 64), (17, 9)):
        for act in G2.ACTS:
            c = G2.case2(family, 17, N, *widths, act)
            b = Call(c)
            old = Guarded(c.K * c.n)
            b.env.logprob_mlp_device(c.pol, *widths, act, "gauss" if c.gauss else "sample", c.sigma, c.K, b.obs_first, b.obs, b.actions, old)
            b.launch(x0=old)
            grad, stats = b.result("unchanged weights")
            assert same(stats[2:5], np.array([0.0, 0.0, 1.0], F)), (family, widths, act, stats)
            assert np.isfinite(grad).all() and np.abs(grad).max() > 0
            assert same(old.payload((c.K, c.n)), R.logprob_mlp(c.pol, c.D, c.A, widths, act, c.obs_first, c.obs, c.actions, c.sigma))
    # no advantage, no entropy bonus: no gradient, every word exactly zero
    b = Call(c)
    b.launch(x1=Guarded(c.K * c.n, 0, np.zeros((c.K, c.n), F)), ent_coef=0.0)
    grad, stats = b.result("adv = 0")
    assert (grad == 0).all() and stats[0] == 0


def test_host_array_forms():
    c = G2.case2("cartpole", 2, N, 17, 9, G2.TANH_FAST)
    e = env_of("cartpole")
    grad, stats = e.ppo_grad_mlp2(R.actor("cartpole", (17, 9))[1], c.obs_first, c.obs, c.actions, c.x0, c.x1, "tanh_fast", clip=c.clip, ent_coef=c.ent_coef, env_slice=(4, 1024))
    assert G2.within(grad, stats, G2.grad64(c, 4, 1024))[0]
    v = G2.case2("cartpole", 2, N, 17, 9, G2.RELU, G2.VALUE)
    grad, stats = e.value_grad_mlp2(value_ref.critic("cartpole", (17, 9))[1], v.obs_first, v.obs, v.x0, "relu", workspace_bytes=2 * 8 * (G2.n_params(4, 1, 17, 9) + 8))
    assert G2.within(grad, stats, G2.grad64(v))[0]
    with pytest.raises(TypeError):   # the one-layer forms keep refusing six weights: pack_mlp takes four, value_grad_mlp names the layer count
        e.ppo_grad_mlp(R.actor("cartpole", (17, 9))[1], c.obs_first, c.obs, c.actions, c.x0, c.x1)
    with pytest.raises(mg.MgymError, match="one hidden layer"):
        e.value_grad_mlp(value_ref.critic("cartpole", (17, 9))[1], v.obs_first, v.obs, v.x0)


def test_torch():
    """TorchVecEnv.ppo_grad_mlp2 / value_grad_mlp2 against torch's f32 device autograd of the textbook loss, one case per head: within (GRAD2_BOUND +
    TORCH32_2_BOUND) S_w, the second the measured distance of torch's own f32 pass from float64 (test_grad2_host.py)"""
    torch = pytest.importorskip("torch")
    from modurl_gym_amd.torch_env import TorchVecEnv
    from test_grad2_host import textbook_loss
    for family, head, act in (("cartpole", G2.PPO, G2.TANH_FAST), ("pendulum", G2.PPO, G2.RELU), ("lunar_lander", G2.VALUE, G2.TANH_FAST)):
        c = G2.case2(family, 17, N, 64, 64, act, head)
        env = TorchVecEnv(families.KIND[family], N)
        dev = env.device
        w = [torch.from_numpy(np.array(x)).to(dev) for x in mlp2_ref.split(c.pol, c.D, c.A, c.H1, c.H2)]
        t = lambda a, dt=torch.float32: torch.from_numpy(np.array(a)).to(dev).to(dt)
        name = R.ACT_NAMES[act]
        if head == G2.VALUE:
            grads, stats = env.value_grad_mlp2(w, t(c.obs_first), t(c.obs), t(c.x0), activation=name)
        else:
            acts = t(c.actions) if c.gauss else t(c.actions.astype(np.int32), torch.int32)
            grads, stats = env.ppo_grad_mlp2(w, t(c.obs_first), t(c.obs), acts, t(c.x0), t(c.x1), activation=name, sigma=c.sigma, clip=c.clip, ent_coef=c.ent_coef)
        assert [tuple(g.shape) for g in grads[:6]] == [tuple(x.shape) for x in w] and len(grads) == (7 if c.gauss else 6) and stats.shape == (8,)
        params = [x.clone().requires_grad_(True) for x in w] + [torch.tensor([np.log(c.sigma)], dtype=torch.float32, device=dev, requires_grad=True)]

        class OnDevice:   # textbook_loss with its inputs moved to the device
            def __getattr__(self, k):
                return getattr(torch, k)

            @staticmethod
            def from_numpy(a):
                return torch.from_numpy(a).to(dev)
        loss = textbook_loss(OnDevice(), c, params, torch.float32)
        loss.backward()
        ref = G2.grad64(c)
        auto = np.concatenate([(p.grad if p.grad is not None else torch.zeros_like(p)).detach().cpu().double().numpy().ravel() for p in params])
        if not c.gauss:
            auto[-1] = 0.0
        got = np.concatenate([g.detach().cpu().double().numpy().ravel() for g in grads] + ([] if c.gauss else [np.zeros(1)]))
        worst, _ = G2.worst(got, auto, ref.S_grad)
        print(f"{family} {head}: largest |device - torch f32 autograd| / S = {worst:.3g}, bound {G2.GRAD2_BOUND + G2.TORCH32_2_BOUND:.3g}")
        assert worst <= G2.GRAD2_BOUND + G2.TORCH32_2_BOUND
        assert G2.within(got, stats.cpu().numpy(), ref)[0]
        env.close()


def test_errors():
    """every refusal names its entry point and its argument, launches nothing and leaves the handle usable"""
    c, v = G2.case2("cartpole", 2, N, 17, 9, G2.RELU), G2.case2("cartpole", 2, N, 17, 9, G2.RELU, G2.VALUE)
    b, e = Call(c), env_of("cartpole")
    lo, _ = e.grad_workspace_bytes2(17, 9)
    one_layer = e.grad_workspace_bytes(17)[0]
    assert one_layer < lo
    nan, inf = float("nan"), float("inf")
    IPOL, IH1, IH2, IACT, IHEAD, ISIG, IK, IFIRST, ICOUNT, IOF, IOBS, IA, IOLD, IADV, ICLIP, IENT, IWS, IWB, IG, IS = range(20)
    good = [c.pol, 17, 9, _lib.ACT_RELU, _lib.HEAD_SAMPLE, nan, 2, 0, N, b.obs_first, b.obs, b.actions, b.x0, b.x1, 0.2, 0.01, b.ws, b.ws_bytes, b.grad, b.stats]
    ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.data_ptr())

    def ppo(repl):
        a = list(good)
        for k, val in repl.items():
            a[k] = val
        fp = None if a[IPOL] is None else np.ascontiguousarray(a[IPOL], F).ctypes.data_as(_lib.C.POINTER(_lib.C.c_float))
        return lambda: mg.envs._check(e._lib.mgym_ppo_grad_mlp2(e._h, fp, *a[IH1: ICOUNT + 1], *(ptr(x) for x in a[IOF: IADV + 1]), a[ICLIP], a[IENT], ptr(a[IWS]), a[IWB],
                                                                ptr(a[IG]), ptr(a[IS])))
    rows = [({IK: 0}, "K"), ({IK: -3}, "K"), ({IPOL: None}, "policy"), ({IOF: None}, "obs_first"), ({IOBS: None}, "obs"), ({IA: None}, "actions"),
            ({IOLD: None}, "logp_old"), ({IADV: None}, "adv"), ({IWS: None}, "workspace"), ({IG: None}, "grad_out"), ({IS: None}, "stats_out"),
            ({IH1: 0}, "hidden1"), ({IH1: 65}, "hidden1"), ({IH2: 0}, "hidden2", "mgym_ppo_grad_mlp /"), ({IH2: 65}, "hidden2"), ({IH2: -1}, "hidden2"),
            ({IACT: _lib.ACT_TANH}, "activation", "MGYM_ACT_TANH", "two hidden layers"), ({IACT: 2}, "activation"), ({IACT: 4}, "activation"), ({IACT: -1}, "activation"),
            ({IHEAD: _lib.HEAD_GREEDY}, "head", "MGYM_HEAD_GREEDY"), ({IHEAD: 3}, "head"), ({IHEAD: _lib.HEAD_GAUSS, ISIG: 0.5}, "head", "MGYM_HEAD_GAUSS", "CartPole"),
            ({ICOUNT: 0}, "env_count"), ({IFIRST: 1}, "env_first", "env_count", "n_envs"), ({IFIRST: N, ICOUNT: 1}, "n_envs"), ({IFIRST: 2 ** 64 - 1, ICOUNT: 2}, "n_envs"),
            ({ICLIP: nan}, "clip"), ({ICLIP: -0.1}, "clip"), ({ICLIP: 1.0}, "clip"), ({ICLIP: inf}, "clip"), ({IENT: nan}, "ent_coef"), ({IENT: inf}, "ent_coef"),
            ({IENT: -inf}, "ent_coef"), ({IWB: lo - 1}, "workspace_bytes", "min_bytes", "mgym_grad_workspace_bytes2"), ({IWB: 0}, "workspace_bytes"),
            ({IWB: one_layer}, "workspace_bytes", "min_bytes"),   # sized by the one-layer query for the same hidden1: too small
            ({IWS: b.ws.ptr + 8}, "workspace", "16-byte aligned"),
            ({IOF: b.obs_first.ptr + 2}, "obs_first", "4-byte aligned"), ({IOBS: b.obs.ptr + 1}, "obs", "4-byte aligned"), ({IA: b.actions.ptr + 2}, "actions", "4-byte"),
            ({IOLD: b.x0.ptr + 3}, "logp_old", "4-byte aligned"), ({IADV: b.x1.ptr + 1}, "adv", "4-byte aligned"), ({IG: b.grad.ptr + 2}, "grad_out", "4-byte aligned"),
            ({IS: b.stats.ptr + 1}, "stats_out", "4-byte aligned"), ({IG: b.obs.ptr}, "grad_out", "obs"), ({IS: b.x1.ptr}, "stats_out", "adv"),
            ({IS: b.x0.ptr}, "stats_out", "logp_old"), ({IWS: b.obs_first.ptr}, "workspace", "obs_first"), ({IG: b.actions.ptr}, "grad_out", "actions"),
            ({IS: b.grad.ptr}, "stats_out", "grad_out"), ({IG: b.ws.ptr}, "grad_out", "workspace"), ({IS: b.ws.ptr}, "stats_out", "workspace"),
            # two faults: the earlier group's is the one reported — K, the NULLs, widths and activation, head and sigma, the call's own checks, alignment, aliasing
            ({IK: 0, IPOL: None}, "K must be"), ({IG: None, IH1: 0}, "grad_out is NULL"), ({IH1: 0, IH2: 0}, "hidden1 must be"), ({IH2: 0, IACT: _lib.ACT_TANH}, "hidden2 must be"),
            ({IACT: _lib.ACT_TANH, IHEAD: 3}, "MGYM_ACT_TANH"), ({IHEAD: 3, IOBS: b.obs.ptr + 1}, "head must be"), ({IHEAD: 3, ICOUNT: 0}, "head must be"),
            ({IWB: lo - 1, IOBS: b.obs.ptr + 1}, "workspace_bytes is below"), ({IOBS: b.obs.ptr + 1, IG: b.actions.ptr}, "obs must be 4-byte aligned")]
    state = e.get_state()
    for repl, *needles in rows:
        bad_arg(ppo(repl), "mgym_ppo_grad_mlp2", *needles)
    e.sync()
    assert b.grad.untouched() and b.stats.untouched() and b.ws.untouched() and same(e.get_state(), state)
    ppo({})()
    b.check("after the refused calls")
    # the continuous side: the sample head, and a sigma that has no density
    p = Call(G2.case2("pendulum", 2, N, 17, 9, G2.RELU))
    for repl, *needles in (({"head": "sample"}, "head", "MGYM_HEAD_SAMPLE", "Pendulum"), ({"sigma": 0.0}, "sigma"), ({"sigma": nan}, "sigma"), ({"sigma": 1e-45}, "sigma")):
        a = dict(head="gauss", sigma=0.5)
        a.update(repl)
        bad_arg(lambda: p.env.ppo_grad_mlp2_device(p.c.pol, 17, 9, "relu", a["head"], a["sigma"], 2, 0, N, p.obs_first, p.obs, p.actions, p.x0, p.x1, 0.2, 0.0, p.ws,
                                                   p.ws_bytes, p.grad, p.stats), "mgym_ppo_grad_mlp2", *needles)
    assert p.grad.untouched()
    # the critic's call
    q = Call(v)
    vgood = [v.pol, 17, 9, _lib.ACT_RELU, 2, 0, N, q.obs_first, q.obs, q.x0, q.ws, q.ws_bytes, q.grad, q.stats]

    def val(repl):
        a = list(vgood)
        for k, x in repl.items():
            a[k] = x
        fp = None if a[0] is None else np.ascontiguousarray(a[0], F).ctypes.data_as(_lib.C.POINTER(_lib.C.c_float))
        return lambda: mg.envs._check(e._lib.mgym_value_grad_mlp2(e._h, fp, *a[1:7], *(ptr(x) for x in a[7:11]), a[11], ptr(a[12]), ptr(a[13])))
    for repl, *needles in (({4: 0}, "K"), ({0: None}, "critic"), ({7: None}, "obs_first"), ({8: None}, "obs"), ({9: None}, "ret"), ({10: None}, "workspace"),
                           ({12: None}, "grad_out"), ({13: None}, "stats_out"), ({1: 65}, "hidden1"), ({2: 0}, "hidden2", "mgym_value_grad_mlp"), ({2: 65}, "hidden2"),
                           ({3: _lib.ACT_TANH}, "activation", "MGYM_ACT_TANH"), ({3: 2}, "activation"), ({6: 0}, "env_count"), ({5: 5}, "n_envs"),
                           ({11: 8}, "workspace_bytes"), ({11: one_layer}, "workspace_bytes", "mgym_grad_workspace_bytes2"), ({10: q.ws.ptr + 4}, "workspace", "16-byte"),
                           ({9: q.x0.ptr + 2}, "ret", "4-byte aligned"), ({12: q.x0.ptr}, "grad_out", "ret"), ({13: q.grad.ptr}, "stats_out", "grad_out"),
                           ({10: q.obs.ptr}, "workspace", "obs"),
                           ({4: 0, 0: None}, "K must be"), ({12: None, 1: 0}, "grad_out is NULL"), ({1: 0, 6: 0}, "hidden1 must be"),   # two faults, as above
                           ({11: 8, 8: q.obs.ptr + 1}, "workspace_bytes is below"), ({8: q.obs.ptr + 1, 12: q.x0.ptr}, "obs must be 4-byte aligned")):
        bad_arg(val(repl), "mgym_value_grad_mlp2", *needles)
    e.sync()
    assert q.grad.untouched() and q.ws.untouched()
    val({})()
    q.check("the critic after the refused calls")


def test_no_environments():
    e = mg.VecEnv(mg.CARTPOLE, 0)
    x, pol = mg.DeviceArray(4096, F), R.actor("cartpole", (17, 9))[0]
    p = [x.ptr + 256 * k for k in range(8)]
    e.ppo_grad_mlp2_device(pol, 17, 9, "relu", "sample", 0.0, 3, 0, 0, p[0], p[1], p[2], p[3], p[4], 0.2, 0.0, p[5], 4096, p[6], p[7])   # MGYM_OK without a launch
    with pytest.raises(mg.MgymError):
        e.ppo_grad_mlp2_device(pol, 17, 9, "relu", "sample", 0.0, 0, 0, 0, p[0], p[1], p[2], p[3], p[4], 0.2, 0.0, p[5], 4096, p[6], p[7])   # ... after the argument checks
    e.close()
