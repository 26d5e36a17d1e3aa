"""mgym_ppo_grad_mlp / mgym_value_grad_mlp and mgym_ppo_grad_mlp2 / mgym_value_grad_mlp2 on the device against the float64 restatement (tests/grad_ref.py:
grad64), every gradient word within the depth's gradient bound x S_w and every statistic within its statistics bound x S_w — S_w the word's mean absolute
per-env-step term, the bounds 4 x what the f32 text itself is from float64 (test_grad_host.py; GRAD_BOUND / STAT_BOUND and GRAD2_BOUND / STAT2_BOUND) — and a
word whose terms are all zero exactly zero.  A case's `widths`, (H,) or (H1, H2), choose the entry points; checks(depth) makes the tests of one depth:
this file runs the one-layer ones under their names, tests/test_gpu_grad2_mlp.py the two-layer ones.

One layer.  One case per family of test_one_per_lane is a batch of 10 env-steps (one partly filled wave), which is compared with the f32 text summed in float64
(grad_ref.grad32) under the same bounds: the text's own distance from float64 does not average out over 10 terms as it does at the batch sizes the bounds were
measured at.  Shapes: n = 2052 is two 1024-environment tiles of the four-per-lane kernel plus one lane; n = 1030, env_first = 1 and an obs buffer 4 bytes off a
16-byte boundary take the one-environment-per-lane kernel; K = 1, 2 and 17 leave a partial group of steps, K = 254 and 255 at n = 1028 stand on the two sides
of the tile count at which the four-per-lane kernel goes from one step per lane to two.

Two layers.  The bounds are wide (a second layer behind a ReLU makes words of one near-kink term), so the K = 1 and K = 2 cases, the one-per-lane batch of 10
env-steps and the slices are also held against the f32 text summed in float64 (grad_ref.grad32) under grad_ref.SUM_BOUND, which the number formats give: the
device differs from that text by its sums alone.  Shapes: the kernels' tile is 256 lanes x 4 env-steps (four environments of one step, or one environment at
four steps) for every K and n — the launch has no threshold between forms — so n = 2052 is two tiles plus one lane of the four-per-lane form; K = 1, 2 and 17
give one tile row, and in the one-per-lane form (n = 1030, env_first = 1, an obs buffer 4 bytes off a 16-byte boundary) a partly filled group of four steps
(K = 1, 2: 1 and 2 of 4; K = 17: four whole groups and 1 of 4).  Widths: (64, 64) the whole of every chain and tile; (17, 9) one whole 16-block plus one unit,
and a partial block; (1, 1); (8, 64) and (64, 17) the pack's chunk-of-8 tail and uneven block counts in both operands of the products.

grad_out, stats_out and the workspace are poisoned slabs between guards: every output word must have been written, no guard and no word at or beyond
workspace_bytes may have been, and the inputs are untouched.  A workspace of one, two or three slabs makes the blocks stride over the tiles."""
import functools

import numpy as np
import pytest

import device_buffers
import families
import grad_ref as G
import logprob_ref as R
import modurl_gym_amd as mg
import value_ref
from modurl_gym_amd import _lib
from words import same

pytestmark = pytest.mark.gpu

F = np.float32
N = 2052
KS = (1, 2, 17)
HS = {1: ((1,), (17,), (64,)), 2: G.WIDTHS}
MID = {1: (17,), 2: (17, 9)}
WIDE = {1: (64,), 2: (64, 64)}
Guarded = functools.partial(device_buffers.Guarded, fill=R.POISON)
bad_arg = device_buffers.bad_arg


@functools.lru_cache(maxsize=None)
def _env(family, n):
    return mg.VecEnv(families.KIND[family], n)


def env_of(family, n=N):
    """the one handle of a family and a population (its stream is the one every call on it is ordered on)"""
    return _env(family, n)


def workspace_bytes(env, widths):
    return env.grad_workspace_bytes(*widths) if len(widths) == 1 else env.grad_workspace_bytes2(*widths)


class Call:
    """the device buffers of one gradient call, of either depth, on the inputs of a grad_ref case"""

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
        self.P = G.n_params(c.D, c.A, c.widths)
        lo, hi = workspace_bytes(self.env, c.widths)
        self.ws_bytes = hi if slabs is None else slabs * lo + 8   # (the 8 bytes are no slab: they are never written)
        self.ws, self.grad, self.stats = Guarded((self.ws_bytes + 3) // 4), Guarded(self.P + 1), Guarded(8)

    def _poisoned(self, a):
        a = np.array(a)
        keep = np.zeros(a.shape[-1], bool)
        keep[self.first: self.first + self.count] = True
        nan = np.uint32(0x7FC00001) if a.dtype == np.uint32 else F(np.nan)
        return np.where(keep, a, nan).astype(a.dtype)

    def launch(self, **kw):
        """the call of the case's head and depth; pol, x0, x1, clip and ent_coef may be replaced"""
        c, e = self.c, self.env
        two = "2" if len(c.widths) == 2 else ""
        a = dict(pol=c.pol, x0=self.x0, x1=self.x1, clip=c.clip, ent_coef=c.ent_coef)
        a.update(kw)
        if c.head == G.VALUE:
            getattr(e, f"value_grad_mlp{two}_device")(a["pol"], *c.widths, c.act, c.K, self.first, self.count, self.obs_first, self.obs, a["x0"], self.ws, self.ws_bytes,
                                                      self.grad, self.stats)
        else:
            getattr(e, f"ppo_grad_mlp{two}_device")(a["pol"], *c.widths, c.act, "gauss" if c.gauss else "sample", c.sigma, c.K, self.first, self.count, self.obs_first,
                                                    self.obs, self.actions, a["x0"], a["x1"], a["clip"], a["ent_coef"], self.ws, self.ws_bytes, self.grad, self.stats)

    def result(self, what):
        self.env.sync()
        grad, stats = self.grad.payload((self.P + 1,)), self.stats.payload((8,))
        assert (grad != R.POISON).all() and (stats != R.POISON).all(), f"{what}: an output word was not written"
        assert self.grad.guards_hold() and self.stats.guards_hold() and self.ws.guards_hold(), f"{what}: a guard word was written"
        assert all(b is None or b.untouched() for b in (self.obs_first, self.obs, self.actions, self.x0, self.x1)), f"{what}: an input was written"
        return grad.view(F).copy(), stats.view(F).copy()

    def check(self, what, ref=None, extra=0.0, sums=False):
        """within the depth's bounds (+ extra) of ref, grad64's unless given; sums: also within SUM_BOUND of the f32 text summed in float64"""
        grad, stats = self.result(what)
        ref = G.grad64(self.c, self.first, self.count) if ref is None else ref
        b = ref.bounds
        ok, (wg, ws) = G.within(grad, stats, ref, extra)
        print(f"{what}: largest |device - grad64| / S: gradient {wg:.3g} (bound {b.grad:.3g}), statistics {ws:.3g} (bound {b.stat:.3g})")
        assert ok, f"{what}: gradient {wg:.3g} of {b.grad:.3g}, statistics {ws:.3g} of {b.stat:.3g}, or a word that must be exact is not"
        if sums:
            tg, ts = G.grad32(self.c, self.first, self.count)
            wg, zg = G.worst(grad, tg, ref.S_grad)
            ws, zs = G.worst(stats[:5], ts[:5], ref.S_stats[:5])
            print(f"{what}: largest |device - grad32| / S: gradient {wg:.3g}, statistics {ws:.3g} (bound {G.SUM_BOUND:.3g})")
            assert wg <= G.SUM_BOUND and ws <= G.SUM_BOUND and zg and zs, f"{what}: the sums: gradient {wg:.3g}, statistics {ws:.3g} of {G.SUM_BOUND:.3g}"
        return grad, stats


def run(family, K, n, widths, act, head=G.PPO, text=False, sums=False, **kw):
    """text: the yardstick is the f32 text summed in float64 (grad_ref.grad32) with grad64's S — for a batch of a few env-steps, where the text's own distance
    from float64 does not average out as it does at the batch sizes the bounds were measured at, and the device differs from the text by the order of its sums
    only.  sums: Call.check's"""
    c = G.case(family, K, n, widths, act, head)
    b = Call(c, **kw)
    b.launch()
    ref = None
    if text:
        ref = G.grad64(c, b.first, b.count)
        ref.grad, ref.stats = (x.astype(np.float64) for x in G.grad32(c, b.first, b.count))
    return b.check(f"{family} {head} K={K} n={n} widths={widths} act={act} {kw}", ref, sums=sums)


POINTERS = ("obs_first", "obs", "actions", "logp_old", "adv", "ret", "workspace", "grad_out", "stats_out")


def c_call(e, name, good, repl):
    """the C entry point `name` on the arguments `good` (in the declaration's order, the weights first) with `repl` replaced"""
    a = dict(good)
    a.update(repl)
    weights, *rest = a.items()
    fp = None if weights[1] is None else np.ascontiguousarray(weights[1], F).ctypes.data_as(_lib.C.POINTER(_lib.C.c_float))
    ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.data_ptr())
    return lambda: mg.envs._check(getattr(e._lib, name)(e._h, fp, *(ptr(x) if k in POINTERS else x for k, x in rest)))


def checks(depth):
    """the device tests of the gradient calls with `depth` hidden layers, by name: tests/test_gpu_grad_mlp.py takes depth 1, tests/test_gpu_grad2_mlp.py depth 2"""
    @pytest.mark.parametrize("K", KS)
    @pytest.mark.parametrize("family", R.ALL)
    def test_four_per_lane(family, K):
        for widths in HS[depth]:
            for act in G.ACTS[depth]:
                run(family, K, N, widths, act, sums=depth == 2 and K <= 2)

    if depth == 1:
        @pytest.mark.parametrize("K", (254, 255))
        def test_both_step_counts_of_the_four_per_lane_form(K):
            """the one-layer four-per-lane kernel takes two steps per lane when that gives at least 256 tiles and one step otherwise: n = 1028 is 2 tiles wide, so
            K = 255 (128 groups of two, the last one half filled: 256 tiles) takes two and K = 254 (127 groups: 254 tiles) takes one; every shape above is below the
            threshold.  With three slabs the blocks of both stride over their tiles"""
            for family, head, act in (("cartpole", G.PPO, G.TANH_FAST), ("pendulum", G.PPO, G.TANH), ("lunar_lander", G.VALUE, G.TANH_FAST)):
                run(family, K, 1028, (17,), act, head)
            run("acrobot", K, 1028, (17,), G.TANH_FAST, slabs=3)

    @pytest.mark.parametrize("family", ("cartpole", "pendulum", "lunar_lander"))
    def test_one_per_lane(family):
        """n = 1030 is no multiple of 4; env_first = 1; an obs buffer 4 bytes off a 16-byte boundary; one batch of 10 env-steps (one partly filled wave) against
        the f32 text summed in float64 — the text's own distance from float64 does not average out over 10 terms"""
        if depth == 1:
            for K in (1, 17):
                run(family, K, 1030, (17,), G.TANH_FAST)
            run(family, 2, N, (17,), G.RELU, first=1, count=N - 1)
            run(family, 2, N, (64,), G.TANH, text=True, first=1, count=5)   # B = 10
            run(family, 17, N, (17,), G.TANH_FAST, mis_obs=1)
        else:
            for K in (1, 2, 17):
                run(family, K, 1030, (17, 9), G.TANH_FAST)
            run(family, 17, 1030, (64, 64), G.RELU)
            run(family, 2, N, (64, 17), G.RELU, first=1, count=N - 1)
            run(family, 2, N, (64, 64), G.TANH_FAST, text=True, sums=True, first=1, count=5)   # B = 10
            run(family, 17, N, (8, 64), G.TANH_FAST, mis_obs=1)

    @pytest.mark.parametrize("family,head", (("cartpole", G.PPO), ("pendulum", G.PPO), ("lunar_lander", G.VALUE)))
    def test_slices(family, head):
        """(4, 1024) and (1028, 1024) of n = 2052, weighted by B, give the gradient of (4, 2048); with a NaN in every input word outside the slice the words are the same"""
        c = G.case(family, 2, N, MID[depth], G.TANH_FAST, head)
        parts = []
        for first in (4, 1028):
            b = Call(c, first, 1024)
            b.launch()
            plain = b.check(f"{family} slice {first}", sums=depth == 2)
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
        one.check(f"{family} (4, 2048)", whole, sums=depth == 2)

    @pytest.mark.parametrize("slabs", (1, 2, 3, None), ids=("1", "2", "3", "best"))
    def test_workspace_sizes(slabs):
        """a workspace of one, two and three slabs (the blocks stride over the tiles of K = 17: one layer 9 x 5; two layers 17 x 3, or the 5 x 5 of the
        one-per-lane form) and best_bytes; nothing at or beyond workspace_bytes is written"""
        rows = {1: ((64,), (17,), (17,), (64,), (17,)), 2: ((64, 64), (17, 9), (8, 64), (64, 64), (64, 17))}[depth]
        for (family, head), widths in zip((("cartpole", G.PPO), ("pendulum", G.PPO), ("cartpole", G.VALUE), ("lunar_lander", G.PPO)), rows):
            run(family, 17, N, widths, G.TANH_FAST, head, slabs=slabs)
        run("cartpole", 17, 1030, rows[4], G.RELU, slabs=slabs)

    def test_workspace_query():
        for family in R.ALL:
            D, A = R.dims(family)
            for widths in ((1,), (64,)) if depth == 1 else ((1, 1), (17, 9), (64, 64)):
                lo, hi = workspace_bytes(env_of(family), widths)
                host = G.check_lib().grad_slab_bytes_of if depth == 1 else G.check_lib().grad2_slab_bytes_of
                assert lo == 8 * (G.n_params(D, A, widths) + 8) and hi == (1024 if depth == 1 else G.SLAB_CAP) * lo and lo == host(D, A, *widths)
        if depth == 2:
            return
        lib, a, b = _lib.load(), _lib.C.c_size_t(), _lib.C.c_size_t()
        for kind, hidden, pa, pb, needle in ((99, 8, a, b, "kind"), (mg.CARTPOLE, 0, a, b, "hidden"), (mg.CARTPOLE, 65, a, b, "hidden"), (mg.CARTPOLE, 8, None, b, "min_bytes"),
                                             (mg.CARTPOLE, 8, a, None, "best_bytes")):
            st = lib.mgym_grad_workspace_bytes(kind, hidden, None if pa is None else _lib.C.byref(pa), None if pb is None else _lib.C.byref(pb))
            msg = lib.mgym_last_error().decode()
            assert st == _lib.ERR_BAD_ARG and msg.startswith("mgym_grad_workspace_bytes:") and needle in msg, msg

    @pytest.mark.parametrize("family,head", (("cartpole", G.PPO), ("pendulum", G.PPO), ("acrobot", G.VALUE)))
    def test_determinism(family, head):
        """the same call twice, and once through a captured graph: identical words"""
        c = G.case(family, 17, N, WIDE[depth], G.TANH_FAST, head)
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

    if depth == 2:
        def test_a_graph_replays_each_call_with_its_own_weights():
            """one captured graph holds mgym_logprob_mlp (two layers), mgym_ppo_grad_mlp2 and mgym_value_grad_mlp2, each with other weights (seeds 0, 1 and the
            critic's): every replay gives what the three eager calls give, so no call found another's pack"""
            family, K, widths = "cartpole", 2, (17, 9)
            c, v = G.case(family, K, N, widths, G.TANH_FAST, G.PPO, 1), G.case(family, K, N, widths, G.TANH_FAST, G.VALUE)
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

    if depth == 1:
        @pytest.mark.parametrize("family", ("cartpole", "acrobot", "pendulum"))
        def test_exact_identities(family):
            for act in (G.TANH_FAST, G.RELU):
                c = G.case(family, 17, N, (17,), act)
                b = Call(c)
                # logp_old from the device's own log-probability call with the same weights: the ratio is exactly 1
                old = Guarded(c.K * c.n)
                b.env.logprob_mlp_device(c.pol, 17, 0, act, "gauss" if c.gauss else "sample", c.sigma, c.K, b.obs_first, b.obs, b.actions, old)
                b.launch(x0=old)
                grad, stats = b.result("unchanged weights")
                assert same(stats[2:5], np.array([0.0, 0.0, 1.0], F)) and np.isfinite(grad).all() and np.abs(grad).max() > 0
                assert same(old.payload((c.K, c.n)), R.logprob_mlp(c.pol, c.D, c.A, (17,), act, c.obs_first, c.obs, c.actions, c.sigma))
                # no advantage, no entropy bonus: no gradient
                b = Call(c)
                b.launch(x1=Guarded(c.K * c.n, 0, np.zeros((c.K, c.n), F)), ent_coef=0.0)
                grad, stats = b.result("adv = 0")
                assert (grad == 0).all() and stats[0] == 0
                # every env-step clipped
                cc = G.case(family, 17, N, (17,), act, all_clipped=True)
                b = Call(cc)
                b.launch(ent_coef=0.0)
                grad, stats = b.result("all clipped")
                assert (grad == 0).all() and stats[3] == F(1.0)
                b = Call(cc)   # and with the bonus the gradient is the entropy term alone: grad64 with g = 0
                b.launch()
                b.check("all clipped, entropy bonus")

    if depth == 2:
        @pytest.mark.parametrize("family", ("cartpole", "acrobot", "pendulum"))
        def test_the_exact_ratio(family):
            """logp_old from mgym_logprob_mlp (hidden2 >= 1) on the same weights: the mean ratio is exactly 1, the approximate KL and the clipped fraction exactly 0 —
            the two-layer gradient kernels' own forward pass makes the words of the forward kernels"""
            for widths in ((64, 64), (17, 9)):
                for act in G.ACTS[2]:
                    c = G.case(family, 17, N, widths, act)
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

    @pytest.mark.parametrize("family", ("cartpole", "lunar_lander"))
    def test_critic(family):
        for K in KS:
            for widths in HS[depth]:
                for act in G.ACTS[depth]:
                    run(family, K, N, widths, act, G.VALUE, sums=depth == 2 and K == 2 and widths != (64, 64))
        if depth == 1:
            run(family, 17, 1030, (17,), G.TANH_FAST, G.VALUE)
            run(family, 2, N, (17,), G.RELU, G.VALUE, first=1, count=N - 1)
            run(family, 2, N, (17,), G.TANH, G.VALUE, mis_obs=1)
        else:
            run(family, 17, 1030, (17, 9), G.TANH_FAST, G.VALUE)
            run(family, 2, N, (64, 17), G.RELU, G.VALUE, first=1, count=N - 1)
            run(family, 2, N, (8, 64), G.TANH_FAST, G.VALUE, mis_obs=1)

    def test_host_array_forms():
        widths, two = MID[depth], "2" if depth == 2 else ""
        c = G.case("cartpole", 2, N, widths, G.TANH_FAST)
        e = env_of("cartpole")
        actor, critic = R.actor("cartpole", widths)[1], value_ref.critic("cartpole", widths)[1]
        grad, stats = getattr(e, f"ppo_grad_mlp{two}")(actor, c.obs_first, c.obs, c.actions, c.x0, c.x1, "tanh_fast", clip=c.clip, ent_coef=c.ent_coef, env_slice=(4, 1024))
        assert G.within(grad, stats, G.grad64(c, 4, 1024))[0]
        v = G.case("cartpole", 2, N, widths, G.RELU, G.VALUE)
        grad, stats = getattr(e, f"value_grad_mlp{two}")(critic, v.obs_first, v.obs, v.x0, "relu", workspace_bytes=2 * 8 * (G.n_params(4, 1, widths) + 8))
        assert G.within(grad, stats, G.grad64(v))[0]
        if depth == 2:
            with pytest.raises(TypeError):   # the one-layer forms keep refusing six weights: pack_mlp takes four, value_grad_mlp names the layer count
                e.ppo_grad_mlp(actor, c.obs_first, c.obs, c.actions, c.x0, c.x1)
            with pytest.raises(mg.MgymError, match="one hidden layer"):
                e.value_grad_mlp(critic, v.obs_first, v.obs, v.x0)

    def test_torch():
        """TorchVecEnv.ppo_grad_mlp / value_grad_mlp (and the mlp2 forms) against torch's f32 device autograd of the textbook loss, one case per head: within
        (the depth's gradient bound + its TORCH32 bound) S_w, the second the measured distance of torch's own f32 pass from float64 (test_grad_host.py)"""
        torch = pytest.importorskip("torch")
        from modurl_gym_amd.torch_env import TorchVecEnv
        from test_grad_host import textbook_loss
        two, bounds = "2" if depth == 2 else "", G.BOUNDS[depth]
        smooth = G.TANH if depth == 1 else G.TANH_FAST
        for family, head, act in (("cartpole", G.PPO, smooth), ("pendulum", G.PPO, G.RELU), ("lunar_lander", G.VALUE, smooth)):
            c = G.case(family, 17, N, WIDE[depth], act, head)
            env = TorchVecEnv(families.KIND[family], N)
            dev = env.device
            w = [torch.from_numpy(np.array(x)).to(dev) for x in G.split(c.pol, c.D, c.A, c.widths)]
            t = lambda a, dt=torch.float32: torch.from_numpy(np.array(a)).to(dev).to(dt)
            name = R.ACT_NAMES[act]
            if head == G.VALUE:
                grads, stats = getattr(env, f"value_grad_mlp{two}")(w, t(c.obs_first), t(c.obs), t(c.x0), activation=name)
            else:
                acts = t(c.actions) if c.gauss else t(c.actions.astype(np.int32), torch.int32)
                grads, stats = getattr(env, f"ppo_grad_mlp{two}")(w, t(c.obs_first), t(c.obs), acts, t(c.x0), t(c.x1), activation=name, sigma=c.sigma, clip=c.clip,
                                                                  ent_coef=c.ent_coef)
            assert [tuple(g.shape) for g in grads[:len(w)]] == [tuple(x.shape) for x in w] and len(grads) == len(w) + (1 if c.gauss else 0) and stats.shape == (8,)
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
            print(f"{family} {head}: largest |device - torch f32 autograd| / S = {worst:.3g}, bound {bounds.grad + bounds.torch32:.3g}")
            assert worst <= bounds.grad + bounds.torch32
            assert G.within(got, stats.cpu().numpy(), ref)[0]
            env.close()

    def test_errors():
        """every refusal names its entry point and its argument, launches nothing and leaves the handle usable"""
        widths, two = MID[depth], "2" if depth == 2 else ""
        H = "hidden" if depth == 1 else "hidden1"   # the first width's name
        hidden = dict(zip((H, "hidden2"), widths))
        TANH = _lib.ACT_TANH
        c, v = G.case("cartpole", 2, N, widths, G.RELU), G.case("cartpole", 2, N, widths, G.RELU, G.VALUE)
        b, e = Call(c), env_of("cartpole")
        lo, _ = workspace_bytes(e, widths)
        one_layer = e.grad_workspace_bytes(17)[0]
        assert depth == 1 or one_layer < lo
        nan, inf = float("nan"), float("inf")
        good = dict(policy=c.pol, **hidden, activation=_lib.ACT_RELU, head=_lib.HEAD_SAMPLE, sigma=nan, K=2, env_first=0, env_count=N, obs_first=b.obs_first, obs=b.obs,
                    actions=b.actions, logp_old=b.x0, adv=b.x1, clip=0.2, ent_coef=0.01, workspace=b.ws, workspace_bytes=b.ws_bytes, grad_out=b.grad, stats_out=b.stats)
        ppo = functools.partial(c_call, e, f"mgym_ppo_grad_mlp{two}", good)
        rows = [({"K": 0}, "K"), ({"K": -3}, "K"), ({"policy": None}, "policy"), ({"obs_first": None}, "obs_first"), ({"obs": None}, "obs"), ({"actions": None}, "actions"),
                ({"logp_old": None}, "logp_old"), ({"adv": None}, "adv"), ({"workspace": None}, "workspace"), ({"grad_out": None}, "grad_out"),
                ({"stats_out": None}, "stats_out"), ({H: 0}, H), ({H: 65}, H), ({"activation": 2}, "activation"), ({"activation": 4}, "activation"),
                ({"activation": -1}, "activation"), ({"head": _lib.HEAD_GREEDY}, "head", "MGYM_HEAD_GREEDY"), ({"head": 3}, "head"),
                ({"head": _lib.HEAD_GAUSS, "sigma": 0.5}, "head", "MGYM_HEAD_GAUSS", "CartPole"), ({"env_count": 0}, "env_count"),
                ({"env_first": 1}, "env_first", "env_count", "n_envs"), ({"env_first": N, "env_count": 1}, "n_envs"), ({"env_first": 2 ** 64 - 1, "env_count": 2}, "n_envs"),
                ({"clip": nan}, "clip"), ({"clip": -0.1}, "clip"), ({"clip": 1.0}, "clip"), ({"clip": inf}, "clip"), ({"ent_coef": nan}, "ent_coef"),
                ({"ent_coef": inf}, "ent_coef"), ({"ent_coef": -inf}, "ent_coef"),
                ({"workspace_bytes": lo - 1}, "workspace_bytes", "min_bytes", f"mgym_grad_workspace_bytes{two}"), ({"workspace_bytes": 0}, "workspace_bytes"),
                ({"workspace": b.ws.ptr + 8}, "workspace", "16-byte aligned"), ({"obs_first": b.obs_first.ptr + 2}, "obs_first", "4-byte aligned"),
                ({"obs": b.obs.ptr + 1}, "obs", "4-byte aligned"), ({"actions": b.actions.ptr + 2}, "actions", "4-byte"), ({"logp_old": b.x0.ptr + 3}, "logp_old", "4-byte aligned"),
                ({"adv": b.x1.ptr + 1}, "adv", "4-byte aligned"), ({"grad_out": b.grad.ptr + 2}, "grad_out", "4-byte aligned"),
                ({"stats_out": b.stats.ptr + 1}, "stats_out", "4-byte aligned"), ({"grad_out": b.obs.ptr}, "grad_out", "obs"), ({"stats_out": b.x1.ptr}, "stats_out", "adv"),
                ({"stats_out": b.x0.ptr}, "stats_out", "logp_old"), ({"workspace": b.obs_first.ptr}, "workspace", "obs_first"), ({"grad_out": b.actions.ptr}, "grad_out", "actions"),
                ({"stats_out": b.grad.ptr}, "stats_out", "grad_out"), ({"grad_out": b.ws.ptr}, "grad_out", "workspace"), ({"stats_out": b.ws.ptr}, "stats_out", "workspace"),
                # two faults: the earlier group's is the one reported — K, the NULLs, widths and activation, head and sigma, the call's own checks, alignment, aliasing
                ({"K": 0, "policy": None}, "K must be"), ({"grad_out": None, H: 0}, "grad_out is NULL"), ({"head": 3, "obs": b.obs.ptr + 1}, "head must be"),
                ({"head": 3, "env_count": 0}, "head must be"), ({"workspace_bytes": lo - 1, "obs": b.obs.ptr + 1}, "workspace_bytes is below"),
                ({"obs": b.obs.ptr + 1, "grad_out": b.actions.ptr}, "obs must be 4-byte aligned")]
        if depth == 1:
            rows += [({H: 0, "head": 3}, "hidden must be")]
        else:
            rows += [({"hidden2": 0}, "hidden2", "mgym_ppo_grad_mlp /"), ({"hidden2": 65}, "hidden2"), ({"hidden2": -1}, "hidden2"),
                     ({"activation": TANH}, "activation", "MGYM_ACT_TANH", "two hidden layers"),
                     ({"workspace_bytes": one_layer}, "workspace_bytes", "min_bytes"),   # sized by the one-layer query for the same hidden1: too small
                     ({H: 0, "hidden2": 0}, "hidden1 must be"), ({"hidden2": 0, "activation": TANH}, "hidden2 must be"), ({"activation": TANH, "head": 3}, "MGYM_ACT_TANH")]
        state = e.get_state()
        for repl, *needles in rows:
            bad_arg(ppo(repl), f"mgym_ppo_grad_mlp{two}", *needles)
        e.sync()
        assert b.grad.untouched() and b.stats.untouched() and b.ws.untouched() and same(e.get_state(), state)
        ppo({})()
        b.check("after the refused calls")
        # the continuous side: the sample head, and every sigma that has no density
        p = Call(G.case("pendulum", 2, N, widths, G.RELU))
        sigmas = (0.0, -1.0, nan, inf, 1e-45) if depth == 1 else (0.0, nan, 1e-45)
        for repl, *needles in (({"head": "sample"}, "head", "MGYM_HEAD_SAMPLE", "Pendulum"), *(({"sigma": s}, "sigma") for s in sigmas)):
            a = dict(head="gauss", sigma=0.5)
            a.update(repl)
            bad_arg(lambda: getattr(p.env, f"ppo_grad_mlp{two}_device")(p.c.pol, *widths, "relu", a["head"], a["sigma"], 2, 0, N, p.obs_first, p.obs, p.actions, p.x0, p.x1, 0.2,
                                                                        0.0, p.ws, p.ws_bytes, p.grad, p.stats), f"mgym_ppo_grad_mlp{two}", *needles)
        assert p.grad.untouched()
        # the critic's call
        q = Call(v)
        vgood = dict(critic=v.pol, **hidden, activation=_lib.ACT_RELU, K=2, env_first=0, env_count=N, obs_first=q.obs_first, obs=q.obs, ret=q.x0, workspace=q.ws,
                     workspace_bytes=q.ws_bytes, grad_out=q.grad, stats_out=q.stats)
        val = functools.partial(c_call, e, f"mgym_value_grad_mlp{two}", vgood)
        rows = [({"K": 0}, "K"), ({"critic": None}, "critic"), ({"obs_first": None}, "obs_first"), ({"obs": None}, "obs"), ({"ret": None}, "ret"),
                ({"workspace": None}, "workspace"), ({"grad_out": None}, "grad_out"), ({"stats_out": None}, "stats_out"), ({H: 65}, H), ({"activation": 2}, "activation"),
                ({"env_count": 0}, "env_count"), ({"env_first": 5}, "n_envs"), ({"workspace_bytes": 8}, "workspace_bytes"), ({"workspace": q.ws.ptr + 4}, "workspace", "16-byte"),
                ({"ret": q.x0.ptr + 2}, "ret", "4-byte aligned"), ({"grad_out": q.x0.ptr}, "grad_out", "ret"), ({"stats_out": q.grad.ptr}, "stats_out", "grad_out"),
                ({"workspace": q.obs.ptr}, "workspace", "obs"),
                ({"K": 0, "critic": None}, "K must be"), ({"grad_out": None, H: 0}, "grad_out is NULL"), ({H: 0, "env_count": 0}, f"{H} must be"),   # two faults, as above
                ({"workspace_bytes": 8, "obs": q.obs.ptr + 1}, "workspace_bytes is below"), ({"obs": q.obs.ptr + 1, "grad_out": q.x0.ptr}, "obs must be 4-byte aligned")]
        if depth == 2:
            rows += [({"hidden2": 0}, "hidden2", "mgym_value_grad_mlp"), ({"hidden2": 65}, "hidden2"), ({"activation": TANH}, "activation", "MGYM_ACT_TANH"),
                     ({"workspace_bytes": one_layer}, "workspace_bytes", "mgym_grad_workspace_bytes2")]
        for repl, *needles in rows:
            bad_arg(val(repl), f"mgym_value_grad_mlp{two}", *needles)
        e.sync()
        assert q.grad.untouched() and q.ws.untouched()
        val({})()
        q.check("the critic after the refused calls")

    def test_no_environments():
        e = mg.VecEnv(mg.CARTPOLE, 0)
        widths = MID[depth]
        x, pol = mg.DeviceArray(4096, F), R.actor("cartpole", widths)[0]
        p = [x.ptr + 256 * k for k in range(8)]
        call = e.ppo_grad_mlp_device if depth == 1 else e.ppo_grad_mlp2_device
        call(pol, *widths, "relu", "sample", 0.0, 3, 0, 0, p[0], p[1], p[2], p[3], p[4], 0.2, 0.0, p[5], 4096, p[6], p[7])   # MGYM_OK without a launch
        with pytest.raises(mg.MgymError):
            call(pol, *widths, "relu", "sample", 0.0, 0, 0, 0, p[0], p[1], p[2], p[3], p[4], 0.2, 0.0, p[5], 4096, p[6], p[7])   # ... after the argument checks
        e.close()

    return {name: f for name, f in locals().items() if name.startswith("test_")}


globals().update(checks(1))
