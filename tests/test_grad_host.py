"""No-GPU checks of the words of mgym_ppo_grad_mlp / mgym_value_grad_mlp and of mgym_ppo_grad_mlp2 / mgym_value_grad_mlp2 (checks(depth) makes the tests of one
depth: this file runs the one-layer ones under their names, tests/test_grad2_host.py the two-layer ones): the
float64 restatement against torch's float64 autograd of the textbook loss; modurl_gym_amd/csrc/grad.h and grad2.h built for the host
(tests/native/grad_check.cpp, -ffp-contract=off) against the numpy restatement of include/mgym.h's text, word for word; the f32 text against float64, which
gives the bounds the device test uses; and the exact identities of the header-driven full call.

Every case keeps its ratios at least 1e-3 from 1 +- clip and, under ReLU, every hidden pre-activation at least 1e-4 from 0 (test_no_case_sits_on_a_kink), so
f32 and float64 take the same side of every kink and no env-step is ever left out of a comparison.

The bound.  For each output word w, S_w is the float64 mean of |per-env-step term| (grad_ref.grad64); test_the_bound measures the largest
|grad32_w - grad64_w| / S_w over its cases and prints it.  The yardstick is reference code, never the kernel.

One hidden layer: every family and the critics of CartPole and LunarLander, H = 64 and 17, the three activations, two seeds, K = 2, n = 1028 —
    gradient words  3.17e-06 (Pendulum, H = 64, ReLU, seed 1)        statistics  1.57e-07
(the scores carry their chains' rounding, about 1e-6 relative at 64 links, mg_tanhf_fast is 2.5 spacings from tanh, and the terms of a word add with both
signs while S_w adds their magnitudes).  grad_ref.GRAD_BOUND and STAT_BOUND are 4 x those, the margin of test_logprob_host.py.  torch's own f32 CPU autograd of
the same loss, the same measure at H = 64: 1.03e-06 (grad_ref.TORCH32_BOUND = 4 x that: the network-rounding bound of the device's torch comparison).

Two hidden layers: the same families and critics, the five widths of grad_ref.WIDTHS, both activations, K = 1 and 2 at n = 2052, the shapes the device test
runs; the figures are checked against grad_ref.GRAD2_MEASURED / STAT2_MEASURED, and GRAD2_BOUND and STAT2_BOUND are 4 x those.  The gradient figure has a
heavy tail under ReLU: a word of dW2 or dW1 whose few terms hold an h1_j = pre1_j just beyond the kink margin carries the chain's absolute rounding (1e-6)
against 4e-4, so the figure is set by one such word (8e-3; the K = 17 shapes stay below 1.8e-3, the tanh_fast cases below 1e-5) and the cases have to be the
device test's own.  The sharp check of the kernels is the other one, against grad32 under SUM_BOUND.  test_torch_f32_against_float64 does the same for
torch's own f32 CPU autograd (TORCH32_2_MEASURED)."""
import numpy as np
import pytest

import grad_ref as G
import logprob_ref as R
from words import same, same_words

F = np.float32
K, N = 2, 1028
BOUND_KS, BOUND_N = (1, 2), 2052   # two layers: the shapes of tests/test_gpu_grad_mlp.py
HS = {1: ((1,), (17,), (64,)), 2: G.WIDTHS}
CRITICS = ("cartpole", "lunar_lander")
CASES = [(f, G.PPO) for f in R.ALL] + [(f, G.VALUE) for f in CRITICS]
MID = {1: (17,), 2: (17, 9)}      # the widths of the identities and the slices
WIDE = {1: (64,), 2: (64, 64)}


def textbook_loss(torch, c, params, dtype):
    """the loss as a learner writes it: log_softmax + gather or Normal.log_prob, torch.min / clamp, the entropy bonus; MSE for the critic.  params: (w, b) of
    every layer in order, then log sigma"""
    *layers, log_sigma = params
    f = torch.relu if c.act == G.RELU else torch.tanh
    x = torch.from_numpy(np.moveaxis(R.acted_rows(c.obs_first, c.obs), 1, 2).reshape(-1, c.D).copy()).to(dtype)
    for k in range(0, len(layers) - 2, 2):
        x = f(x @ layers[k].T + layers[k + 1])
    s = x @ layers[-2].T + layers[-1]
    x0 = torch.from_numpy(np.asarray(c.x0).reshape(-1).copy()).to(dtype)
    if c.head == G.VALUE:
        return 0.5 * ((s[:, 0] - x0) ** 2).mean()
    adv = torch.from_numpy(np.asarray(c.x1).reshape(-1).copy()).to(dtype)
    if c.gauss:
        dist = torch.distributions.Normal(s[:, 0], log_sigma.exp())
        logp, ent = dist.log_prob(torch.from_numpy(np.asarray(c.actions).reshape(-1).copy()).to(dtype)), dist.entropy()
    else:
        ls = torch.log_softmax(s, -1)
        logp = ls.gather(-1, torch.from_numpy(np.asarray(c.actions, np.int64).reshape(-1, 1)))[:, 0]
        ent = -(ls.exp() * ls).sum(-1)
    r = (logp - x0).exp()
    lo, hi = float(F(1.0) - F(c.clip)), float(F(1.0) + F(c.clip))
    return -torch.min(r * adv, torch.clamp(r, lo, hi) * adv).mean() - float(F(c.ent_coef)) * ent.mean()


def autograd(c, dtype):
    torch = pytest.importorskip("torch")
    params = [torch.tensor(np.asarray(w, np.float64), dtype=dtype, requires_grad=True) for w in G.split(c.pol, c.D, c.A, c.widths)]
    params.append(torch.tensor([np.log(float(F(c.sigma)))], dtype=dtype, requires_grad=True))
    loss = textbook_loss(torch, c, params, dtype)
    loss.backward()
    g = [p.grad if p.grad is not None else torch.zeros_like(p) for p in params]
    return np.concatenate([x.detach().double().numpy().ravel() for x in g]), float(loss.detach())


def off_the_kinks(c, ref, what):
    if c.head == G.PPO:
        lo, hi = float(F(1.0) - F(c.clip)), float(F(1.0) + F(c.clip))
        assert min(np.abs(ref.ratio - lo).min(), np.abs(ref.ratio - hi).min()) >= G.KINK_RATIO, what
    if c.act == G.RELU:
        assert np.abs(ref.pre).min() >= G.KINK_PRE, what


def checks(depth):
    """the tests of the gradient calls with `depth` hidden layers, by name: tests/test_grad_host.py takes depth 1, tests/test_grad2_host.py depth 2"""
    def test_no_case_sits_on_a_kink():
        """on the float64 reference alone: every ratio at least 1e-3 from 1 +- clip, every ReLU pre-activation of every hidden layer at least 1e-4 from 0,
        advantages of both signs"""
        for family, head in CASES:
            for widths in HS[depth]:
                for act in G.ACTS[depth]:
                    for seed in (0, 1) if depth == 1 else (0,):
                        c = G.case(family, K, N, widths, act, head, seed)
                        ref = G.grad64(c)
                        off_the_kinks(c, ref, (family, widths, act))
                        if head == G.PPO:
                            assert (c.x1 > 0).any() and (c.x1 < 0).any() and 0.2 < ref.stats[3] < 0.5

    @pytest.mark.parametrize("family,head", CASES)
    def test_float64_restatement_against_autograd(family, head):
        """grad64 against torch's float64 CPU autograd of the textbook loss (float64 rounding over B <= 4 096 terms).  One layer: 1e-12 absolute on gradients of
        order 1.  Two layers: 1e-12 relative to S_w; torch's tanh for tanh_fast, which is differentiated as the tanh it approximates"""
        torch = pytest.importorskip("torch")
        for widths in HS[1] if depth == 1 else ((64, 64), (17, 9), (1, 1)):
            for act in (G.TANH, G.RELU) if depth == 1 else G.ACTS[2]:
                c = G.case(family, K, N, widths, act, head)
                ref = G.grad64(c)
                got, loss = autograd(c, torch.float64)
                if not c.gauss:
                    got[-1] = 0.0   # (the log-sigma word of the other heads is +0)
                if depth == 1:
                    assert np.abs(got - ref.grad).max() <= 1e-12, (family, head, widths, act, float(np.abs(got - ref.grad).max()))
                else:
                    w, zeros = G.worst(got, ref.grad, ref.S_grad)
                    assert w <= 1e-12 and zeros, (family, head, widths, act, w)
                full = ref.stats[0] - (float(F(c.ent_coef)) * ref.stats[1] if head == G.PPO else 0.0)
                assert abs(loss - full) <= 1e-12
                assert np.abs(ref.grad).max() > (1e-3 if depth == 1 else 1e-4)

    @pytest.mark.parametrize("family,head", CASES)
    def test_header_equals_the_text(family, head):
        """the words of the host-compiled header, word for word the numpy restatement's — one layer: ds, g, r, p_a, Hent and the statistics' terms; two layers:
        the scores, ds, the log-sigma term, the statistics' terms, dpre2_k, dh1_j and dpre1_j — and the header-driven full call is the restatement's float64 sum
        of the same words"""
        for widths in HS[depth]:
            for act in (G.TANH, G.RELU, G.TANH_FAST) if widths == (17,) else (G.TANH, G.RELU) if depth == 1 else G.ACTS[2]:
                c = G.case(family, K, N, widths, act, head)
                text, hdr = G.words32(c), G.header_words(c)
                for k in ("ds", "g", "r", "p", "hent", "stat") if depth == 1 else ("s", "ds", "dls", "stat", "dpre2", "dh1", "dpre1"):
                    assert same_words(hdr[k], text[k]), (family, head, widths, act, k)
                assert np.isfinite(text["ds"]).all()
                g32, hg = G.grad32(c, words=text), G.header_grad(c)
                if depth == 1:
                    assert same(g32[0], hg[0]) and same(g32[1], hg[1]), (family, head, widths, act)
                else:
                    ref = G.grad64(c)
                    # the sums: the header adds env-step by env-step in f64, numpy pairwise: equal to f64 rounding, far inside one f32 spacing of most words
                    assert G.worst(g32[0], hg[0], ref.S_grad)[0] <= 1e-7 and G.worst(g32[1][:5], hg[1][:5], ref.S_stats[:5])[0] <= 1e-7, (family, head, widths, act)
                    assert same(g32[1][5:], hg[1][5:])

    def test_the_bound():
        """the f32 text summed in float64 against float64: measured and printed.  One layer: asserted at 4 x the figures of the module docstring (GRAD_BOUND,
        STAT_BOUND).  Two layers: asserted at the recorded figures themselves (4 x them is GRAD2_BOUND / STAT2_BOUND), which may not be stale either"""
        b = G.BOUNDS[depth]
        wg = ws = 0.0
        where = None
        for family, head in CASES:
            for widths in ((64,), (17,)) if depth == 1 else G.WIDTHS:
                for act in G.ACTS[depth]:
                    for k, n, seed in ((K, N, 0), (K, N, 1)) if depth == 1 else [(k, BOUND_N, 0) for k in BOUND_KS]:
                        c = G.case(family, k, n, widths, act, head, seed)
                        ref = G.grad64(c)
                        if depth == 2:
                            off_the_kinks(c, ref, (family, widths, act, k))
                        grad, stats = G.grad32(c)   # the numpy text, never the header
                        ok, (g, s) = G.within(grad, stats, ref)
                        if g > wg:
                            where = (family, head, widths, act, k, seed)
                        wg, ws = max(wg, g), max(ws, s)
                        assert ok, (family, head, widths, act, k, seed, g, s)
        print(f"largest |grad32 - grad64| / S: gradient words {wg:.3g} at {where} (recorded {b.grad_measured:.3g}, bound {b.grad:.3g}), statistics {ws:.3g} "
              f"(recorded {b.stat_measured:.3g}, bound {b.stat:.3g})")
        if depth == 1:
            assert wg <= G.GRAD_BOUND and ws <= G.STAT_BOUND
        else:
            assert wg <= G.GRAD2_MEASURED * 1.0000001 and ws <= G.STAT2_MEASURED * 1.0000001
            assert wg >= 0.5 * G.GRAD2_MEASURED and ws >= 0.5 * G.STAT2_MEASURED, "the recorded figures are stale"

    def test_torch_f32_against_float64():
        """torch's own f32 CPU autograd of the textbook loss against grad64, the same measure: the network-rounding bound of the device's torch comparison"""
        torch = pytest.importorskip("torch")
        worst = 0.0
        for family, head in CASES:
            for act in (G.TANH, G.RELU) if depth == 1 else G.ACTS[2]:
                c = G.case(family, K, N, WIDE[depth], act, head)
                ref = G.grad64(c)
                got, _ = autograd(c, torch.float32)
                if not c.gauss:
                    got[-1] = 0.0
                worst = max(worst, G.worst(got, ref.grad, ref.S_grad)[0])
        print(f"largest |torch f32 - grad64| / S: {worst:.3g} (recorded {G.BOUNDS[depth].torch32_measured:.3g}, bound {G.BOUNDS[depth].torch32:.3g})")
        assert worst <= G.BOUNDS[depth].torch32

    if depth == 1:
        @pytest.mark.parametrize("family", ("cartpole", "acrobot", "pendulum"))
        def test_exact_identities(family):
            D, A = R.dims(family)
            for act in (G.TANH_FAST, G.RELU):
                c = G.case(family, K, N, (17,), act)
                # logp_old from the log-probability call with the same weights: d = +0, the ratio exactly 1
                old = R.logprob_mlp(c.pol, D, A, (17,), act, c.obs_first, c.obs, c.actions, c.sigma).view(F)
                grad, stats = G.header_grad(G.variant(c, x0=old))
                assert same(stats[2:5], np.array([0.0, 0.0, 1.0], F)) and np.isfinite(grad).all() and np.abs(grad).max() > 0
                # no advantage and no entropy bonus: no gradient
                grad, stats = G.header_grad(G.variant(c, x1=np.zeros_like(c.x1), ent_coef=0.0))
                assert (grad == 0).all() and stats[0] == 0
                # every env-step clipped
                cc = G.case(family, K, N, (17,), act, all_clipped=True)
                grad, stats = G.header_grad(G.variant(cc, ent_coef=0.0))
                assert (grad == 0).all() and stats[3] == F(1.0)
                # ent_coef moves the gradient by the entropy term only: with every env-step clipped g = 0, and what is left is grad64's with g = 0
                grad, stats = G.header_grad(cc)
                ref = G.grad64(cc)
                assert ref.stats[3] == 1.0 and G.within(grad, stats, ref)[0]
                plain = G.header_grad(G.variant(c, ent_coef=0.0))[0].astype(np.float64)
                both, ent_only = G.header_grad(c)[0].astype(np.float64), grad.astype(np.float64)
                ref_c, ref_0 = G.grad64(c), G.grad64(G.variant(c, ent_coef=0.0))
                moved, want = both - plain, ref_c.grad - ref_0.grad   # the entropy term of the unclipped case, in f32 and in float64
                assert np.abs(moved - want).max() <= 2 * G.GRAD_BOUND * np.maximum(ref_c.S_grad, ref_0.S_grad).max()
                assert np.abs(want).max() > 0 and np.isfinite(ent_only).all()

    def test_slices_partition_the_batch():
        """two slices' gradients weighted by their B give the full range's, in float64 exactly enough and in the header-driven call within the bound"""
        for family, head in (("cartpole", G.PPO), ("pendulum", G.PPO), ("lunar_lander", G.VALUE)):
            c = G.case(family, K, N, MID[depth], G.TANH_FAST, head)
            full, a, b = G.grad64(c), G.grad64(c, 4, 512), G.grad64(c, 516, 512)
            whole = G.grad64(c, 4, 1024)
            mix = (a.grad + b.grad) / 2
            assert np.abs(mix - whole.grad).max() <= 1e-12
            if depth == 1:
                assert not np.allclose(whole.grad, full.grad, atol=1e-9)
            ga, gb = G.header_grad(c, 4, 512), G.header_grad(c, 516, 512)
            assert G.within((ga[0].astype(np.float64) + gb[0]) / 2, (ga[1].astype(np.float64) + gb[1]) / 2 * np.array([1, 1, 1, 1, 1, 2, 1, 1]), whole)[0]

    if depth == 1:
        def test_the_arguments_the_calls_accept():
            lib = G.check_lib()
            for clip in (0.0, 0.2, float(np.nextafter(F(1.0), F(0.0)))):
                assert lib.grad_clip_ok_of(clip) == 1, clip
            for clip in (-0.0001, 1.0, 2.0, np.nan, np.inf, -np.inf):
                assert lib.grad_clip_ok_of(clip) == 0, clip
            for x in (0.0, -0.0, 0.01, -3.0, float(np.finfo(F).max)):
                assert lib.grad_ent_coef_ok_of(x) == 1, x
            for x in (np.nan, np.inf, -np.inf):
                assert lib.grad_ent_coef_ok_of(x) == 0, x
            assert lib.grad_slab_bytes_of(8, 4, 64) == 8 * (836 + 8) and lib.grad_slab_bytes_of(4, 2, 1) == 8 * (9 + 8)

    if depth == 2:
        def test_the_slab():
            lib = G.check_lib()
            assert lib.grad2_slab_bytes_of(8, 4, 64, 64) == 8 * (4996 + 8) and lib.grad2_slab_bytes_of(4, 2, 1, 1) == 8 * (5 + 2 + 4 + 8)
            assert lib.grad2_slab_cap() == G.SLAB_CAP

    return {name: f for name, f in locals().items() if name.startswith("test_")}


globals().update(checks(1))
