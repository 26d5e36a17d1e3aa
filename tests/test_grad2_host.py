"""No-GPU checks of the words of mgym_ppo_grad_mlp2 and mgym_value_grad_mlp2: the float64 restatement against torch's float64 autograd of the textbook loss;
modurl_gym_amd/csrc/grad2.h built for the host (tests/native/grad2_check.cpp, -ffp-contract=off) against the numpy restatement of include/mgym.h's text, word
for word; the f32 text against float64, which gives the bounds the device test uses.

Every case keeps its ratios at least 1e-3 from 1 +- clip and, under ReLU, every |pre1_j| and |pre2_k| at least 1e-4 from 0 (test_no_case_sits_on_a_kink).

The bound.  For each output word w, S_w is the float64 mean of |per-env-step term| (grad2_ref.grad64).  test_the_bound measures the largest
|grad32_w - grad64_w| / S_w over its cases — every family and the critics of CartPole and LunarLander, the five widths of grad2_ref.WIDTHS, both activations,
K = 1 and 2 at n = 2052, the shapes the device test runs — prints it and checks it against grad2_ref.GRAD2_MEASURED / STAT2_MEASURED; GRAD2_BOUND and
STAT2_BOUND are 4 x those.  The gradient figure has a heavy tail under ReLU: a word of dW2 or dW1 whose few terms hold an h1_j = pre1_j just beyond the kink
margin carries the chain's absolute rounding (1e-6) against 4e-4, so the figure is set by one such word (8e-3; the K = 17 shapes stay below 1.8e-3, the tanh_fast
cases below 1e-5) and the cases have to be the device test's own.  The sharp check of the kernels is the other one, against grad32 under SUM_BOUND.  The yardstick
is reference code, never the kernel.  test_torch_f32_against_float64 does the same for torch's own f32 CPU autograd (TORCH32_2_MEASURED)."""
import numpy as np
import pytest

import grad2_ref as G2
import logprob_ref as R
import mlp2_ref
from words import same, same_words

F = np.float32
K, N = 2, 1028
BOUND_KS, BOUND_N = (1, 2), 2052   # the shapes of tests/test_gpu_grad2_mlp.py
CRITICS = ("cartpole", "lunar_lander")
CASES = [(f, G2.PPO) for f in R.ALL] + [(f, G2.VALUE) for f in CRITICS]


def textbook_loss(torch, c, params, dtype):
    """the loss as a learner writes it: log_softmax + gather or Normal.log_prob, torch.min / clamp, the entropy bonus; MSE for the critic"""
    w1, b1, w2, b2, w3, b3, log_sigma = params
    f = torch.relu if c.act == G2.RELU else torch.tanh
    x = torch.from_numpy(np.moveaxis(R.acted_rows(c.obs_first, c.obs), 1, 2).reshape(-1, c.D).copy()).to(dtype)
    s = f(f(x @ w1.T + b1) @ w2.T + b2) @ w3.T + b3
    x0 = torch.from_numpy(np.asarray(c.x0).reshape(-1).copy()).to(dtype)
    if c.head == G2.VALUE:
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
    params = [torch.tensor(np.asarray(w, np.float64), dtype=dtype, requires_grad=True) for w in mlp2_ref.split(c.pol, c.D, c.A, c.H1, c.H2)]
    params.append(torch.tensor([np.log(float(F(c.sigma)))], dtype=dtype, requires_grad=True))
    loss = textbook_loss(torch, c, params, dtype)
    loss.backward()
    g = [p.grad if p.grad is not None else torch.zeros_like(p) for p in params]
    return np.concatenate([x.detach().double().numpy().ravel() for x in g]), float(loss.detach())


def test_no_case_sits_on_a_kink():
    """on the float64 reference alone: every ratio at least 1e-3 from 1 +- clip, every ReLU pre-activation of both layers at least 1e-4 from 0, advantages of
    both signs"""
    for family, head in CASES:
        for H1, H2 in G2.WIDTHS:
            for act in G2.ACTS:
                c = G2.case2(family, K, N, H1, H2, act, head)
                ref = G2.grad64(c)
                if head == G2.PPO:
                    lo, hi = float(F(1.0) - F(c.clip)), float(F(1.0) + F(c.clip))
                    assert min(np.abs(ref.ratio - lo).min(), np.abs(ref.ratio - hi).min()) >= G2.KINK_RATIO, (family, H1, H2, act)
                    assert (c.x1 > 0).any() and (c.x1 < 0).any() and 0.2 < ref.stats[3] < 0.5
                if act == G2.RELU:
                    assert np.abs(ref.pre).min() >= G2.KINK_PRE, (family, H1, H2, act)


@pytest.mark.parametrize("family,head", CASES)
def test_float64_restatement_against_autograd(family, head):
    """grad64 against torch's float64 CPU autograd of the textbook loss: 1e-12 relative to S_w (float64 rounding over B <= 4 096 terms); torch's tanh for
    tanh_fast, which is differentiated as the tanh it approximates"""
    torch = pytest.importorskip("torch")
    for H1, H2 in ((64, 64), (17, 9), (1, 1)):
        for act in G2.ACTS:
            c = G2.case2(family, K, N, H1, H2, act, head)
            ref = G2.grad64(c)
            got, loss = autograd(c, torch.float64)
            if not c.gauss:
                got[-1] = 0.0   # (the log-sigma word of the other heads is +0)
            w, zeros = G2.worst(got, ref.grad, ref.S_grad)
            assert w <= 1e-12 and zeros, (family, head, H1, H2, act, w)
            full = ref.stats[0] - (float(F(c.ent_coef)) * ref.stats[1] if head == G2.PPO else 0.0)
            assert abs(loss - full) <= 1e-12
            assert np.abs(ref.grad).max() > 1e-4


@pytest.mark.parametrize("family,head", CASES)
def test_header_equals_the_text(family, head):
    """ds, the log-sigma term, the statistics' terms, dpre2_k, dh1_j and dpre1_j of the host-compiled header, word for word the numpy restatement's; and the
    header-driven full call is the restatement's float64 sum of the same words, to the word"""
    for H1, H2 in G2.WIDTHS:
        for act in G2.ACTS:
            c = G2.case2(family, K, N, H1, H2, act, head)
            text, hdr = G2.words32(c), G2.header_words(c)
            for k in ("s", "ds", "dls", "stat", "dpre2", "dh1", "dpre1"):
                assert same_words(hdr[k], text[k]), (family, head, H1, H2, act, k)
            assert np.isfinite(text["ds"]).all()
            g32, hg = G2.grad32(c, words=text), G2.header_grad(c)
            ref = G2.grad64(c)
            # the sums: the header adds env-step by env-step in f64, numpy pairwise: equal to f64 rounding, far inside one f32 spacing of most words
            assert G2.worst(g32[0], hg[0], ref.S_grad)[0] <= 1e-7 and G2.worst(g32[1][:5], hg[1][:5], ref.S_stats[:5])[0] <= 1e-7, (family, head, H1, H2, act)
            assert same(g32[1][5:], hg[1][5:])


def test_the_bound():
    """the f32 text summed in float64 against float64: measured, printed, and asserted at the recorded figures (4 x them is GRAD2_BOUND / STAT2_BOUND)"""
    wg = ws = 0.0
    where = None
    for family, head in CASES:
        for H1, H2 in G2.WIDTHS:
            for act in G2.ACTS:
                for k in BOUND_KS:
                    c = G2.case2(family, k, BOUND_N, H1, H2, act, head)
                    ref = G2.grad64(c)
                    if act == G2.RELU:
                        assert np.abs(ref.pre).min() >= G2.KINK_PRE
                    if head == G2.PPO:
                        lo, hi = float(F(1.0) - F(c.clip)), float(F(1.0) + F(c.clip))
                        assert min(np.abs(ref.ratio - lo).min(), np.abs(ref.ratio - hi).min()) >= G2.KINK_RATIO
                    grad, stats = G2.grad32(c)   # the numpy text, never the header
                    ok, (g, s) = G2.within(grad, stats, ref)
                    if g > wg:
                        where = (family, head, H1, H2, act, k)
                    wg, ws = max(wg, g), max(ws, s)
                    assert ok, (family, head, H1, H2, act, k, g, s)
    print(f"largest |grad32 - grad64| / S: gradient words {wg:.3g} at {where} (recorded {G2.GRAD2_MEASURED:.3g}), statistics {ws:.3g} (recorded {G2.STAT2_MEASURED:.3g})")
    assert wg <= G2.GRAD2_MEASURED * 1.0000001 and ws <= G2.STAT2_MEASURED * 1.0000001
    assert wg >= 0.5 * G2.GRAD2_MEASURED and ws >= 0.5 * G2.STAT2_MEASURED, "the recorded figures are stale"


def test_torch_f32_against_float64():
    """torch's own f32 CPU autograd of the textbook loss against grad64, the same measure: the network-rounding bound of the device's torch comparison"""
    torch = pytest.importorskip("torch")
    worst = 0.0
    for family, head in CASES:
        for act in G2.ACTS:
            c = G2.case2(family, K, N, 64, 64, act, head)
            ref = G2.grad64(c)
            got, _ = autograd(c, torch.float32)
            if not c.gauss:
                got[-1] = 0.0
            worst = max(worst, G2.worst(got, ref.grad, ref.S_grad)[0])
    print(f"largest |torch f32 - grad64| / S: {worst:.3g} (recorded {G2.TORCH32_2_MEASURED:.3g})")
    assert worst <= G2.TORCH32_2_BOUND


def test_slices_partition_the_batch():
    """two slices' gradients weighted by their B give the full range's, in float64 and in the header-driven call within the bound"""
    for family, head in (("cartpole", G2.PPO), ("pendulum", G2.PPO), ("lunar_lander", G2.VALUE)):
        c = G2.case2(family, K, N, 17, 9, G2.TANH_FAST, head)
        a, b, whole = G2.grad64(c, 4, 512), G2.grad64(c, 516, 512), G2.grad64(c, 4, 1024)
        assert np.abs((a.grad + b.grad) / 2 - whole.grad).max() <= 1e-12
        ga, gb = G2.header_grad(c, 4, 512), G2.header_grad(c, 516, 512)
        assert G2.within((ga[0].astype(np.float64) + gb[0]) / 2, (ga[1].astype(np.float64) + gb[1]) / 2 * np.array([1, 1, 1, 1, 1, 2, 1, 1]), whole)[0]


def test_the_slab():
    lib = G2.check_lib()
    assert lib.grad2_slab_bytes_of(8, 4, 64, 64) == 8 * (4996 + 8) and lib.grad2_slab_bytes_of(4, 2, 1, 1) == 8 * (5 + 2 + 4 + 8)
    assert lib.grad2_slab_cap() == G2.SLAB_CAP
