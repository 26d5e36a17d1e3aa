"""No-GPU checks of the words of mgym_ppo_grad_mlp and mgym_value_grad_mlp: the float64 restatement against torch's float64 autograd of the textbook loss;
modurl_gym_amd/csrc/grad.h built for the host (tests/native/grad_check.cpp, -ffp-contract=off) against the numpy restatement of include/mgym.h's text, word
for word; the f32 text against float64, which gives the bounds the device test uses; and the exact identities of the header-driven full call.

Every case keeps its ratios at least 1e-3 from 1 +- clip and, under ReLU, every |pre_j| at least 1e-4 from 0 (test_no_case_sits_on_a_kink), so f32 and float64
take the same side of every kink and no env-step is ever left out of a comparison.

The bound.  For each output word w, S_w is the float64 mean of |per-env-step term| (grad_ref.grad64).  Measured over the cases of test_the_bound — every
family and the critics of CartPole and LunarLander, H = 64 and 17, the three activations, two seeds, K = 2, n = 1028 — the largest |grad32_w - grad64_w| / S_w is
    gradient words  3.17e-06 (Pendulum, H = 64, ReLU, seed 1)        statistics  1.57e-07
(the scores carry their chains' rounding, about 1e-6 relative at 64 links, mg_tanhf_fast is 2.5 spacings from tanh, and the terms of a word add with both
signs while S_w adds their magnitudes).  grad_ref.GRAD_BOUND and STAT_BOUND are 4 x those, the margin of test_logprob_host.py.  The yardstick is reference
code, never the kernel.  torch's own f32 CPU autograd of the same loss, the same measure at H = 64: 1.03e-06 (grad_ref.TORCH32_BOUND = 4 x that: the
network-rounding bound of the device's torch comparison)."""
import numpy as np
import pytest

import grad_ref as G
import logprob_ref as R
from words import same, same_words

F = np.float32
K, N = 2, 1028
HS = (1, 17, 64)
CRITICS = ("cartpole", "lunar_lander")
CASES = [(f, G.PPO) for f in R.ALL] + [(f, G.VALUE) for f in CRITICS]


def textbook_loss(torch, c, params, dtype):
    """the loss as a learner writes it: log_softmax + gather or Normal.log_prob, torch.min / clamp, the entropy bonus; MSE for the critic"""
    w1, b1, w2, b2, log_sigma = params
    x = torch.from_numpy(np.moveaxis(R.acted_rows(c.obs_first, c.obs), 1, 2).reshape(-1, c.D).copy()).to(dtype)
    h = x @ w1.T + b1
    h = torch.relu(h) if c.act == G.RELU else torch.tanh(h)
    s = h @ w2.T + b2
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
    import mlp_ref
    params = [torch.tensor(np.asarray(w, np.float64), dtype=dtype, requires_grad=True) for w in mlp_ref.split(c.pol, c.D, c.A, c.H)]
    params.append(torch.tensor([np.log(float(F(c.sigma)))], dtype=dtype, requires_grad=True))
    loss = textbook_loss(torch, c, params, dtype)
    loss.backward()
    g = [p.grad if p.grad is not None else torch.zeros_like(p) for p in params]
    return np.concatenate([x.detach().double().numpy().ravel() for x in g]), float(loss.detach())


def test_no_case_sits_on_a_kink():
    """on the float64 reference alone: every ratio at least 1e-3 from 1 +- clip, every ReLU pre-activation at least 1e-4 from 0, advantages of both signs"""
    for family, head in CASES:
        for H in HS:
            for act in G.ACTS:
                for seed in (0, 1):
                    c = G.case(family, K, N, H, act, head, seed)
                    ref = G.grad64(c)
                    if head == G.PPO:
                        lo, hi = float(F(1.0) - F(c.clip)), float(F(1.0) + F(c.clip))
                        assert min(np.abs(ref.ratio - lo).min(), np.abs(ref.ratio - hi).min()) >= G.KINK_RATIO, (family, H, act)
                        assert (c.x1 > 0).any() and (c.x1 < 0).any() and 0.2 < ref.stats[3] < 0.5
                    if act == G.RELU:
                        assert np.abs(ref.pre).min() >= G.KINK_PRE, (family, H, act)


@pytest.mark.parametrize("family,head", CASES)
def test_float64_restatement_against_autograd(family, head):
    """grad64 against torch's float64 CPU autograd: 1e-12 absolute on gradients of order 1 (float64 rounding over B <= 4 096 terms)"""
    for H in HS:
        for act in (G.TANH, G.RELU):
            c = G.case(family, K, N, H, act, head)
            ref = G.grad64(c)
            got, loss = autograd(c, pytest.importorskip("torch").float64)
            if not c.gauss:
                got[-1] = 0.0   # (the log-sigma word of the other heads is +0)
            assert np.abs(got - ref.grad).max() <= 1e-12, (family, head, H, act, float(np.abs(got - ref.grad).max()))
            full = ref.stats[0] - (float(F(c.ent_coef)) * ref.stats[1] if head == G.PPO else 0.0)
            assert abs(loss - full) <= 1e-12
            assert np.abs(ref.grad).max() > 1e-3


@pytest.mark.parametrize("family,head", CASES)
def test_header_equals_the_text(family, head):
    """ds, g, r, p_a, Hent and the statistics' terms of the host-compiled header, word for word the numpy restatement's; and the header-driven full call is the
    restatement's float64 sum of the same words"""
    for H in HS:
        for act in (G.TANH, G.RELU, G.TANH_FAST) if H == 17 else (G.TANH, G.RELU):
            c = G.case(family, K, N, H, act, head)
            text, hdr = G.words32(c), G.header_words(c)
            for k in ("ds", "g", "r", "p", "hent", "stat"):
                assert same_words(hdr[k], text[k]), (family, head, H, act, k)
            assert np.isfinite(text["ds"]).all()
            g32, hg = G.grad32(c, words=text), G.header_grad(c)
            assert same(g32[0], hg[0]) and same(g32[1], hg[1]), (family, head, H, act)


def test_the_bound():
    """the f32 text summed in float64 against float64: the measured figures of the module docstring, asserted at 4 x (grad_ref.GRAD_BOUND, STAT_BOUND)"""
    wg = ws = 0.0
    for family, head in CASES:
        for H in (64, 17):
            for act in G.ACTS:
                for seed in (0, 1):
                    c = G.case(family, K, N, H, act, head, seed)
                    ref = G.grad64(c)
                    grad, stats = G.grad32(c)   # the numpy text, never the header
                    ok, (g, s) = G.within(grad, stats, ref)
                    wg, ws = max(wg, g), max(ws, s)
                    assert ok, (family, head, H, act, seed, g, s)
    print(f"largest |grad32 - grad64| / S: gradient words {wg:.3g} (bound {G.GRAD_BOUND:.3g}), statistics {ws:.3g} (bound {G.STAT_BOUND:.3g})")
    assert wg <= G.GRAD_BOUND and ws <= G.STAT_BOUND


def test_torch_f32_against_float64():
    """torch's own f32 CPU autograd of the textbook loss against grad64, the same measure: the network-rounding bound of the device's torch comparison"""
    torch = pytest.importorskip("torch")
    worst = 0.0
    for family, head in CASES:
        for act in (G.TANH, G.RELU):
            c = G.case(family, K, N, 64, act, head)
            ref = G.grad64(c)
            got, _ = autograd(c, torch.float32)
            if not c.gauss:
                got[-1] = 0.0
            worst = max(worst, G.worst(got, ref.grad, ref.S_grad)[0])
    print(f"largest |torch f32 - grad64| / S: {worst:.3g} (bound {G.TORCH32_BOUND:.3g})")
    assert worst <= G.TORCH32_BOUND


@pytest.mark.parametrize("family", ("cartpole", "acrobot", "pendulum"))
def test_exact_identities(family):
    D, A = R.dims(family)
    for act in (G.TANH_FAST, G.RELU):
        c = G.case(family, K, N, 17, act)
        # logp_old from the log-probability call with the same weights: d = +0, the ratio exactly 1
        old = R.logprob_mlp(c.pol, D, A, (17,), act, c.obs_first, c.obs, c.actions, c.sigma).view(F)
        grad, stats = G.header_grad(G.variant(c, x0=old))
        assert same(stats[2:5], np.array([0.0, 0.0, 1.0], F)) and np.isfinite(grad).all() and np.abs(grad).max() > 0
        # no advantage and no entropy bonus: no gradient
        grad, stats = G.header_grad(G.variant(c, x1=np.zeros_like(c.x1), ent_coef=0.0))
        assert (grad == 0).all() and stats[0] == 0
        # every env-step clipped
        cc = G.case(family, K, N, 17, act, all_clipped=True)
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
        c = G.case(family, K, N, 17, G.TANH_FAST, head)
        full, a, b = G.grad64(c), G.grad64(c, 4, 512), G.grad64(c, 516, 512)
        whole = G.grad64(c, 4, 1024)
        mix = (a.grad + b.grad) / 2
        assert np.abs(mix - whole.grad).max() <= 1e-12 and not np.allclose(whole.grad, full.grad, atol=1e-9)
        ga, gb = G.header_grad(c, 4, 512), G.header_grad(c, 516, 512)
        assert G.within((ga[0].astype(np.float64) + gb[0]) / 2, (ga[1].astype(np.float64) + gb[1]) / 2 * np.array([1, 1, 1, 1, 1, 2, 1, 1]), whole)[0]


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
