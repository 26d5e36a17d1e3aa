"""No-GPU check of mgym_value_mlp's mapping: modurl_gym_amd/csrc/value.h over the policy headers (the lines the kernels of value.hip compile) built for the host
by tests/native/value_check.cpp with -ffp-contract=off, against the numpy restatement of include/mgym.h's text in tests/value_ref.py (glibc fmaf) — every
word, no tolerance, the words the text does not write included (they keep the poison); a poisoned final_obs; and the restatement against the float64 network.

The float64 bound.  On the draws of f64_case (value_ref.critic_weights: mlp_ref / mlp2_ref.normal_weights with a value head of scale 10, observations uniform
inside each family's obs_low / obs_high, 4 seeds x 5 families x 2048 observations, |V| up to 69) the restatement's largest |f32 - f64| was measured as
    (64,) relu: 9.85e-06   (64,) tanh: 8.85e-06   (64,) tanh_fast: 8.85e-06   (64, 64) relu: 1.14e-05   (64, 64) tanh_fast: 7.53e-06
    (17,) relu: 9.02e-06   (17,) tanh: 5.16e-06   (17,) tanh_fast: 5.47e-06   (17, 33) relu: 9.50e-06   (17, 33) tanh_fast: 5.59e-06
(a chain of H links each rounding at half a spacing of its partial sum, 1.9e-6 at magnitude 32; mg_tanhf_fast is within 2.5 spacings of tanh, 1.5e-7 at 1, times
a head weight of order 10 / sqrt(H)).  The asserted bound is 4 x the measured maximum of the row's widths and activation, the margin of test_gae_host.py.  The
comparison side is value_ref.value64, numpy's float64 dot products and np.tanh, never the header."""
import numpy as np
import pytest

import families
import value_ref as R
from words import same

F = np.float32
N = 1028   # four whole waves of the final pass and one of 4 environments; a multiple of 4, so the host check also takes the dense rows four to a lane
KS = (1, 2, 17)
FAMILIES = ("mountain_car", "pendulum", "cartpole", "acrobot", "lunar_lander")   # D = 2, 3, 4, 6, 8
F64_MEASURED = {((64,), R.RELU): 9.85e-06, ((64,), R.TANH): 8.85e-06, ((64,), R.TANH_FAST): 8.85e-06, ((64, 64), R.RELU): 1.14e-05, ((64, 64), R.TANH_FAST): 7.53e-06,
                ((17,), R.RELU): 9.02e-06, ((17,), R.TANH): 5.16e-06, ((17,), R.TANH_FAST): 5.47e-06, ((17, 33), R.RELU): 9.50e-06, ((17, 33), R.TANH_FAST): 5.59e-06}
F64_BOUND = {k: 4 * v for k, v in F64_MEASURED.items()}


def triple_same(got, exp):
    return same(got[0], exp[0]) and same(got[1], exp[1]) and ((got[2] is None and exp[2] is None) or same(got[2], exp[2]))


def test_the_families_cover_every_width():
    assert [families.FAMILIES[f].D for f in FAMILIES] == [2, 3, 4, 6, 8]
    assert R.chunk() == 16 and R.wave_envs() == 256


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("K", KS)
def test_header_equals_the_restatement(family, K):
    """every accepted (depth, activation) at small widths; the final triple with done, with done NULL, and absent"""
    c = R.case(family, K, N)
    for widths in ((17,), (3, 5)):
        crit, _ = R.critic(family, widths)
        for act in R.ACTS[len(widths)]:
            for fo, d, u in ((c["final_obs_d"], c["d"], c["u"]), (c["final_obs_nd"], None, c["u"]), (None, None, None), (None, c["d"], c["u"])):
                exp = R.value_mlp(crit, c["D"], widths, act, c["obs_first"], c["obs"], fo, d, u)
                got = R.header_value_mlp(crit, c["D"], widths, act, c["obs_first"], c["obs"], fo, d, u)
                assert triple_same(got, exp), (family, K, widths, act, d is None, fo is None)
                assert np.isfinite(exp[0]).all() and np.isfinite(exp[1]).all()
                if fo is not None:
                    sel = R.selection(d, u)
                    assert (exp[2][~sel] == R.POISON).all() and np.isfinite(exp[2][sel].view(F)).all() and sel.sum() >= 130 + K


@pytest.mark.parametrize("widths", R.WIDTHS, ids=str)
def test_every_width_class(widths):
    """H = 1, a partial chunk of 8, 64; (1, 1), (3, 5), (17, 33), (64, 64) — on CartPole's D = 4 and LunarLander's D = 8 at K = 2"""
    for family in ("cartpole", "lunar_lander"):
        c = R.case(family, 2, N)
        crit, _ = R.critic(family, widths)
        for act in R.ACTS[len(widths)]:
            args = (crit, c["D"], widths, act, c["obs_first"], c["obs"], c["final_obs_d"], c["d"], c["u"])
            assert triple_same(R.header_value_mlp(*args), R.value_mlp(*args)), (family, widths, act)


def test_a_population_that_is_no_multiple_of_four():
    """n = 1030: the last wave of the final pass holds 6 environments, every one of them selected on every step"""
    c = R.case("mountain_car", 17, 1030)
    for widths, act in (((17,), R.RELU), ((3, 5), R.TANH_FAST)):
        crit, _ = R.critic("mountain_car", widths)
        for fo, d in ((c["final_obs_d"], c["d"]), (c["final_obs_nd"], None)):
            args = (crit, 2, widths, act, c["obs_first"], c["obs"], fo, d, c["u"])
            assert triple_same(R.header_value_mlp(*args), R.value_mlp(*args)), (widths, act, d is None)


@pytest.mark.parametrize("K", KS)
def test_poisoned_final_obs_equals_the_clean_run(K):
    """every word of final_obs outside the selected set is NaN: all results are finite and equal to the run on the clean buffer"""
    c = R.case("pendulum", K, N)
    for widths, act in (((17,), R.TANH), ((17, 33), R.TANH_FAST)):
        crit, _ = R.critic("pendulum", widths)
        for d, poisoned in ((c["d"], c["final_obs_d"]), (None, c["final_obs_nd"])):
            sel = R.selection(d, c["u"])
            assert np.isnan(poisoned[~np.broadcast_to(sel[:, None, :], poisoned.shape)]).all() and not np.isnan(poisoned[:, 0, :][sel]).any()
            for impl in (R.value_mlp, R.header_value_mlp):
                clean = impl(crit, 3, widths, act, c["obs_first"], c["obs"], c["final_obs"], d, c["u"])
                got = impl(crit, 3, widths, act, c["obs_first"], c["obs"], poisoned, d, c["u"])
                assert triple_same(got, clean) and np.isfinite(got[2][sel].view(F)).all() and (got[2][~sel] == R.POISON).all()


@pytest.mark.parametrize("act", (R.RELU, R.TANH_FAST))
def test_a_signed_zero_reaches_the_value(act):
    """mlp2_ref.signed_zero_policy: V = -0 at every observation, +0 under a chain padded with zero weights"""
    import mlp2_ref
    c = R.case("pendulum", 2, N)
    crit = R.packed(mlp2_ref.signed_zero_policy(3, act))
    for impl in (R.value_mlp, R.header_value_mlp):
        v, last, _ = impl(crit, 3, (3, 5), act, c["obs_first"], c["obs"])
        assert (v.view(np.uint32) == 0x80000000).all() and (last.view(np.uint32) == 0x80000000).all()


def f64_case(family, widths, seed):
    rng = np.random.default_rng(50 + seed)
    w = R.critic_weights(rng, family, widths)
    return R.packed(w), R.observations(rng, family, (), 2048)


@pytest.mark.parametrize("key", sorted(F64_MEASURED, key=str), ids=lambda k: f"{k[0]}-{R.ACT_NAMES[k[1]]}")
def test_against_float64(key):
    widths, act = key
    worst, top = 0.0, 0.0
    for family in FAMILIES:
        D = families.FAMILIES[family].D
        for seed in range(4):
            crit, obs = f64_case(family, widths, seed)
            v64 = R.value64(crit, D, widths, act, obs)
            v32 = R.values(crit, D, widths, act, obs)
            worst, top = max(worst, float(np.abs(v32 - v64).max())), max(top, float(np.abs(v64).max()))
    print(f"{widths} {R.ACT_NAMES[act]}: largest |f32 - f64| = {worst:.3g} at |V| <= {top:.3g}, bound {F64_BOUND[key]:.3g}")
    assert worst <= F64_BOUND[key]
