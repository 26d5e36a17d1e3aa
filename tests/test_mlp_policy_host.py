"""No-GPU check of the MLP policy header: modurl_gym_amd/csrc/mlp_policy.h (the lines the CartPole / MountainCar rollout kernels and LunarLander's
policy kernel compile) built for the host by tests/native/policy_check.cpp with -ffp-contract=off, against the Python restatement of
include/mgym.h's mgym_rollout_mlp text in tests/mlp_ref.py (glibc fmaf / tanhf) — the action word and every score, bit for bit."""
import itertools
import subprocess

import numpy as np
import pytest

import mlp_ref as M
from mlp_policy_ref import RELU, TANH, mlp_refs, n_floats, split
from policy_header import GREEDY, check_program, header_actions

FAMILIES = {fam: M.FAMILIES[fam] for fam in ("cartpole", "mountain_car", "mountain_car_continuous", "lunar_lander")}   # the four families of this file's cases (policy_check.cpp knows all six)
HIDDEN = (1, 2, 7, 32, 64)
CASE_KINDS = (("ordinary", 40), ("ties", 15), ("zeros", 15), ("huge", 15), ("inf", 15))


@pytest.fixture(scope="module")
def check_exe():
    return check_program()


def hexs(a):
    return " ".join(f"{v:x}" for v in np.asarray(a, np.float32).view(np.uint32))


def make_case(rng, kind, D, A, H):
    nf = n_floats(D, A, H)
    if kind == "ordinary":
        return rng.normal(0, 1.5, nf).astype(np.float32), rng.normal(0, 1.5, D).astype(np.float32)
    if kind == "ties":   # equal rows of W2 with equal biases: exactly equal scores
        pol = rng.normal(0, 1, nf).astype(np.float32)
        w1, b1, w2, b2 = split(pol, D, A, H)
        if A > 1:
            i, j = rng.choice(A, 2, replace=False)
            w2[j], b2[j] = w2[i], b2[i]
            if rng.random() < 0.3:
                w2[:], b2[:] = 0.0, np.float32(rng.integers(-2, 3))
        return pol, rng.normal(0, 1, D).astype(np.float32)
    if kind == "zeros":  # +-0 in weights, biases and observations: -0 pre-activations (ReLU gives +0), -0 == +0 is a tie
        pol = rng.choice(np.array([0.0, -0.0, 1.0, -1.0], np.float32), nf)
        w1, b1, w2, b2 = split(pol, D, A, H)
        if rng.random() < 0.5:
            j = int(rng.integers(0, H))
            w1[j], b1[j] = np.float32(-0.0), np.float32(-0.0)   # every product -0 under a non-negative observation, bias -0: pre_j = -0
        o = rng.choice(np.array([0.0, 1.0, 2.0], np.float32), D) if rng.random() < 0.5 else rng.choice(np.array([0.0, -0.0, 1.0], np.float32), D)
        return pol, o
    if kind == "huge":   # products and sums overflow to +-inf, inf - inf gives NaN scores
        with np.errstate(over="ignore"):
            pol = (rng.normal(0, 1, nf) * 10.0 ** rng.integers(15, 39, nf)).astype(np.float32)
        return pol, (rng.normal(0, 1, D) * 10.0 ** rng.integers(0, 10, D)).astype(np.float32)
    pol = rng.normal(0, 1, nf).astype(np.float32)   # infinite weights: inf * 0 and inf - inf
    pol[rng.choice(nf, int(rng.integers(1, 4)), replace=False)] = rng.choice(np.array([np.inf, -np.inf], np.float32))
    o = rng.normal(0, 1, D).astype(np.float32)
    o[rng.random(D) < 0.3] = 0.0
    return pol, o


def cases():
    rng = np.random.default_rng(20)
    out = []
    for fam, (D, A, cont) in FAMILIES.items():
        for act in (RELU, TANH):
            for H in HIDDEN:
                for kind, count in CASE_KINDS:
                    for _ in range(count):
                        pol, o = make_case(rng, kind, D, A, H)
                        out.append((kind, D, A, cont, act, H, pol, o))
    return out


def same_word(got, exp):
    """equal bit patterns; two NaNs are equal whatever their sign and payload"""
    g, e = np.uint32(got).view(np.float32), np.uint32(exp).view(np.float32)
    return got == exp or (np.isnan(g) and np.isnan(e))


def test_header_matches_the_restatement_of_the_documented_policy(check_exe):
    cs = cases()
    assert len(cs) == 4 * 2 * len(HIDDEN) * 100
    text = "\n".join(f"{D} {A} {cont} {act} {H} {hexs(pol)} {hexs(o)}" for _, D, A, cont, act, H, pol, o in cs) + "\n"
    out = subprocess.run([check_exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(cs)
    seen = {"tie": 0, "nan_first": 0, "nan_later": 0, "relu_pos": 0, "relu_nonpos": 0, "neg_zero_pre": 0, "nan_pre": 0, "inf_score": 0}
    actions = {fam: set() for fam in FAMILIES}
    refs = []   # the restatement, the cases of one shape at once
    for shape, group in itertools.groupby(cs, key=lambda c: c[1:6]):
        group = list(group)
        a, s, pres = mlp_refs(*shape, [c[6] for c in group], [c[7] for c in group])
        refs += [(int(a[i]), [float(v) for v in s[i]], [float(v) for v in pres[i]]) for i in range(len(group))]
    for line, (kind, D, A, cont, act, H, pol, o), (action, s, pres) in zip(out, cs, refs):
        got = [int(v, 16) for v in line.split()]
        exp = [action] + [int(np.float32(v).view(np.uint32)) for v in s]
        assert len(got) == len(exp)
        assert (same_word(got[0], exp[0]) if cont else got[0] == exp[0]) and all(same_word(g, e) for g, e in zip(got[1:], exp[1:])), \
            f"{kind} D={D} A={A} act={act} H={H}: header {line}, restatement {' '.join(f'{v:x}' for v in exp)}"
        fam = [f for f, v in FAMILIES.items() if v == (D, A, cont)][0]
        if not cont:
            actions[fam].add(action)
            fin = [v for v in s if not np.isnan(v)]
            seen["tie"] += len(fin) > 1 and fin.count(max(fin)) > 1
            seen["nan_first"] += bool(np.isnan(s[0]))
            seen["nan_later"] += bool(not np.isnan(s[0]) and any(np.isnan(v) for v in s[1:]))
            if np.isnan(s[0]):
                assert got[0] == 0   # nothing compares greater than a NaN s_0
        seen["inf_score"] += any(np.isinf(v) for v in s)
        if act == RELU:
            seen["relu_pos"] += sum(1 for p in pres if p > 0.0)
            seen["relu_nonpos"] += sum(1 for p in pres if p <= 0.0)
            seen["neg_zero_pre"] += sum(1 for p in pres if p == 0.0 and np.signbit(p))
            seen["nan_pre"] += sum(1 for p in pres if np.isnan(p))
    # the adversarial kinds really happen
    assert all(v > 20 for v in seen.values()), seen
    assert actions["cartpole"] == {0, 1} and actions["mountain_car"] == {0, 1, 2} and actions["lunar_lander"] == {0, 1, 2, 3}


def test_relu_of_negative_zero_and_nan_is_positive_zero(check_exe):
    """h_j = pre_j > 0 ? pre_j : +0: with W2 = 1 and b2 = -0 the score is fmaf(1, h, -0), which is -0 only if h were -0"""
    for b1, w1 in ((-0.0, -0.0), (np.nan, 0.0)):
        pol = np.array([w1, w1, b1, 1.0, -0.0], np.float32)   # MountainCarContinuous, H = 1: W1[1][2], b1, W2[1][1], b2
        line = f"2 1 1 {RELU} 1 {hexs(pol)} {hexs(np.array([1.0, 2.0], np.float32))}\n"
        out = subprocess.run([check_exe], input=line, capture_output=True, text=True, check=True).stdout.split()
        assert out == ["0", "0"], (b1, out)   # +0 (bits 0), not -0 (80000000) and not a NaN


def test_shared_object_form_equals_the_program(check_exe):
    """the bulk form test_gpu_mlp_policy.py uses is the same header: same actions as the program on one batch per family"""
    rng = np.random.default_rng(21)
    for D, A, cont in FAMILIES.values():
        H, n = 7, 33
        pol = rng.normal(0, 1, n_floats(D, A, H)).astype(np.float32)
        obs = rng.normal(0, 1, (D, n)).astype(np.float32)
        for act in (RELU, TANH):
            bulk = header_actions(D, A, 1, act, GREEDY, (H,), pol, obs)[0]
            text = "\n".join(f"{D} {A} {cont} {act} {H} {hexs(pol)} {hexs(obs[:, i])}" for i in range(n)) + "\n"
            out = subprocess.run([check_exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
            assert [int(l.split()[0], 16) for l in out] == [int(v) for v in bulk]
