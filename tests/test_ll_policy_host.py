"""No-GPU check of the LunarLander policy header: modurl_gym_amd/csrc/ll_policy.h (what the persistent rollout launch and the K-step
form's policy kernel evaluate) compiled for the host by tests/native/ll_policy_check.cpp, against numpy / oracle.philox restatements of the
documented policies (include/mgym.h mgym_rollout_linear / mgym_rollout_uniform, LunarLander)."""
import subprocess

import numpy as np
import pytest

import native_build
from oracle import oracle as ora


@pytest.fixture(scope="module")
def check_exe():
    return native_build.program("ll_policy_check.cpp")


def run(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    return np.array([int(v) for v in out.split()], np.uint32)


def lin_ref(w, o):
    """f32, each product and sum rounded on its own, in the documented order; strict sequential argmax"""
    w = np.asarray(w, np.float32).reshape(4, 9)
    o = np.asarray(o, np.float32)
    best, a = None, 0
    with np.errstate(all="ignore"):
        for j in range(4):
            s = np.float32(w[j, 0] * o[0])
            for q in range(1, 8):
                s = np.float32(s + np.float32(w[j, q] * o[q]))
            s = np.float32(s + w[j, 8])
            if j == 0:
                best = s
            elif s > best:
                best, a = s, j
    return a


def hexs(a):
    return " ".join(f"{v:x}" for v in np.asarray(a, np.float32).view(np.uint32))


def cases():
    rng = np.random.default_rng(7)
    out = []
    for _ in range(3000):   # ordinary weights and observations
        out.append((rng.normal(0, 2, 36).astype(np.float32), rng.normal(0, 1.5, 8).astype(np.float32)))
    for _ in range(500):    # exact ties between rows (repeated rows, zero weights with equal biases)
        w = rng.normal(0, 1, 36).astype(np.float32).reshape(4, 9)
        i, j = rng.choice(4, 2, replace=False)
        w[j] = w[i]
        if rng.random() < 0.5:
            w[:, :8] = 0
            w[:, 8] = np.float32(rng.integers(-2, 3))
        out.append((w.ravel(), rng.normal(0, 1, 8).astype(np.float32)))
    for _ in range(500):    # +-0.0 everywhere: -0.0 == +0.0 is a tie, not a win
        w = rng.choice(np.array([0.0, -0.0, 1.0, -1.0], np.float32), 36)
        o = rng.choice(np.array([0.0, -0.0, 1.0], np.float32), 8)
        out.append((w, o))
    for _ in range(500):    # huge magnitudes: products and sums overflow to +-inf, inf - inf = NaN
        with np.errstate(over="ignore"):
            w = (rng.normal(0, 1, 36) * 10.0 ** rng.integers(30, 39, 36)).astype(np.float32)
        o = (rng.normal(0, 1, 8) * 10.0 ** rng.integers(0, 10, 8)).astype(np.float32)
        out.append((w, o))
    for _ in range(500):    # infinite weights: inf * 0 and inf - inf give NaN scores (never chosen over an earlier row; NaN s_0 -> 0)
        w = rng.normal(0, 1, 36).astype(np.float32)
        w[rng.choice(36, rng.integers(1, 4), replace=False)] = rng.choice(np.array([np.inf, -np.inf], np.float32))
        o = rng.normal(0, 1, 8).astype(np.float32)
        o[rng.random(8) < 0.3] = 0.0
        out.append((w, o))
    return out


def test_linear_action_matches_numpy_restatement(check_exe):
    cs = cases()
    got = run(check_exe, [f"L {hexs(w)} {hexs(o)}" for w, o in cs])
    exp = np.array([lin_ref(w, o) for w, o in cs], np.uint32)
    assert got.shape == exp.shape
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, f"{bad.size} mismatches, first case {cs[bad[0]]}: header {got[bad[0]]}, restatement {exp[bad[0]]}"
    assert all((exp == j).any() for j in range(4))
    # the adversarial kinds really happen: NaN first scores, ties
    nan_first = [i for i, (w, o) in enumerate(cs) if np.isnan(np.float32(lin_score0(w, o)))]
    assert len(nan_first) > 20 and all(got[i] == 0 for i in nan_first)


def lin_score0(w, o):
    with np.errstate(all="ignore"):
        s = np.float32(w[0] * o[0])
        for q in range(1, 8):
            s = np.float32(s + np.float32(w[q] * o[q]))
        return np.float32(s + w[8])


def test_uniform_action_matches_philox_restatement(check_exe):
    rng = np.random.default_rng(11)
    cs = []
    for _ in range(4000):
        seed = int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(0, 2))
        call = int(rng.integers(0, 2 ** 32)) if rng.random() < 0.3 else int(rng.integers(0, 8))
        g = int(rng.integers(0, 2 ** 40)) if rng.random() < 0.3 else int(rng.integers(0, 600000))
        t = int(rng.integers(0, 2 ** 20)) if rng.random() < 0.2 else int(rng.integers(0, 300))
        cs.append((seed, call, g, t))
    got = run(check_exe, [f"U {s} {c} {g} {t}" for s, c, g, t in cs])
    exp = []
    for s, c, g, t in cs:
        w = ora.philox([(g & ~3) & 0xFFFFFFFF, (g & ~3) >> 32, c, 0x40000000 + t // 16], [s & 0xFFFFFFFF, s >> 32])
        exp.append((int(w[g % 4]) >> (2 * (t % 16))) & 3)
    exp = np.array(exp, np.uint32)
    assert np.array_equal(got, exp)
    assert all(0.22 < float((exp == j).mean()) < 0.28 for j in range(4))
