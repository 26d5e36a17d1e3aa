"""No-GPU checks of the one host check of the hidden-layer action call itself: tests/native/policy_check.cpp (modurl_gym_amd/csrc/mlp_policy.h and mlp2_policy.h
built for the host with -ffp-contract=off) through tests/policy_header.py, over both depths and every head — that the header's one-per-lane form (N = 1,
LunarLander's) and its four-per-lane form (N = 4, the classic kernels') give the same action words wherever a family has both, and that policy_eval refuses every
combination no family has.  What the words must be is checked per subject: test_mlp_policy_host.py, test_mlp_tanh_fast_host.py, test_mlp_gauss_host.py,
test_mlp2_host.py.  (The GAUSS head has the four-per-lane form only, so for it the first test checks no more than that the call is accepted.)"""
import numpy as np
import pytest

import mlp2_ref as R
import mlp_ref as M
import policy_header as P

F = np.float32

WIDTHS = {1: ((1,), (7,), (64,)), 2: ((1, 1), (3, 5), (64, 64))}
DEPTH_ACTS = {1: (M.RELU, M.TANH, M.TANH_FAST), 2: (M.RELU, M.TANH_FAST)}   # no two-layer source has the exact tanh


@pytest.mark.parametrize("fam", list(R.FAMILIES))
def test_one_per_lane_and_four_per_lane_forms_agree_everywhere(fam):
    """policy_eval's status is 0, never 2 (header_actions asserts it), for every activation, head and depth the family has: n = 8 is two lanes of four, so GREEDY and
    SAMPLE are evaluated in both forms; the observations hold +0, -0, +inf and -inf, the weights +0 and -0"""
    D, A, cont = R.FAMILIES[fam]
    rng = np.random.default_rng(500 + D * 10 + A)
    n, combos = 8, 0
    for depth in (1, 2):
        for widths in WIDTHS[depth]:
            nf = M.n_floats(D, A, *widths) if depth == 1 else R.n_floats(D, A, *widths)
            for act in DEPTH_ACTS[depth]:
                for head in (P.GREEDY, P.GAUSS if cont else P.SAMPLE):
                    pol = rng.normal(0, 1.5, nf).astype(F)
                    pol[rng.random(nf) < 0.1] = rng.choice(np.array([0.0, -0.0], F))
                    obs = rng.normal(0, 1.5, (D, n)).astype(F)
                    for col, v in zip((1, 2, 5, 6), (0.0, -0.0, np.inf, -np.inf)):   # one in each lane's first and second pair
                        obs[rng.integers(0, D), col] = F(v)
                    a, s = P.header_actions(D, A, depth, act, head, widths, pol, obs, 0.75, 0x1234567811, 5, 4096, 3)
                    assert a.shape == (n,) and s.shape == (A, n) and (cont or a.max() < A)
                    combos += 1
    assert combos == 2 * 3 * (3 + 2)


def test_policy_eval_refuses_what_no_family_has():
    """status 1 for each class of combination the check names: a draw on a continuous family, a Gaussian on a discrete one or on an n that is no multiple of 4, a
    width outside 1 .. 64, an unknown activation, head, depth or (D, A), and the exact tanh at depth 2; depth 1 does not read H2"""
    lib = P.check_lib()
    z = np.zeros(8192, F)
    out = np.zeros(8, np.uint32)
    def call(D, A, depth, act, head, H1, H2, n=4):
        return lib.policy_eval(D, A, depth, act, head, H1, H2, z.ctypes.data, 0.0, n, n, z.ctypes.data, out.ctypes.data, out.ctypes.data, None)
    for depth in (1, 2):
        assert call(4, 2, depth, M.RELU, P.GREEDY, 64, 64) == 0 and call(3, 1, depth, M.TANH_FAST, P.GAUSS, 3, 5) == 0
        assert call(3, 1, depth, M.RELU, P.SAMPLE, 3, 5) == 1 and call(2, 1, depth, M.RELU, P.SAMPLE, 3, 5) == 1          # SAMPLE with A == 1
        assert call(4, 2, depth, M.RELU, P.GAUSS, 3, 5) == 1 and call(8, 4, depth, M.RELU, P.GAUSS, 3, 5) == 1            # GAUSS with A != 1
        assert call(3, 1, depth, M.RELU, P.GAUSS, 3, 5, n=6) == 1 and call(3, 1, depth, M.RELU, P.GREEDY, 3, 5, n=6) == 0   # GAUSS with n % 4 != 0
        assert call(4, 2, depth, M.RELU, P.GREEDY, 0, 5) == 1 and call(4, 2, depth, M.RELU, P.GREEDY, 65, 5) == 1          # widths
        assert call(4, 2, depth, 2, P.GREEDY, 3, 5) == 1 and call(4, 2, depth, 4, P.GREEDY, 3, 5) == 1 and call(4, 2, depth, -1, P.GREEDY, 3, 5) == 1   # activation
        assert call(4, 2, depth, M.RELU, 3, 3, 5) == 1 and call(4, 2, depth, M.RELU, -1, 3, 5) == 1                        # head
        assert call(4, 3, depth, M.RELU, P.GREEDY, 3, 5) == 1 and call(5, 2, depth, M.RELU, P.GREEDY, 3, 5) == 1 and call(1, 1, depth, M.RELU, P.GREEDY, 3, 5) == 1   # (D, A)
    assert call(4, 2, 2, M.RELU, P.GREEDY, 5, 0) == 1 and call(4, 2, 2, M.RELU, P.GREEDY, 5, 65) == 1
    assert call(4, 2, 1, M.RELU, P.GREEDY, 5, 0) == 0 and call(4, 2, 1, M.RELU, P.GREEDY, 5, 65) == 0                      # depth 1: H2 is ignored
    assert call(4, 2, 1, M.TANH, P.GREEDY, 3, 5) == 0 and call(4, 2, 2, M.TANH, P.GREEDY, 3, 5) == 1                       # no two-layer exact tanh
    assert call(4, 2, 0, M.RELU, P.GREEDY, 3, 5) == 1 and call(4, 2, 3, M.RELU, P.GREEDY, 3, 5) == 1                       # depth
