"""Shared by test_mlp_policy_host.py and the GPU suites of mgym_rollout_mlp: the restatement of tests/mlp_ref.py on one observation (the host-compiled
header is tests/policy_header.py's).  No test here."""
import numpy as np

import mlp_ref as M
from mlp_ref import FAMILIES, RELU, TANH, n_floats, split  # noqa: F401
from words import words_of


def mlp_refs(D, A, cont, act, H, policies, obs):
    """m cases of one shape at once: policies [m, n_floats], obs [m, D] -> (action words [m], scores [m, A], hidden pre-activations [m, H])"""
    s, pres = M.scores(np.asarray(policies, np.float32).T, D, A, H, np.asarray(obs, np.float32).T, act, want_pre=True)
    return (words_of(s[0]) if cont else M.argmax_words(s)), s.T, pres.T


def mlp_ref(D, A, cont, act, H, policy, o):
    """-> (action word, scores as Python floats, hidden pre-activations) for one observation o [D]"""
    a, s, pres = mlp_refs(D, A, cont, act, H, [policy], [o])
    return int(a[0]), [float(v) for v in s[0]], [float(v) for v in pres[0]]
