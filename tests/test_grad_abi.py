"""No-GPU checks of the public surface of the gradient calls of both depths — mgym_grad_workspace_bytes, mgym_ppo_grad_mlp, mgym_value_grad_mlp and
mgym_grad_workspace_bytes2, mgym_ppo_grad_mlp2, mgym_value_grad_mlp2 (include/mgym.h): each is declared in the header, the ctypes table and the Rust FFI with
one signature, the library exports it, the version stays 4, a NULL handle is refused before any HIP call, the workspace queries (which take no handle) answer
and refuse here, and VecEnv / TorchVecEnv, the C++ mirror and the Rust wrapper carry the calls.  The refusals that need a handle — every one names its
argument — are in tests/test_gpu_grad_mlp.py::test_errors, as mgym_logprob_mlp's are in its device test."""
import ctypes as C
import inspect
import os
import re

import pytest

import modurl_gym_amd as mg
from abi_surface import check_exported_and_tables_match_the_header, header_params, read
from modurl_gym_amd import _lib, torch_env

SLAB_CAP = {1: 1024, 2: 256}
WIDTHS = {1: ((1,), (17,), (64,)), 2: ((1, 1), (17, 9), (64, 64))}
DEPTHS = pytest.mark.parametrize("depth", (1, 2))


def table(depth):
    """(name, parameter names, parameter types) of the depth's query, actor call and critic call, as include/mgym.h declares them"""
    two = "2" if depth == 2 else ""
    hidden = ["hidden"] if depth == 1 else ["hidden1", "hidden2"]
    i32 = ["int32_t "] * depth
    tail = (["workspace", "workspace_bytes", "grad_out", "stats_out"], ["void *", "size_t ", "float *", "float *"])
    return ((f"mgym_grad_workspace_bytes{two}", ["kind", *hidden, "min_bytes", "best_bytes"], ["int ", *i32, "size_t *", "size_t *"]),
            (f"mgym_ppo_grad_mlp{two}",
             ["env", "policy", *hidden, "activation", "head", "sigma", "K", "env_first", "env_count", "obs_first", "obs", "actions", "logp_old", "adv", "clip", "ent_coef", *tail[0]],
             ["mgym_env *", "const float *", *i32, "int32_t ", "int32_t ", "float ", "int32_t ", "uint64_t ", "uint64_t ", "const float *", "const float *", "const void *",
              "const float *", "const float *", "float ", "float ", *tail[1]]),
            (f"mgym_value_grad_mlp{two}", ["env", "critic", *hidden, "activation", "K", "env_first", "env_count", "obs_first", "obs", "ret", *tail[0]],
             ["mgym_env *", "const float *", *i32, "int32_t ", "int32_t ", "uint64_t ", "uint64_t ", "const float *", "const float *", "const float *", *tail[1]]))


NAMES = [name for depth in (1, 2) for name, _, _ in table(depth)]


@DEPTHS
def test_the_declarations_are_the_issue_s(depth):
    for name, names, types in table(depth):
        assert header_params(name) == list(zip(types, names)), name


@pytest.mark.parametrize("name", NAMES)
def test_the_call_is_exported_and_the_tables_match_the_header(name):
    check_exported_and_tables_match_the_header(name, None if "workspace" in name else 1)   # (the one host pointer: the weights' words)


@DEPTHS
def test_null_handle_is_a_bad_argument(depth):
    lib = _lib.load()
    (_, _, _), (ppo, _, _), (value, _, _) = table(depth)
    hidden = (8,) * depth
    assert getattr(lib, ppo)(None, None, *hidden, 0, _lib.HEAD_SAMPLE, 1.0, 1, 0, 1, None, None, None, None, None, 0.2, 0.0, None, 0, None, None) == _lib.ERR_BAD_ARG
    assert b"NULL env handle" in lib.mgym_last_error()
    assert getattr(lib, value)(None, None, *hidden, 0, 1, 0, 1, None, None, None, None, 0, None, None) == _lib.ERR_BAD_ARG
    assert b"NULL env handle" in lib.mgym_last_error()


@DEPTHS
def test_the_workspace_query_needs_no_device(depth):
    lib, lo, hi = _lib.load(), C.c_size_t(), C.c_size_t()
    name, params, _ = table(depth)[0]
    query = getattr(lib, name)
    dims = {mg.CARTPOLE: (4, 2), mg.MOUNTAINCAR: (2, 3), mg.MOUNTAINCAR_CONT: (2, 1), mg.PENDULUM: (3, 1), mg.ACROBOT: (6, 3), mg.LUNARLANDER: (8, 4)}
    for kind, (D, A) in dims.items():
        for widths in WIDTHS[depth]:
            assert query(kind, *widths, C.byref(lo), C.byref(hi)) == _lib.OK
            floats = sum(h * (d + 1) for h, d in zip((*widths, A), (D, *widths)))
            assert lo.value == 8 * (floats + 8) and hi.value == SLAB_CAP[depth] * lo.value and lo.value % 8 == 0
            if depth == 2:
                one = C.c_size_t()
                assert lib.mgym_grad_workspace_bytes(kind, widths[0], C.byref(one), C.byref(hi)) == _lib.OK and one.value < lo.value   # the one-layer size is too small
    good = dict(zip(params, (mg.CARTPOLE, *(8,) * depth, lo, hi)))
    rows = [({"kind": 99}, b"kind"), ({"kind": -1}, b"kind"), ({"min_bytes": None}, b"min_bytes"), ({"best_bytes": None}, b"best_bytes")]
    rows += [({h: bad}, h.encode()) for h in params[1: 1 + depth] for bad in (0, 65)]
    for repl, needle in rows:
        a = {**good, **repl}
        st = query(*(x if x is None or isinstance(x, int) else C.byref(x) for x in a.values()))
        msg = lib.mgym_last_error()
        assert st == _lib.ERR_BAD_ARG and msg.startswith(name.encode() + b":") and needle in msg, msg


@DEPTHS
def test_python_surface(depth):
    two = "2" if depth == 2 else ""
    (_, query, _), (_, ppo, _), (_, value, _) = table(depth)
    params = lambda cls, name: list(inspect.signature(getattr(cls, name)).parameters)
    assert params(mg.VecEnv, f"grad_workspace_bytes{two}") == ["self"] + query[1: 1 + depth]
    assert params(mg.VecEnv, f"ppo_grad_mlp{two}_device") == ["self"] + ppo[1:]
    assert params(mg.VecEnv, f"value_grad_mlp{two}_device") == ["self"] + value[1:]
    host = params(mg.VecEnv, f"ppo_grad_mlp{two}")
    assert host[:7] == ["self", "weights", "obs_first", "obs", "actions", "logp_old", "adv"] and "env_slice" in host
    assert params(mg.VecEnv, f"value_grad_mlp{two}")[:5] == ["self", "weights", "obs_first", "obs", "ret"]
    sig = inspect.signature(getattr(torch_env.TorchVecEnv, f"ppo_grad_mlp{two}"))
    assert list(sig.parameters) == ["self", "weights", "obs_first", "obs", "actions", "logp_old", "adv", "activation", "head", "sigma", "clip", "ent_coef", "env_slice"]
    assert sig.parameters["env_slice"].default is None and sig.parameters["activation"].default == "relu"
    assert params(torch_env.TorchVecEnv, f"value_grad_mlp{two}") == ["self", "critic", "obs_first", "obs", "ret", "activation", "env_slice"]


@DEPTHS
def test_cpp_and_rust_wrappers(depth):
    hpp, rs = read("include", "mgym.hpp"), read("rust", "modurl_gym_mgym", "src", "vec_gym.rs")
    two = "2" if depth == 2 else ""
    hidden = ["hidden"] if depth == 1 else ["hidden1", "hidden2"]
    ints, names = ", ".join(f"int {h}" for h in hidden), ", ".join(hidden)
    # (the one- and the two-layer mirrors break their argument lists at different places)
    assert re.search(r"void ppo_grad_mlp%s\(const float\* policy, %s, .*?\{\s*check\(mgym_ppo_grad_mlp%s\(env_, policy, %s, activation, head, sigma, K, env_first, "
                     r"env_count, obs_first, obs, actions, logp_old, adv, clip,\s*ent_coef,\s*workspace, workspace_bytes, grad_out, stats_out\)\);" % (two, ints, two, names),
                     hpp, re.S)
    assert re.search(r"void value_grad_mlp%s\(const float\* critic, %s, .*?\{\s*check\(mgym_value_grad_mlp%s\(env_, critic, %s, activation, K, env_first, env_count, "
                     r"obs_first, obs, ret, workspace, workspace_bytes, grad_out,\s*stats_out\)\);" % (two, ints, two, names), hpp, re.S)
    assert f"mgym_grad_workspace_bytes{two}(kind, {names}, min_bytes, best_bytes)" in hpp
    widths = "".join(r"\s*%s: i32," % h for h in hidden) if depth == 2 else ""
    for fn in ("ppo_grad_mlp", "value_grad_mlp"):
        assert re.search(r"pub fn %s%s\(\s*&mut self,\s*(policy|critic): &\[f32\],%s" % (fn, two, widths), rs)
    assert f"pub fn grad_workspace_bytes{two}(kind: i32, {', '.join(f'{h}: i32' for h in hidden)})" in rs


@DEPTHS
def test_the_documents_describe_the_calls(depth):
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md", os.path.join("include", "mgym.h"), os.path.join("tools", "README.md")):
        for name, _, _ in table(depth)[1:]:
            assert name in read(doc), (doc, name)
    header = read("include", "mgym.h")
    if depth == 1:
        assert "grad.hip" in read("modurl_gym_amd", "csrc", "Makefile")
        for text in (header, read("modurl_gym_amd", "csrc", "grad.h"), read("README.md")):
            for phrase in ("wo hidden layers", "optimizer step", "dvantage normalisation", "lat-index minibatches", "clipped value loss"):
                assert phrase in text, phrase
        assert "the caller's error" in header and "No float atomics" in header
    else:
        assert "grad2.hip" in read("modurl_gym_amd", "csrc", "Makefile")
        for text in (header, read("modurl_gym_amd", "csrc", "grad2.h")):
            for phrase in ("dh2_k", "dpre2_k", "dh1_j", "dpre1_j", "dW3[a][k]"):
                assert phrase in text, phrase
        assert "mgym_grad_workspace_bytes2" in header and "5j" in read("DESIGN.md") and "--hidden2" in read("tools", "README.md")
