"""No-GPU checks of the public surface of mgym_grad_workspace_bytes, mgym_ppo_grad_mlp and mgym_value_grad_mlp (include/mgym.h): each is declared in the header,
the ctypes table and the Rust FFI with one signature, the library exports it, the version stays 4, a NULL handle is refused before any HIP call, the workspace
query (which takes no handle) answers and refuses here, and VecEnv / TorchVecEnv, the C++ mirror and the Rust wrapper carry the calls.  The refusals that need a
handle — every one names its argument — are in tests/test_gpu_grad_mlp.py::test_errors, as mgym_logprob_mlp's are in its device test."""
import ctypes as C
import inspect
import os
import re

import pytest

import modurl_gym_amd as mg
from abi_surface import check_exported_and_tables_match_the_header, header_params, read
from modurl_gym_amd import _lib, torch_env

NAMES = ("mgym_grad_workspace_bytes", "mgym_ppo_grad_mlp", "mgym_value_grad_mlp")
PPO = ["env", "policy", "hidden", "activation", "head", "sigma", "K", "env_first", "env_count", "obs_first", "obs", "actions", "logp_old", "adv", "clip", "ent_coef",
       "workspace", "workspace_bytes", "grad_out", "stats_out"]
VALUE = ["env", "critic", "hidden", "activation", "K", "env_first", "env_count", "obs_first", "obs", "ret", "workspace", "workspace_bytes", "grad_out", "stats_out"]


def test_the_declarations_are_the_issue_s():
    assert header_params(NAMES[0]) == [("int ", "kind"), ("int32_t ", "hidden"), ("size_t *", "min_bytes"), ("size_t *", "best_bytes")]
    assert [n for _, n in header_params(NAMES[1])] == PPO and [n for _, n in header_params(NAMES[2])] == VALUE
    assert [t for t, _ in header_params(NAMES[1])] == ["mgym_env *", "const float *", "int32_t ", "int32_t ", "int32_t ", "float ", "int32_t ", "uint64_t ", "uint64_t ",
                                                       "const float *", "const float *", "const void *", "const float *", "const float *", "float ", "float ", "void *",
                                                       "size_t ", "float *", "float *"]
    assert [t for t, _ in header_params(NAMES[2])] == ["mgym_env *", "const float *", "int32_t ", "int32_t ", "int32_t ", "uint64_t ", "uint64_t ", "const float *",
                                                       "const float *", "const float *", "void *", "size_t ", "float *", "float *"]


@pytest.mark.parametrize("name", NAMES)
def test_the_call_is_exported_and_the_tables_match_the_header(name):
    check_exported_and_tables_match_the_header(name, None if name == NAMES[0] else 1)   # (the one host pointer: the weights' words)


def test_null_handle_is_a_bad_argument():
    lib = _lib.load()
    assert lib.mgym_ppo_grad_mlp(None, None, 8, 0, _lib.HEAD_SAMPLE, 1.0, 1, 0, 1, None, None, None, None, None, 0.2, 0.0, None, 0, None, None) == _lib.ERR_BAD_ARG
    assert b"NULL env handle" in lib.mgym_last_error()
    assert lib.mgym_value_grad_mlp(None, None, 8, 0, 1, 0, 1, None, None, None, None, 0, None, None) == _lib.ERR_BAD_ARG
    assert b"NULL env handle" in lib.mgym_last_error()


def test_the_workspace_query_needs_no_device():
    lib, lo, hi = _lib.load(), C.c_size_t(), C.c_size_t()
    dims = {mg.CARTPOLE: (4, 2), mg.MOUNTAINCAR: (2, 3), mg.MOUNTAINCAR_CONT: (2, 1), mg.PENDULUM: (3, 1), mg.ACROBOT: (6, 3), mg.LUNARLANDER: (8, 4)}
    for kind, (D, A) in dims.items():
        for H in (1, 17, 64):
            assert lib.mgym_grad_workspace_bytes(kind, H, C.byref(lo), C.byref(hi)) == _lib.OK
            assert lo.value == 8 * (H * (D + 1) + A * (H + 1) + 8) and hi.value == 1024 * lo.value and lo.value % 8 == 0
    for kind, H, a, b, needle in ((99, 8, lo, hi, b"kind"), (-1, 8, lo, hi, b"kind"), (mg.CARTPOLE, 0, lo, hi, b"hidden"), (mg.CARTPOLE, 65, lo, hi, b"hidden"),
                                  (mg.CARTPOLE, 8, None, hi, b"min_bytes"), (mg.CARTPOLE, 8, lo, None, b"best_bytes")):
        st = lib.mgym_grad_workspace_bytes(kind, H, None if a is None else C.byref(a), None if b is None else C.byref(b))
        msg = lib.mgym_last_error()
        assert st == _lib.ERR_BAD_ARG and msg.startswith(b"mgym_grad_workspace_bytes:") and needle in msg, msg


def test_python_surface():
    assert list(inspect.signature(mg.VecEnv.grad_workspace_bytes).parameters) == ["self", "hidden"]
    p = list(inspect.signature(mg.VecEnv.ppo_grad_mlp_device).parameters)
    assert p == ["self"] + PPO[1:]
    assert list(inspect.signature(mg.VecEnv.value_grad_mlp_device).parameters) == ["self"] + VALUE[1:]
    host = list(inspect.signature(mg.VecEnv.ppo_grad_mlp).parameters)
    assert host[:7] == ["self", "weights", "obs_first", "obs", "actions", "logp_old", "adv"] and "env_slice" in host
    assert list(inspect.signature(mg.VecEnv.value_grad_mlp).parameters)[:5] == ["self", "weights", "obs_first", "obs", "ret"]
    sig = inspect.signature(torch_env.TorchVecEnv.ppo_grad_mlp)
    assert list(sig.parameters) == ["self", "weights", "obs_first", "obs", "actions", "logp_old", "adv", "activation", "head", "sigma", "clip", "ent_coef", "env_slice"]
    assert sig.parameters["env_slice"].default is None and sig.parameters["activation"].default == "relu"
    assert list(inspect.signature(torch_env.TorchVecEnv.value_grad_mlp).parameters) == ["self", "critic", "obs_first", "obs", "ret", "activation", "env_slice"]


def test_cpp_and_rust_wrappers():
    hpp, rs = read("include", "mgym.hpp"), read("rust", "modurl_gym_mgym", "src", "vec_gym.rs")
    assert re.search(r"void ppo_grad_mlp\(const float\* policy, int hidden, .*?\{\s*check\(mgym_ppo_grad_mlp\(env_, policy, hidden, activation, head, sigma, K, env_first, "
                     r"env_count, obs_first, obs, actions, logp_old, adv, clip, ent_coef,\s*workspace, workspace_bytes, grad_out, stats_out\)\);", hpp, re.S)
    assert re.search(r"void value_grad_mlp\(const float\* critic, int hidden, .*?\{\s*check\(mgym_value_grad_mlp\(env_, critic, hidden, activation, K, env_first, env_count, "
                     r"obs_first, obs, ret, workspace, workspace_bytes, grad_out, stats_out\)\);", hpp, re.S)
    assert "mgym_grad_workspace_bytes(kind, hidden, min_bytes, best_bytes)" in hpp
    for fn in ("ppo_grad_mlp", "value_grad_mlp"):
        assert re.search(r"pub fn %s\(\s*&mut self,\s*(policy|critic): &\[f32\]," % fn, rs)
    assert "pub fn grad_workspace_bytes(kind: i32, hidden: i32)" in rs


def test_the_documents_describe_the_calls():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md", os.path.join("include", "mgym.h"), os.path.join("tools", "README.md")):
        for name in NAMES[1:]:
            assert name in read(doc), (doc, name)
    assert "grad.hip" in read("modurl_gym_amd", "csrc", "Makefile")
    header, gradh = read("include", "mgym.h"), read("modurl_gym_amd", "csrc", "grad.h")
    for text in (header, gradh, read("README.md")):
        for phrase in ("wo hidden layers", "optimizer step", "dvantage normalisation", "lat-index minibatches", "clipped value loss"):
            assert phrase in text, phrase
    assert "the caller's error" in header and "No float atomics" in header
