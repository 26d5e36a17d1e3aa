"""No-GPU checks of the public surface of mgym_grad_workspace_bytes2, mgym_ppo_grad_mlp2 and mgym_value_grad_mlp2 (include/mgym.h): each is declared in the
header, the ctypes table and the Rust FFI with one signature, the library exports it, the version stays 4, a NULL handle is refused before any HIP call, the
workspace query (which takes no handle) answers and refuses here, and VecEnv / TorchVecEnv, the C++ mirror and the Rust wrapper carry the calls.  The refusals
that need a handle — every one names its argument — are in tests/test_gpu_grad2_mlp.py::test_errors."""
import ctypes as C
import inspect
import os
import re

import pytest

import modurl_gym_amd as mg
from abi_surface import check_exported_and_tables_match_the_header, header_params, read
from modurl_gym_amd import _lib, torch_env

NAMES = ("mgym_grad_workspace_bytes2", "mgym_ppo_grad_mlp2", "mgym_value_grad_mlp2")
PPO = ["env", "policy", "hidden1", "hidden2", "activation", "head", "sigma", "K", "env_first", "env_count", "obs_first", "obs", "actions", "logp_old", "adv", "clip",
       "ent_coef", "workspace", "workspace_bytes", "grad_out", "stats_out"]
VALUE = ["env", "critic", "hidden1", "hidden2", "activation", "K", "env_first", "env_count", "obs_first", "obs", "ret", "workspace", "workspace_bytes", "grad_out",
         "stats_out"]
SLAB_CAP = 256


def test_the_declarations_are_the_issue_s():
    assert header_params(NAMES[0]) == [("int ", "kind"), ("int32_t ", "hidden1"), ("int32_t ", "hidden2"), ("size_t *", "min_bytes"), ("size_t *", "best_bytes")]
    assert [n for _, n in header_params(NAMES[1])] == PPO and [n for _, n in header_params(NAMES[2])] == VALUE
    assert [t for t, _ in header_params(NAMES[1])] == ["mgym_env *", "const float *", "int32_t ", "int32_t ", "int32_t ", "int32_t ", "float ", "int32_t ", "uint64_t ",
                                                       "uint64_t ", "const float *", "const float *", "const void *", "const float *", "const float *", "float ", "float ",
                                                       "void *", "size_t ", "float *", "float *"]
    assert [t for t, _ in header_params(NAMES[2])] == ["mgym_env *", "const float *", "int32_t ", "int32_t ", "int32_t ", "int32_t ", "uint64_t ", "uint64_t ",
                                                       "const float *", "const float *", "const float *", "void *", "size_t ", "float *", "float *"]


@pytest.mark.parametrize("name", NAMES)
def test_the_call_is_exported_and_the_tables_match_the_header(name):
    check_exported_and_tables_match_the_header(name, None if name == NAMES[0] else 1)   # (the one host pointer: the weights' words)


def test_null_handle_is_a_bad_argument():
    lib = _lib.load()
    assert lib.mgym_ppo_grad_mlp2(None, None, 8, 8, 0, _lib.HEAD_SAMPLE, 1.0, 1, 0, 1, None, None, None, None, None, 0.2, 0.0, None, 0, None, None) == _lib.ERR_BAD_ARG
    assert b"NULL env handle" in lib.mgym_last_error()
    assert lib.mgym_value_grad_mlp2(None, None, 8, 8, 0, 1, 0, 1, None, None, None, None, 0, None, None) == _lib.ERR_BAD_ARG
    assert b"NULL env handle" in lib.mgym_last_error()


def test_the_workspace_query_needs_no_device():
    lib, lo, hi = _lib.load(), C.c_size_t(), C.c_size_t()
    dims = {mg.CARTPOLE: (4, 2), mg.MOUNTAINCAR: (2, 3), mg.MOUNTAINCAR_CONT: (2, 1), mg.PENDULUM: (3, 1), mg.ACROBOT: (6, 3), mg.LUNARLANDER: (8, 4)}
    for kind, (D, A) in dims.items():
        for H1, H2 in ((1, 1), (17, 9), (64, 64)):
            assert lib.mgym_grad_workspace_bytes2(kind, H1, H2, C.byref(lo), C.byref(hi)) == _lib.OK
            assert lo.value == 8 * (H1 * (D + 1) + H2 * (H1 + 1) + A * (H2 + 1) + 8) and hi.value == SLAB_CAP * lo.value
            one = C.c_size_t()
            assert lib.mgym_grad_workspace_bytes(kind, H1, C.byref(one), C.byref(hi)) == _lib.OK and one.value < lo.value   # the one-layer size is too small
    for kind, H1, H2, a, b, needle in ((99, 8, 8, lo, hi, b"kind"), (-1, 8, 8, lo, hi, b"kind"), (mg.CARTPOLE, 0, 8, lo, hi, b"hidden1"), (mg.CARTPOLE, 65, 8, lo, hi, b"hidden1"),
                                       (mg.CARTPOLE, 8, 0, lo, hi, b"hidden2"), (mg.CARTPOLE, 8, 65, lo, hi, b"hidden2"), (mg.CARTPOLE, 8, 8, None, hi, b"min_bytes"),
                                       (mg.CARTPOLE, 8, 8, lo, None, b"best_bytes")):
        st = lib.mgym_grad_workspace_bytes2(kind, H1, H2, None if a is None else C.byref(a), None if b is None else C.byref(b))
        msg = lib.mgym_last_error()
        assert st == _lib.ERR_BAD_ARG and msg.startswith(b"mgym_grad_workspace_bytes2:") and needle in msg, msg


def test_python_surface():
    assert list(inspect.signature(mg.VecEnv.grad_workspace_bytes2).parameters) == ["self", "hidden1", "hidden2"]
    assert list(inspect.signature(mg.VecEnv.ppo_grad_mlp2_device).parameters) == ["self"] + PPO[1:]
    assert list(inspect.signature(mg.VecEnv.value_grad_mlp2_device).parameters) == ["self"] + VALUE[1:]
    host = list(inspect.signature(mg.VecEnv.ppo_grad_mlp2).parameters)
    assert host[:7] == ["self", "weights", "obs_first", "obs", "actions", "logp_old", "adv"] and "env_slice" in host
    assert list(inspect.signature(mg.VecEnv.value_grad_mlp2).parameters)[:5] == ["self", "weights", "obs_first", "obs", "ret"]
    sig = inspect.signature(torch_env.TorchVecEnv.ppo_grad_mlp2)
    assert list(sig.parameters) == ["self", "weights", "obs_first", "obs", "actions", "logp_old", "adv", "activation", "head", "sigma", "clip", "ent_coef", "env_slice"]
    assert sig.parameters["env_slice"].default is None and sig.parameters["activation"].default == "relu"
    assert list(inspect.signature(torch_env.TorchVecEnv.value_grad_mlp2).parameters) == ["self", "critic", "obs_first", "obs", "ret", "activation", "env_slice"]
    # the one-layer forms keep their signatures
    assert list(inspect.signature(mg.VecEnv.grad_workspace_bytes).parameters) == ["self", "hidden"]
    assert list(inspect.signature(mg.VecEnv.ppo_grad_mlp_device).parameters)[1:4] == ["policy", "hidden", "activation"]


def test_cpp_and_rust_wrappers():
    hpp, rs = read("include", "mgym.hpp"), read("rust", "modurl_gym_mgym", "src", "vec_gym.rs")
    assert re.search(r"void ppo_grad_mlp2\(const float\* policy, int hidden1, int hidden2, .*?\{\s*check\(mgym_ppo_grad_mlp2\(env_, policy, hidden1, hidden2, activation, head, "
                     r"sigma, K, env_first, env_count, obs_first, obs, actions, logp_old, adv, clip,\s*ent_coef, workspace, workspace_bytes, grad_out, stats_out\)\);", hpp, re.S)
    assert re.search(r"void value_grad_mlp2\(const float\* critic, int hidden1, int hidden2, .*?\{\s*check\(mgym_value_grad_mlp2\(env_, critic, hidden1, hidden2, activation, K, "
                     r"env_first, env_count, obs_first, obs, ret, workspace, workspace_bytes, grad_out,\s*stats_out\)\);", hpp, re.S)
    assert "mgym_grad_workspace_bytes2(kind, hidden1, hidden2, min_bytes, best_bytes)" in hpp
    for fn in ("ppo_grad_mlp2", "value_grad_mlp2"):
        assert re.search(r"pub fn %s\(\s*&mut self,\s*(policy|critic): &\[f32\],\s*hidden1: i32,\s*hidden2: i32," % fn, rs)
    assert "pub fn grad_workspace_bytes2(kind: i32, hidden1: i32, hidden2: i32)" in rs


def test_the_documents_describe_the_calls():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md", os.path.join("include", "mgym.h"), os.path.join("tools", "README.md")):
        for name in NAMES[1:]:
            assert name in read(doc), (doc, name)
    assert "grad2.hip" in read("modurl_gym_amd", "csrc", "Makefile")
    header, grad2h = read("include", "mgym.h"), read("modurl_gym_amd", "csrc", "grad2.h")
    for text in (header, grad2h):
        for phrase in ("dh2_k", "dpre2_k", "dh1_j", "dpre1_j", "dW3[a][k]"):
            assert phrase in text, phrase
    assert "mgym_grad_workspace_bytes2" in header and "5j" in read("DESIGN.md") and "--hidden2" in read("tools", "README.md")
