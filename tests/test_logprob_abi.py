"""No-GPU checks of mgym_logprob_mlp's public surface (include/mgym.h): the call is declared in the header, the ctypes table and the Rust FFI with one signature,
the library exports it, the version stays 4, a NULL handle is refused before any HIP call, and VecEnv / TorchVecEnv, the C++ mirror and the Rust wrapper carry it."""
import inspect
import os
import re

import modurl_gym_amd as mg
from abi_surface import check_exported_and_tables_match_the_header, header_params, read
from modurl_gym_amd import _lib, torch_env

NAME = "mgym_logprob_mlp"


def test_the_declaration_is_the_issue_s():
    assert [n for _, n in header_params(NAME)] == ["env", "policy", "hidden1", "hidden2", "activation", "head", "sigma", "K", "obs_first", "obs", "actions", "logp_out"]
    assert [t for t, _ in header_params(NAME)] == ["mgym_env *", "const float *", "int32_t ", "int32_t ", "int32_t ", "int32_t ", "float ", "int32_t ", "const float *",
                                               "const float *", "const void *", "float *"]


def test_the_call_is_exported_and_the_tables_match_the_header():
    check_exported_and_tables_match_the_header(NAME)   # (the one host pointer: the policy's words)


def test_null_handle_is_a_bad_argument():
    lib = _lib.load()
    assert lib.mgym_logprob_mlp(None, None, 8, 0, 0, _lib.HEAD_SAMPLE, 1.0, 1, None, None, None, None) == _lib.ERR_BAD_ARG
    assert b"NULL env handle" in lib.mgym_last_error()


def test_python_surface():
    p = list(inspect.signature(mg.VecEnv.logprob_mlp_device).parameters)
    assert p == ["self", "policy", "hidden1", "hidden2", "activation", "head", "sigma", "K", "obs_first", "obs", "actions", "logp_out"]
    assert list(inspect.signature(mg.VecEnv.logprob_mlp).parameters) == ["self", "weights", "obs_first", "obs", "actions", "activation", "head", "sigma"]
    sig = inspect.signature(torch_env.TorchVecEnv.logprob_mlp)
    assert list(sig.parameters) == ["self", "weights", "obs_first", "obs", "actions", "activation", "head", "sigma"]
    assert sig.parameters["activation"].default == "relu" and sig.parameters["head"].default is None


def test_cpp_and_rust_wrappers():
    assert re.search(r"void logprob_mlp\(const float\* policy, int hidden1, int hidden2, int activation, int head, float sigma, int K, .*?\{\s*check\(%s\(env_, policy, "
                     r"hidden1, hidden2, activation, head, sigma, K, obs_first, obs, actions, logp_out\)\);" % NAME, read("include", "mgym.hpp"), re.S)
    assert re.search(r"pub fn logprob_mlp\(\s*&mut self,\s*policy: &\[f32\],", read("rust", "modurl_gym_mgym", "src", "vec_gym.rs"))


def test_the_documents_describe_the_call():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md", os.path.join("include", "mgym.h"), os.path.join("tools", "README.md")):
        assert NAME in read(doc), doc
    assert "logprob.hip" in read("modurl_gym_amd", "csrc", "Makefile")
    header = read("include", "mgym.h")
    assert "Entropy is not returned" in header and "Nothing is returned from inside the rollout kernels" in header
