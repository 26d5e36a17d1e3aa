"""No-GPU checks of mgym_logprob_mlp's public surface (include/mgym.h): the call is declared in the header, the ctypes table and the Rust FFI with one signature,
the library exports it, the version stays 4, a NULL handle is refused before any HIP call, and VecEnv / TorchVecEnv, the C++ mirror and the Rust wrapper carry it."""
import ctypes as C
import inspect
import os
import re

import modurl_gym_amd as mg
from modurl_gym_amd import _lib, torch_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mgym_logprob_mlp"
C_TYPES = {"mgym_env *": C.c_void_p, "const float *": C.c_void_p, "const void *": C.c_void_p, "float *": C.c_void_p, "int32_t ": C.c_int32, "float ": C.c_float}
RUST_TYPES = {"mgym_env *": "*mut mgym_env", "const float *": "*const f32", "const void *": "*const c_void", "float *": "*mut f32", "int32_t ": "i32", "float ": "f32"}


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def header_params():
    """[(C type as written, name)] of the declaration in include/mgym.h"""
    text = re.sub(r"/\*.*?\*/", "", read("include", "mgym.h"), flags=re.S)
    args = re.search(r"\bint %s\((.*?)\);" % NAME, text, re.S).group(1)
    return [re.fullmatch(r"(.*?[ *])([A-Za-z0-9_]+)", " ".join(a.split())).groups() for a in args.split(",")]


def test_the_declaration_is_the_issue_s():
    assert [n for _, n in header_params()] == ["env", "policy", "hidden1", "hidden2", "activation", "head", "sigma", "K", "obs_first", "obs", "actions", "logp_out"]
    assert [t for t, _ in header_params()] == ["mgym_env *", "const float *", "int32_t ", "int32_t ", "int32_t ", "int32_t ", "float ", "int32_t ", "const float *",
                                               "const float *", "const void *", "float *"]


def test_the_call_is_exported_and_the_tables_match_the_header():
    assert hasattr(C.CDLL(_lib.LIB_PATH), NAME), f"libmgym.so does not export {NAME}"
    res, args = _lib.PROTOTYPES[NAME]
    want = [C_TYPES[t] for t, _ in header_params()]
    want[1] = C.POINTER(C.c_float)   # the one host pointer: the policy's words
    assert res is C.c_int and args == want
    sys_rs = read("rust", "modurl_gym_mgym", "src", "sys.rs")
    decl = re.search(r"pub fn %s\((.*?)\) -> c_int;" % NAME, sys_rs, re.S).group(1)
    rust = [tuple(x.strip() for x in a.split(":")) for a in decl.split(",") if a.strip()]
    assert [t for _, t in rust] == [RUST_TYPES[t] for t, _ in header_params()]
    assert [n for n, _ in rust] == [n.lower() for _, n in header_params()]
    assert _lib.load().mgym_abi_version() == 4   # an added entry point: the version stays
    assert re.search(r"#define MGYM_ABI_VERSION 4\b", read("include", "mgym.h"))


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
