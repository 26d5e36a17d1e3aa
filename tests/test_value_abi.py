"""No-GPU checks of mgym_value_mlp's public surface (include/mgym.h): the call is declared in the header, the ctypes table and the Rust FFI with one signature,
the library exports it, a NULL handle is refused before any HIP call, and VecEnv / TorchVecEnv, the C++ mirror and the Rust wrapper carry it."""
import ctypes as C
import inspect
import os
import re

import modurl_gym_amd as mg
from modurl_gym_amd import _lib, torch_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mgym_value_mlp"
C_TYPES = {"mgym_env *": C.c_void_p, "const float *": C.c_void_p, "const uint8_t *": C.c_void_p, "float *": C.c_void_p, "int32_t ": C.c_int32}
RUST_TYPES = {"mgym_env *": "*mut mgym_env", "const float *": "*const f32", "const uint8_t *": "*const u8", "float *": "*mut f32", "int32_t ": "i32"}


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def header_params():
    """[(C type as written, name)] of the declaration in include/mgym.h"""
    text = re.sub(r"/\*.*?\*/", "", read("include", "mgym.h"), flags=re.S)
    args = re.search(r"\bint %s\((.*?)\);" % NAME, text, re.S).group(1)
    return [re.fullmatch(r"(.*?[ *])([A-Za-z0-9_]+)", " ".join(a.split())).groups() for a in args.split(",")]


def test_the_declaration_is_the_issue_s():
    names = [n for _, n in header_params()]
    assert names == ["env", "critic", "hidden1", "hidden2", "activation", "K", "obs_first", "obs", "final_obs", "done", "trunc", "value_out", "last_value_out",
                     "final_value_out"]
    assert [t for t, _ in header_params()] == ["mgym_env *", "const float *", "int32_t ", "int32_t ", "int32_t ", "int32_t ", "const float *", "const float *",
                                               "const float *", "const uint8_t *", "const uint8_t *", "float *", "float *", "float *"]


def test_the_call_is_exported_and_the_tables_match_the_header():
    assert hasattr(C.CDLL(_lib.LIB_PATH), NAME), f"libmgym.so does not export {NAME}"
    res, args = _lib.PROTOTYPES[NAME]
    want = [C_TYPES[t] for t, _ in header_params()]
    want[1] = C.POINTER(C.c_float)   # the one host pointer: the critic's words
    assert res is C.c_int and args == want
    sys_rs = read("rust", "modurl_gym_mgym", "src", "sys.rs")
    decl = re.search(r"pub fn %s\((.*?)\) -> c_int;" % NAME, sys_rs, re.S).group(1)
    rust = [tuple(x.strip() for x in a.split(":")) for a in decl.split(",") if a.strip()]
    assert [t for _, t in rust] == [RUST_TYPES[t] for t, _ in header_params()]
    assert [n for n, _ in rust] == [n.lower() for _, n in header_params()]
    assert _lib.load().mgym_abi_version() == 4   # an added entry point: the version stays


def test_null_handle_is_a_bad_argument():
    lib = _lib.load()
    assert lib.mgym_value_mlp(None, None, 8, 0, 0, 1, None, None, None, None, None, None, None, None) == _lib.ERR_BAD_ARG
    assert b"NULL env handle" in lib.mgym_last_error()


def test_python_surface():
    p = list(inspect.signature(mg.VecEnv.value_mlp_device).parameters)
    assert p == ["self", "critic", "hidden1", "hidden2", "activation", "K", "obs_first", "obs", "final_obs", "done", "trunc", "value_out", "last_value_out",
                 "final_value_out"]
    assert list(inspect.signature(mg.VecEnv.value_mlp).parameters) == ["self", "weights", "obs_first", "obs", "final_obs", "done", "trunc", "activation"]
    sig = inspect.signature(torch_env.TorchVecEnv.value_mlp)
    assert list(sig.parameters) == ["self", "weights", "obs_first", "obs", "done", "truncated", "activation"]
    assert sig.parameters["activation"].default == "relu" and sig.parameters["done"].default is None and sig.parameters["truncated"].default is None


def test_cpp_and_rust_wrappers():
    assert re.search(r"void value_mlp\(const float\* critic, int hidden1, int hidden2, int activation, int K, .*?\{\s*check\(%s\(env_, critic, hidden1, hidden2, "
                     r"activation, K, obs_first, obs, final_obs, done, trunc, value_out, last_value_out, final_value_out\)\);" % NAME, read("include", "mgym.hpp"), re.S)
    assert re.search(r"pub fn value_mlp\(\s*&mut self,\s*critic: &\[f32\],", read("rust", "modurl_gym_mgym", "src", "vec_gym.rs"))


def test_the_documents_describe_the_call():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md", os.path.join("include", "mgym.h"), os.path.join("tools", "README.md")):
        assert NAME in read(doc), doc
    assert "value.hip" in read("modurl_gym_amd", "csrc", "Makefile")
