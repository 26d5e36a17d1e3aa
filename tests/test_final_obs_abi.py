"""No-GPU checks of the final-observation channel's public surface (include/mgym.h: mgym_set_final_obs_out): the call is declared in the header,
the ctypes table and the Rust FFI, the library exports it, a NULL handle is refused before any HIP call, and VecEnv / TorchVecEnv, the C++
mirror and the Rust wrapper carry it."""
import ctypes as C
import inspect
import os
import re

import modurl_gym_amd as mg
from modurl_gym_amd import _lib, torch_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mgym_set_final_obs_out"


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_the_call_is_declared_and_exported():
    assert re.search(r"\bint %s\(mgym_env \*env, float \*final_obs_out, int32_t steps_cap\);" % NAME, read("include", "mgym.h"))
    assert hasattr(C.CDLL(_lib.LIB_PATH), NAME), f"libmgym.so does not export {NAME}"
    assert _lib.PROTOTYPES[NAME] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32])
    assert re.search(r"pub fn %s\(env: \*mut mgym_env, final_obs_out: \*mut f32, steps_cap: i32\) -> c_int;" % NAME, read("rust", "modurl_gym_mgym", "src", "sys.rs"))
    assert _lib.load().mgym_abi_version() == 4   # an added entry point: the version stays


def test_null_handle_is_a_bad_argument():
    lib = _lib.load()
    assert lib.mgym_set_final_obs_out(None, None, 0) == _lib.ERR_BAD_ARG
    assert lib.mgym_set_final_obs_out(None, C.c_void_p(4096), 16) == _lib.ERR_BAD_ARG
    assert b"NULL env handle" in lib.mgym_last_error()


def test_python_surface():
    p = inspect.signature(mg.VecEnv.set_final_obs_out_device).parameters
    assert list(p)[:3] == ["self", "final_obs_out", "steps_cap"]
    assert inspect.signature(torch_env.TorchVecEnv.__init__).parameters["final_obs_steps"].default == 0
    assert list(inspect.signature(torch_env.TorchVecEnv.bootstrap_obs).parameters) == ["self", "obs", "done", "truncated"]


def test_cpp_and_rust_wrappers():
    assert re.search(r"void set_final_obs_out\(float\* final_obs_out, int32_t steps_cap\) \{ check\(%s\(env_, final_obs_out, steps_cap\)\); \}" % NAME, read("include", "mgym.hpp"))
    assert re.search(r"pub fn set_final_obs_out\(&mut self, buf: Option<&mut DeviceBuf<f32>>, steps_cap: i32\)", read("rust", "modurl_gym_mgym", "src", "vec_gym.rs"))


def test_no_document_still_calls_the_final_observation_undeliverable():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md", os.path.join("include", "mgym.h")):
        text = " ".join(read(doc).split())
        assert "truncated episode is not delivered" not in text, doc
        assert NAME in text, doc
