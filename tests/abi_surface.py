"""What the no-GPU checks of an entry point's public surface share (test_value_abi.py, test_logprob_abi.py, test_grad_abi.py): the repository's files, the
declaration as include/mgym.h writes it, and the check that the library, the ctypes table and the Rust FFI carry that declaration.  No test here."""
import ctypes as C
import os
import re

from modurl_gym_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_TYPES = {"mgym_env *": C.c_void_p, "const float *": C.c_void_p, "const uint8_t *": C.c_void_p, "const void *": C.c_void_p, "float *": C.c_void_p, "void *": C.c_void_p,
           "int32_t ": C.c_int32, "float ": C.c_float, "uint64_t ": C.c_uint64, "size_t ": C.c_size_t, "int ": C.c_int, "size_t *": C.POINTER(C.c_size_t)}
RUST_TYPES = {"mgym_env *": "*mut mgym_env", "const float *": "*const f32", "const uint8_t *": "*const u8", "const void *": "*const c_void", "float *": "*mut f32",
              "void *": "*mut c_void", "int32_t ": "i32", "float ": "f32", "uint64_t ": "u64", "size_t ": "usize", "int ": "c_int", "size_t *": "*mut usize"}


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def header_params(name):
    """[(C type as written, name)] of the declaration in include/mgym.h"""
    text = re.sub(r"/\*.*?\*/", "", read("include", "mgym.h"), flags=re.S)
    args = re.search(r"\bint %s\((.*?)\);" % name, text, re.S).group(1)
    return [re.fullmatch(r"(.*?[ *])([A-Za-z0-9_]+)", " ".join(a.split())).groups() for a in args.split(",")]


def check_exported_and_tables_match_the_header(name, host_pointer=1):
    """libmgym.so exports `name`; the ctypes table and the Rust FFI declare it as the header does, argument `host_pointer` (None: none) being the one host
    pointer, the weights' words; an added entry point leaves the version at 4"""
    assert hasattr(C.CDLL(_lib.LIB_PATH), name), f"libmgym.so does not export {name}"
    res, args = _lib.PROTOTYPES[name]
    want = [C_TYPES[t] for t, _ in header_params(name)]
    if host_pointer is not None:
        want[host_pointer] = C.POINTER(C.c_float)
    assert res is C.c_int and args == want
    sys_rs = read("rust", "modurl_gym_mgym", "src", "sys.rs")
    decl = re.search(r"pub fn %s\((.*?)\) -> c_int;" % name, sys_rs, re.S).group(1)
    rust = [tuple(x.strip() for x in a.split(":")) for a in decl.split(",") if a.strip()]
    assert [t for _, t in rust] == [RUST_TYPES[t] for t, _ in header_params(name)]
    assert [n for n, _ in rust] == [n.lower() for _, n in header_params(name)]
    assert _lib.load().mgym_abi_version() == 4
    assert re.search(r"#define MGYM_ABI_VERSION 4\b", read("include", "mgym.h"))
