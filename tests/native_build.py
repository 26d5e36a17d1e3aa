"""The one place that compiles tests/native/*.cpp with g++: program() and shared() return the artefact's path under tests/native/_build/.  Each distinct
(source, name, kind, flags) is compiled once per process, on first use, and always on that first use: an artefact left behind by another checkout is never
loaded unbuilt.  ctypes signatures stay with the module that owns the check program.  No test here."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
BUILD = os.path.join(NATIVE, "_build")
BASE = ("-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math")   # one rounded operation per source operation: what every word comparison rests on
_ORACLE, _PACKAGE = os.path.join(ROOT, "oracle", "_build"), os.path.join(ROOT, "modurl_gym_amd")
ORACLE_LINK = (f"-L{_ORACLE}", "-loracle", f"-Wl,-rpath,{_ORACLE}")   # after oracle.oracle.build()
MGYM_LINK = (f"-L{_PACKAGE}", "-lmgym", f"-Wl,-rpath,{_PACKAGE}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64")

_built = {}


def _compile(src, out, kind, extra, base, link):
    key = (src, out, kind, tuple(extra), tuple(base), tuple(link))
    if key not in _built:
        os.makedirs(BUILD, exist_ok=True)
        path = os.path.join(BUILD, out)
        subprocess.run(["g++", *base, *extra, *kind, "-o", path, os.path.join(NATIVE, src), *link], check=True)
        _built[key] = path
    return _built[key]


def program(src, name=None, extra=(), base=BASE, link=("-lm",)):
    """tests/native/<src> as the program _build/<name> (default: the source's stem): g++ <base> <extra> -o ... <src> <link>.  A call site with its own
    optimisation level passes base=() and the whole of its flags as extra."""
    return _compile(src, name or os.path.splitext(src)[0], (), extra, base, link)


def shared(src, name=None, extra=(), base=BASE, link=("-lm",)):
    """the same as the shared object _build/lib<name>.so"""
    return _compile(src, f"lib{name or os.path.splitext(src)[0]}.so", ("-shared", "-fPIC"), extra, base, link)


def host_has_fma():
    """whether this CPU has the FMA instruction glibc selects its sinf / cosf build by (and -mfma compiles fmaf to)"""
    with open("/proc/cpuinfo") as f:
        return any(line.startswith("flags") and " fma " in f" {line.split(':', 1)[1].strip()} " for line in f)
