"""The device's mg_tanhf_fast (mgym_act_probe with MGYM_ACT_TANH_FAST: csrc/mgym_math.h compiled for gfx950) against the same header compiled for the host
(tests/native/tanh_fast_check.cpp, which tests/test_tanh_fast_host.py holds to the text of include/mgym.h and to float64 tanh), bit for bit, NaNs as a class.
This sees what only the device build can get wrong: denormal flushing of u and r * r, contraction, or a divide or a round-to-nearest that is not IEEE's.

Patterns: every one from 0 to just past the clamp, [0, 0x41200100), in chunks as tests/test_gpu_math_exhaustive.py does.  Above that every
2^8-th pattern up to the infinity and the NaNs, and the same set with the sign bit set, would be enough; the probe takes contiguous spans, so those two
ranges are probed and compared whole, which contains the sampled sets; so is the negative side below the clamp.  All 2^32 patterns take
about a second and a half on an MI355X."""
import ctypes as C
import time

import numpy as np
import pytest

import native_build
import tanh_fast_ref as T
from glibc_f32 import tanhf
from words import same_words
from modurl_gym_amd import _lib

pytestmark = pytest.mark.gpu

CHUNK = 1 << 26   # patterns per probe launch: 256 MiB of result words
RANGES = {"below_clamp": (0x00000000, T.CLAMP_END), "above_clamp": (T.CLAMP_END, 0x80000000), "negative_above_clamp": (0x80000000 + T.CLAMP_END, 1 << 32),
          "negative_below_clamp": (0x80000000, 0x80000000 + T.CLAMP_END)}


@pytest.fixture(scope="module")
def host():
    """the host build of the header; with the CPU's own FMA instruction where it has one (one correctly rounded operation, as glibc's fmaf is, and inline)"""
    return T.check_lib(fma=native_build.host_has_fma())


@pytest.fixture(scope="module")
def device_buffer():
    lib = _lib.load()
    dev = C.c_void_p()
    assert lib.mgym_malloc(0, CHUNK * 4, C.byref(dev)) == _lib.OK, lib.mgym_last_error()
    yield dev
    lib.mgym_free(0, dev)


@pytest.mark.parametrize("name", list(RANGES))
def test_device_words_equal_the_host_build(host, device_buffer, name):
    lib = _lib.load()
    lo, hi = RANGES[name]
    words = np.empty(CHUNK, np.uint32)
    bad_total, first_bad, t0 = 0, None, time.perf_counter()
    fb = C.c_uint32(0)
    for first in range(lo, hi, CHUNK):
        count = min(CHUNK, hi - first)
        assert lib.mgym_act_probe(0, _lib.ACT_TANH_FAST, first, count, device_buffer) == _lib.OK, lib.mgym_last_error()
        assert lib.mgym_memcpy_d2h(0, words.ctypes.data, device_buffer, count * 4) == _lib.OK, lib.mgym_last_error()
        bad = host.tanh_fast_compare(first, count, words.ctypes.data, C.byref(fb))
        if bad and first_bad is None:
            x = np.array([fb.value], np.uint32)
            first_bad = (hex(fb.value), hex(int(words[fb.value - first])), hex(int(T.words_of(T.header_tanh_fast(x))[0])))
        bad_total += int(bad)
    print(f"\n{name}: {hi - lo} patterns in {time.perf_counter() - t0:.2f} s")
    assert bad_total == 0, f"{name}: {bad_total} patterns differ; first (pattern, device, host): {first_bad}"


def test_the_fma_build_of_the_host_header_is_the_glibc_fmaf_build(host):
    """the comparison above may run the host header with the CPU's FMA instruction: the same words as the build that calls glibc's fmaf"""
    idx = np.arange(1 << 18, dtype=np.uint64)
    from philox_ref import philox4x32_10
    w = np.ascontiguousarray(np.concatenate(philox4x32_10(idx, 1, 2, 3, 0x1234, 0x5678)), np.uint32)
    out = np.empty_like(w)
    host.tanh_fast_bulk(w.size, w.ctypes.data, out.ctypes.data)
    assert same_words(out, T.header_tanh_fast(w))


def test_argument_checks_and_the_other_activations(device_buffer):
    lib = _lib.load()
    dev = device_buffer
    for act in (2, 4, -1):
        assert lib.mgym_act_probe(0, act, 0, 16, dev) == _lib.ERR_BAD_ARG
        assert "activation" in lib.mgym_last_error().decode()
    assert lib.mgym_act_probe(0, _lib.ACT_TANH_FAST, 0, 16, None) == _lib.ERR_BAD_ARG
    assert lib.mgym_act_probe(0, _lib.ACT_TANH_FAST, 0, 0, dev) == _lib.ERR_BAD_ARG
    assert lib.mgym_act_probe(0, _lib.ACT_TANH_FAST, 1, 1 << 32, dev) == _lib.ERR_BAD_ARG
    assert lib.mgym_act_probe(0, _lib.ACT_TANH_FAST, 0xFFFFFFF0, 17, dev) == _lib.ERR_BAD_ARG
    # RELU and TANH are accepted, and their words are mlp_activate's: pre > 0 ? pre : +0, and glibc's tanhf (which mg_tanhf equals: test_gpu_math_exhaustive.py)
    n = 1 << 16
    for first in (0x3F000000, 0xBF000000, 0x00000000, 0x7F7FFF00, 0xFFFF0000):
        n_span = min(n, (1 << 32) - first)
        x = (np.uint32(first) + np.arange(n_span, dtype=np.uint32)).view(np.float32)
        got = np.empty(n_span, np.uint32)
        assert lib.mgym_act_probe(0, _lib.ACT_RELU, first, n_span, dev) == _lib.OK, lib.mgym_last_error()
        assert lib.mgym_memcpy_d2h(0, got.ctypes.data, dev, n_span * 4) == _lib.OK
        with np.errstate(invalid="ignore"):
            relu = np.where(x > 0, x, np.float32(0.0)).astype(np.float32)
        assert np.array_equal(got, relu.view(np.uint32)), hex(first)
        assert lib.mgym_act_probe(0, _lib.ACT_TANH, first, n_span, dev) == _lib.OK, lib.mgym_last_error()
        assert lib.mgym_memcpy_d2h(0, got.ctypes.data, dev, n_span * 4) == _lib.OK
        assert same_words(got.view(np.float32), tanhf(x)), hex(first)
