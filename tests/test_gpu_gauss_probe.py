"""mgym_gauss_probe (include/mgym.h): mlp_gauss_pair of modurl_gym_amd/csrc/mlp_policy.h compiled for gfx950, one pair of Philox words per lane, against the
same lines compiled for the host (tests/native/mlp_gauss_check.cpp, which tests/test_mlp_gauss_host.py pins to the numpy restatement of the documented draw):
z_even, z_odd and q word for word over all 2^24 values of k1 — so the f64 division, the f32 square root and the sincos of the device are the host's."""
import numpy as np
import pytest

import modurl_gym_amd as mg
import mlp_gauss_ref as R
from modurl_gym_amd import _lib

pytestmark = pytest.mark.gpu


def probe(wa, wb, want_q=True):
    lib = _lib.load()
    n = wa.size
    da, db = mg.DeviceArray.from_numpy(np.ascontiguousarray(wa, np.uint32)), mg.DeviceArray.from_numpy(np.ascontiguousarray(wb, np.uint32))
    ze, zo, q = (mg.DeviceArray(n, np.float32) for _ in range(3))
    assert lib.mgym_gauss_probe(0, n, da.ptr, db.ptr, ze.ptr, zo.ptr, q.ptr if want_q else None) == _lib.OK, lib.mgym_last_error()
    return ze.numpy(), zo.numpy(), q.numpy() if want_q else None


def test_device_pair_equals_the_host_compiled_header_on_every_k1():
    """one launch over 2^24 + the hand cases: five device buffers of 64 MiB"""
    wa, wb = R.all_cases()
    assert wa.size == (1 << 24) + len(R.K1_HAND) * len(R.K2_HAND)
    got = probe(wa, wb)
    exp = R.header_pair(wa, wb)
    for nm, g, e in zip(("z_even", "z_odd", "q"), got, exp):
        bad = np.nonzero(g.view(np.uint32) != e.view(np.uint32))[0]
        assert bad.size == 0, f"{nm}: {bad.size} words differ; first at wa {wa[bad[0]]:#x} wb {wb[bad[0]]:#x}: device {g[bad[0]]!r}, host {e[bad[0]]!r}"
    # q_out may be NULL
    ze, zo, _ = probe(wa[:4096], wb[:4096], want_q=False)
    assert np.array_equal(ze.view(np.uint32), exp[0][:4096].view(np.uint32)) and np.array_equal(zo.view(np.uint32), exp[1][:4096].view(np.uint32))


def test_bad_arguments():
    lib = _lib.load()
    w = mg.DeviceArray.from_numpy(np.arange(64, dtype=np.uint32))
    z = mg.DeviceArray(64, np.float32)
    for args in ((0, w.ptr, w.ptr, z.ptr, z.ptr, None), (64, None, w.ptr, z.ptr, z.ptr, None), (64, w.ptr, None, z.ptr, z.ptr, None), (64, w.ptr, w.ptr, None, z.ptr, None),
                 (64, w.ptr, w.ptr, z.ptr, None, None), ((1 << 31) + 1, w.ptr, w.ptr, z.ptr, z.ptr, None)):
        assert lib.mgym_gauss_probe(0, *args) == _lib.ERR_BAD_ARG, args
        assert lib.mgym_last_error().decode().startswith("mgym_gauss_probe:")
    assert lib.mgym_gauss_probe(0, 64, w.ptr, w.ptr, z.ptr, z.ptr, None) == _lib.OK
