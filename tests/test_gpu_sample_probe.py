"""mgym_sample_probe (include/mgym.h): mlp_sample of modurl_gym_amd/csrc/mlp_policy.h compiled for gfx950, one case per lane, against the Python restatement
of the documented draw in tests/mlp_sample_ref.py — the action and c_0 .. c_{A-1}, word for word (NaN as a class) — on the host test's seeded and hand-built
cases and on 2^20 cases per A whose gaps below the best sweep (-104, 0], so that every branch of mg_expm1f on the negative side runs on the device."""
import numpy as np
import pytest

import modurl_gym_amd as mg
import mlp_sample_ref as R
from glibc_f32 import glibc_has_fdlibm_expm1f
from words import same_words
from modurl_gym_amd import _lib

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not glibc_has_fdlibm_expm1f(), reason="this glibc's expm1f is not the fdlibm one that mg_expm1f restates")]


def probe(scores, words, want_cum=True):
    lib = _lib.load()
    A, n = scores.shape
    ds, dw = mg.DeviceArray.from_numpy(np.ascontiguousarray(scores, np.float32)), mg.DeviceArray.from_numpy(np.ascontiguousarray(words, np.uint32))
    da, dc = mg.DeviceArray(n, np.uint32), mg.DeviceArray((A, n), np.float32)
    assert lib.mgym_sample_probe(0, A, n, ds.ptr, dw.ptr, da.ptr, dc.ptr if want_cum else None) == _lib.OK, lib.mgym_last_error()
    return da.numpy(), dc.numpy() if want_cum else None


def check(A, s, w):
    act, cum = probe(s, w)
    ract, rcum = R.draw(s, w)
    bad = np.nonzero(act != ract)[0]
    assert bad.size == 0, f"{bad.size} actions differ; case {bad[0]}: scores {s[:, bad[0]]}, word {w[bad[0]]:#x}: device {act[bad[0]]}, restatement {ract[bad[0]]}"
    assert same_words(cum, rcum)
    return act


@pytest.mark.parametrize("A", [2, 3, 4])
def test_device_draw_equals_the_restatement_on_seeded_and_hand_built_cases(A):
    s, w = R.seeded_cases(A)
    act = check(A, s, w)
    assert set(np.unique(act)) == set(range(A)) and (act != np.argmax(s, axis=0)).sum() > 1000
    assert np.array_equal(probe(s, w, want_cum=False)[0], act)   # cum_out may be NULL
    s, w = R.hand_cases(A)
    check(A, s, w)


@pytest.mark.parametrize("A", [2, 3, 4])
def test_device_draw_equals_the_restatement_on_the_gap_sweep(A):
    s, w = R.gap_sweep_cases(A)
    assert s.shape == (A, 1 << 20)
    gap = s - s.max(axis=0)
    # the regions of mg_expm1f's negative side: 0, below 2^-25, up to 0.5 ln2, up to 1.5 ln2, the general reduction, beyond 27 ln2, beyond 88.72
    for lo, hi in ((-2.0 ** -25, 0.0), (-0.3465, -2.0 ** -25), (-1.0397, -0.3466), (-18.7, -1.04), (-88.7, -18.72), (-112.0, -88.73)):
        assert ((gap < hi) & (gap > lo)).sum() > 1000, (lo, hi)
    assert (gap == 0).any(axis=0).all() and gap.min() > -112.0
    check(A, s, w)


def test_bad_arguments():
    lib = _lib.load()
    s, w = R.seeded_cases(2, 64)
    ds, dw, da = mg.DeviceArray.from_numpy(s), mg.DeviceArray.from_numpy(w), mg.DeviceArray(64, np.uint32)
    for args in ((1, 64, ds.ptr, dw.ptr, da.ptr, None), (5, 64, ds.ptr, dw.ptr, da.ptr, None), (0, 64, ds.ptr, dw.ptr, da.ptr, None), (-2, 64, ds.ptr, dw.ptr, da.ptr, None),
                 (2, 0, ds.ptr, dw.ptr, da.ptr, None), (2, 64, None, dw.ptr, da.ptr, None), (2, 64, ds.ptr, None, da.ptr, None), (2, 64, ds.ptr, dw.ptr, None, None)):
        assert lib.mgym_sample_probe(0, *args) == _lib.ERR_BAD_ARG, args
        assert lib.mgym_last_error().decode().startswith("mgym_sample_probe:")
    assert lib.mgym_sample_probe(0, 2, 64, ds.ptr, dw.ptr, da.ptr, None) == _lib.OK
