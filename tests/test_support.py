"""The support layer the other tests stand on: philox_ref's Philox against the published vectors, the two meanings of word equality in words.py,
glibc_f32.fmaf's single rounding and broadcasting, native_build's one compilation per process, the family table of families.py against the library's spec,
and the buffers of device_buffers.py on host memory: each stray write they exist to catch is caught.  No GPU."""
import os

import numpy as np
import pytest

import device_buffers as B
import glibc_f32
import native_build
import philox_ref
from families import FAMILIES
from words import same, same_words

F = np.float32


def f32(*words):
    return np.array(words, np.uint32).view(F)


def test_philox_gives_the_published_known_answers():
    """the three vectors of the Random123 distribution's kat_vectors for philox4x32 with 10 rounds"""
    kat = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))
    for ctr, key, out in kat:
        assert tuple(int(v) for v in philox_ref.philox4x32_10(*ctr, *key)) == out
    # over arrays: the three at once in the counter, one key
    got = np.stack(philox_ref.philox4x32_10(*np.array([k[0] for k in kat], np.uint64).T, *kat[2][1]), axis=1)
    assert tuple(int(v) for v in got[2]) == kat[2][2] and got.dtype == np.uint32


def test_block_words_key_the_block_of_four_and_env_draw_the_environment():
    seed, call, slot = 0x1234567811, 3, philox_ref.SLOT_POLICY_SAMPLE + 5
    g = np.array([4, 5, 6, 7, (1 << 32) + 5], np.uint64)
    w = philox_ref.block_words(seed, call, g, slot)
    for i, gi in enumerate(int(v) for v in g):
        exp = philox_ref.philox4x32_10((gi & ~3) & 0xFFFFFFFF, (gi & ~3) >> 32, call, slot, seed & 0xFFFFFFFF, seed >> 32)
        assert [int(v[i]) for v in w] == [int(v) for v in exp]
        assert int(philox_ref.own_word(seed, call, g, slot)[i]) == int(exp[gi % 4])
        assert [int(v[i]) for v in philox_ref.env_draw(seed, g, 9, 1)] == [int(v) for v in philox_ref.philox4x32_10(gi & 0xFFFFFFFF, gi >> 32, 9, 1, seed & 0xFFFFFFFF, seed >> 32)]
    assert (philox_ref.SLOT_POLICY, philox_ref.SLOT_POLICY_SAMPLE, philox_ref.SLOT_POLICY_GAUSS) == (0x40000000, 0x50000000, 0x60000000)


def test_same_words_takes_nans_as_a_class_and_same_takes_nothing_as_one():
    nan_a, nan_b, zeros = f32(0x7FC00000, 0x3F800000), f32(0xFFC0DEAD, 0x3F800000), (f32(0x00000000), f32(0x80000000))
    assert same_words(nan_a, nan_b) and not same(nan_a, nan_b)
    assert not same_words(*zeros) and not same(*zeros)
    assert same_words(nan_a, nan_a.copy()) and same(nan_a, nan_a.copy())
    assert not same_words(nan_a, f32(0x7FC00000, 0x3F800001))                     # a NaN beside a difference does not hide it
    assert same_words(nan_a.view(np.uint32), nan_b)                               # uint32 arrays are words, not numbers to convert
    assert same(np.arange(3, dtype=np.uint8), np.arange(3, dtype=np.uint8)) and not same(np.zeros(3, F), np.zeros(4, F))


def test_fmaf_rounds_once():
    """a = b = 1 + 2^-12: a * b = 1 + 2^-11 + 2^-24 is exactly halfway between two floats, and c = 2^-60 lifts it above the tie.  One rounding gives the upper
    neighbour; the float64 sum cannot hold the 2^-60, is the tie itself, and rounds to even, the lower one.  (Constructed, then confirmed by running it.)"""
    a, b, c = f32(0x3F800800), f32(0x3F800800), f32(0x21800000)
    twice = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)
    assert twice.view(np.uint32)[0] == 0x3F801000
    assert glibc_f32.fmaf(a, b, c).view(np.uint32)[0] == 0x3F801001
    assert glibc_f32.fmaf_scalar(a[0], b[0], c[0]).view(np.uint32) == 0x3F801001


def test_fmaf_broadcasts_scalars():
    rng = np.random.default_rng(3)
    b, c = rng.normal(0, 1, 1000).astype(F), rng.normal(0, 1, 1000).astype(F)
    a = F(1.0000001)
    whole = glibc_f32.fmaf(np.full(1000, a, F), b, c)
    assert same(glibc_f32.fmaf(a, b, c), whole) and same(glibc_f32.fmaf(b, a, c), whole)
    assert same(glibc_f32.fmaf(b, c, a), glibc_f32.fmaf(b, c, np.full(1000, a, F)))
    assert same(whole[:8], np.array([glibc_f32.fmaf_scalar(a, b[i], c[i]) for i in range(8)], F))
    assert glibc_f32.fmaf(a, b.reshape(10, 100), c.reshape(10, 100)).shape == (10, 100)


def test_each_artefact_is_compiled_once_per_process():
    first = native_build.shared("glibc_f32.cpp")
    assert first == os.path.join(native_build.BUILD, "libglibc_f32.so")
    mtime = os.stat(first).st_mtime_ns
    assert native_build.shared("glibc_f32.cpp") == first and os.stat(first).st_mtime_ns == mtime      # no second run of the compiler
    stale = os.path.join(native_build.BUILD, "libglibc_f32_again.so")                                  # what another checkout might have left behind
    with open(stale, "wb") as f:
        f.write(b"not a shared object")
    other = native_build.shared("glibc_f32.cpp", "glibc_f32_again")                                    # another key: compiled on its first use, whatever is there
    with open(other, "rb") as f:
        assert other == stale and f.read(4) == b"\x7fELF"
    assert os.stat(first).st_mtime_ns == mtime


# ---- families.py and device_buffers.py: the table is the library's, and each checker catches what it is there to catch ------------------------
def test_family_table_agrees_with_the_library_spec():
    import modurl_gym_amd as mg
    for name, f in FAMILIES.items():
        s = mg.get_spec(f.kind)
        assert (s.obs_dim, s.n_actions, s.action_is_float, s.state_cols) == (f.D, f.n_actions, int(f.box is not None), f.state_cols), name
        assert (s.action_low, s.action_high) == (f.box or (0.0, 0.0)), name
        assert f.A == (1 if f.box else f.n_actions) and (f.f32_cols is None or f.f32_cols < f.state_cols), name


class HostArray:
    """host memory behind mg.DeviceArray's ptr, copy_from and numpy; the pointer is `skew` bytes past a 256-byte boundary (a device allocation: 0)"""
    skew = 0

    def __init__(self, shape, dtype):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.raw = np.zeros(n + 512, np.uint8)
        start = -self.raw.ctypes.data % 256 + self.skew
        self.a = self.raw[start: start + n].view(dtype).reshape(shape)
        self.ptr = self.raw.ctypes.data + start

    def copy_from(self, host):
        self.a[...] = np.ascontiguousarray(host, self.a.dtype).reshape(self.a.shape)

    def numpy(self):
        return self.a.copy()


@pytest.mark.parametrize("mis", [0, 1])
def test_guarded_sees_a_write_to_either_guard_and_to_the_payload(mis):
    words = 10
    for fill in (B.FILL, 0x7FC0BEEF):
        for at, held, same_bytes in ((None, True, True), (2 + mis, False, False), (4 + mis + words + 3, False, False), (4 + mis + 5, True, False)):
            g = B.Guarded(words, mis, fill=fill, alloc=HostArray)
            assert g.ptr % 16 == 4 * mis and (g.payload(words) == fill).all()
            if at is not None:
                g.dev.a[at] ^= 1
            assert g.guards_hold() == held and g.untouched() == same_bytes, (fill, at)
    g = B.Guarded(words, mis, np.arange(words, dtype=F), alloc=HostArray)
    assert same(g.payload(words, F), np.arange(words, dtype=F)) and g.guards_hold() and g.untouched()


@pytest.mark.parametrize("mis", [0, 1])
def test_final_buf_check_fails_on_each_kind_of_stray_write(mis):
    cap, D, n = 2, 3, 8
    rng = np.random.default_rng(5)
    finals = rng.normal(0, 1, (cap, D, n)).astype(F)
    finished = rng.random((cap, n)) < 0.4
    finished[0, 0], finished[1, 7], finished[0, 1] = True, True, False

    def written():
        fb = B.FinalBuf(cap, D, n, mis, alloc=HostArray)
        body = fb.dev.a[fb.off: fb.off + fb.words].reshape(cap, D, n)
        for t in range(cap):
            body[t][:, finished[t]] = finals[t][:, finished[t]].view(np.uint32)
        return fb, body

    fb, body = written()
    fb.check(finals, finished, "exact")
    body[0, 2, 1] = 0x3F800000            # an unfinished env-step
    with pytest.raises(AssertionError, match="1 words outside the finished env-steps were written"):
        fb.check(finals, finished, "stray")
    fb, body = written()
    body[1, 0, 7] ^= 1                    # a finished word, one bit off
    for eq in (same, same_words):
        with pytest.raises(AssertionError, match="1 of .* final words differ"):
            fb.check(finals, finished, "bit", eq)
    for at in (3 + mis, fb.off + fb.words):
        fb, _ = written()
        fb.dev.a[at] = 0
        with pytest.raises(AssertionError, match="a guard word was written"):
            fb.check(finals, finished, "guard")
    fb, body = written()                  # NaNs are equal as a class only where the caller says so
    body[0, 0, 0], finals.view(np.uint32)[0, 0, 0] = 0x7FC00001, 0x7FC00002
    fb.check(finals, finished, "nan class", same_words)
    with pytest.raises(AssertionError, match="final words differ"):
        fb.check(finals, finished, "nan bits")


def test_call_buffers_hand_out_the_alignment_asked_for_and_read_what_lies_there():
    for K, n, D, mis in ((1, 5, 3, 0), (3, 5, 3, 0), (1, 5, 3, (4, 4, 4, 1, 3)), (3, 5, 3, (4, 4, 4, 1, 3)), (3, 8, 2, 4)):
        b = B.CallBuffers(n, D, F, K, mis, alloc=HostArray)
        off = (0, 0, mis, 0, 0) if isinstance(mis, int) else mis
        assert [p % 16 for p in b.pointers()] == list(off)
        rng = np.random.default_rng(K + n)
        placed = []
        for a, o, shape, dt in zip(b.arr, off, b.shapes, b.dtypes):   # words put where the pointers point, by hand
            v = rng.integers(0, 256, int(np.prod(shape)) * dt.itemsize).astype(np.uint8)
            a.raw[:] = 0xEE
            a.a[o: o + v.size] = v
            placed.append(v.view(dt).reshape(shape))
        assert same(b.actions(), placed[0]) and all(same(g, e) for g, e in zip(b.read(), placed[1:]))
        acts = rng.normal(0, 1, (K, n)).astype(F)
        b.put_actions(acts)
        assert same(b.actions(), acts) and same(b.arr[0].a[off[0]: off[0] + acts.nbytes].view(F), acts.ravel())
        if K == 3:   # the slabs of step 2 start two steps' worth of bytes in
            assert [q - p for p, q in zip(b.pointers(), b.pointers(2))] == [8 * n, 8 * D * n, 8 * n, 2 * n, 2 * n]
    b = B.CallBuffers(5, 3, np.uint32, 2, 4, with_obs=False, alloc=HostArray)
    assert b.pointers()[1] is None and b.pointers(1)[1] is None and b.read()[0] is None and b.read()[1].shape == (2, 5)
    skewed = type("Skewed", (HostArray,), dict(skew=12))
    for mis in ((0, 0, 0, 4, 0), 0):   # 12 + 4: the done pointer comes out aligned after all; 12: nothing is aligned
        with pytest.raises(AssertionError, match="alignment"):
            B.CallBuffers(8, 2, F, mis=mis, alloc=skewed)
