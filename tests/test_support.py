"""The support layer the other tests stand on: philox_ref's Philox against the published vectors, the two meanings of word equality in words.py,
glibc_f32.fmaf's single rounding and broadcasting, and native_build's one compilation per process.  No GPU."""
import os

import numpy as np

import glibc_f32
import native_build
import philox_ref
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
