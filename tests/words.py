"""Word comparison, in its two meanings.  same_words: float32 bit patterns, NaNs equal as a class (a restatement against a header, where the NaN's payload
is nobody's contract).  same: exact words, whatever the dtype (one build of the engine against another, or against itself).  No test here."""
import numpy as np

F = np.float32


def words_of(a):
    """the uint32 words of a float32 array (anything else is converted to float32 first)"""
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_words(got, exp):
    """equal bit patterns; NaNs are equal as a class.  Arrays of uint32 are taken as the words of float32 values"""
    g, e = (v.view(F) if v.dtype == np.uint32 else np.ascontiguousarray(v, F) for v in (np.ascontiguousarray(got), np.ascontiguousarray(exp)))
    return bool(np.all((g.view(np.uint32) == e.view(np.uint32)) | (np.isnan(g) & np.isnan(e))))


def bits(a):
    """float32 as its words, every other dtype as it is"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    """exact: equal shapes and equal words; two different NaN words differ, and so do +0 and -0"""
    return np.array_equal(bits(a), bits(b))
