"""Philox4x32-10 on numpy arrays and the two ways include/mgym.h keys it: per environment and episode (the reset draws) and per block of four consecutive
global environment ids (the policies' draws).  tests/ll_contact_ref.py keeps a Philox of its own on purpose.  No test here."""
import numpy as np

F = np.float32
M32 = np.uint64(0xFFFFFFFF)
# the fourth counter word of the policies' draws, from the text of include/mgym.h: mgym_rollout_uniform, mgym_rollout_mlp_sample, mgym_rollout_mlp_gauss
SLOT_POLICY, SLOT_POLICY_SAMPLE, SLOT_POLICY_GAUSS = 0x40000000, 0x50000000, 0x60000000


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over arrays of counters -> the four output words (uint32 arrays)"""
    c0, c1, c2, c3 = (np.asarray(v, np.uint64) & M32 for v in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & M32, p1 >> np.uint64(32), p1 & M32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return [v.astype(np.uint32) for v in (c0, c1, c2, c3)]


def _keyed(seed, gid, c2, c3):
    gid = np.asarray(gid, np.uint64)
    return philox4x32_10(gid & M32, gid >> np.uint64(32), np.asarray(c2, np.uint64), np.uint64(c3), int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)


def env_draw(seed, gid, episode, slot=0):
    """the four words of env gid's draw number `slot` for its episode number `episode`"""
    return _keyed(seed, gid, episode, slot)


def block_words(seed, call, g, slot):
    """the four words of the block of four consecutive ids that holds env g, at counter word `slot` (a slot base + f(t)) of call number `call`"""
    return _keyed(seed, np.asarray(g, np.uint64) & ~np.uint64(3), call, slot)


def own_word(seed, call, g, slot):
    """word g % 4 of env g's block"""
    g = np.asarray(g, np.uint64)
    return np.choose((g & np.uint64(3)).astype(np.intp), block_words(seed, call, g, slot))


def u53(hi, lo):
    m = ((hi.astype(np.uint64) >> np.uint64(5)) << np.uint64(26)) | (lo.astype(np.uint64) >> np.uint64(6))
    return m.astype(np.float64) * (1.0 / 9007199254740992.0)


def uniform_f64_to_f32(lo, hi, w_hi, w_lo):
    return (u53(w_hi, w_lo) * (hi - lo) + lo).astype(F)
