"""Support for the tests that run the kernels at the bounds of their 32-bit addressing (test_gpu_addressing_bounds.py): populations of up to 2^27
environments and buffers beyond 4 GiB, checked without the population ever leaving the device.  Torch is plumbing (memory and elementwise compares); every
helper takes CPU tensors as well, which is how test_big_population.py checks that the helpers fail when they should.  No test here.

Two references, neither a new one:
  * periodicity.  From reset_deterministic() with auto-reset off, an environment's step is a function of its state and action alone, so under an action
    table whose column i equals column i mod P every output column i equals column i mod P.  assert_periodic checks that over the whole population on the
    device; the first P columns are compared with a P-environment handle, whose path the rest of the suite pins to the oracle and the float64 references.
  * windows.  Sharding is invisible: a handle of b - a environments with env_id_base + a gives the words of environments a .. b - 1 of the big handle.
    assert_windows_equal compares P-wide slices, the only data that travels to the host.

Every comparison is one of words: float32 tensors are viewed as int32, so NaNs, signed zeros and the sentinel are compared as bit patterns."""
import numpy as np
import pytest
import torch

from families import FAMILIES

P = 4096                 # the period of the action tables and the width of a window
SENTINEL_BYTE = 0xFF     # outputs are prefilled with 0xFF bytes: the word 0xFFFFFFFF (a NaN no kernel here produces), the flag byte 0xFF (flags are 0 / 1)
GIB = 1 << 30
MEMORY_CAP = 40 * GIB    # no test may need more
SCRATCH = 2 * GIB        # what the compares below leave in torch's cache at most (they work through the big tensors in pieces of at most CHUNK elements)
CHUNK = 1 << 27
N_SEEDED = 6


# ---- words ----------------------------------------------------------------------------------------------------------------------------------
def words(x):
    """4-byte dtypes as int32 words, byte dtypes as they are"""
    if x.dtype in (torch.float32, torch.uint32):
        return x.view(torch.int32)
    if x.dtype == torch.bool:
        return x.view(torch.uint8)
    assert x.dtype in (torch.int32, torch.uint8), x.dtype
    return x


def sentinel(shape, dtype, device):
    """a tensor of the given shape whose every byte is SENTINEL_BYTE"""
    x = torch.empty(shape, dtype=dtype, device=device)
    fill_sentinel(x)
    return x


def fill_sentinel(*tensors):
    for x in tensors:
        words(x).fill_(-1 if x.element_size() == 4 else SENTINEL_BYTE)


def has_sentinel(x):
    """whether any element of x is the sentinel word (byte for byte dtypes)"""
    w = words(x).reshape(-1)
    s = -1 if w.element_size() == 4 else SENTINEL_BYTE
    return any(bool((w[a: a + CHUNK] == s).any()) for a in range(0, w.numel(), CHUNK))


# ---- periodic inputs ------------------------------------------------------------------------------------------------------------------------
def tile_last(base, n):
    """base [.., p] -> [.., n] with column i = column i mod p, built on base's device without an intermediate larger than the result"""
    p = base.shape[-1]
    out = torch.empty(base.shape[:-1] + (n,), dtype=base.dtype, device=base.device)
    full = n // p * p
    if full:
        out[..., :full].unflatten(-1, (n // p, p)).copy_(base.unsqueeze(-2))
    if n > full:
        out[..., full:] = base[..., : n - full]
    return out


def periodic_actions(K, n, period=P, n_actions=None, box=None, seed=0, device="cpu"):
    """A [K][n] action table whose column i equals column i mod period: int32 in [0, n_actions), or float32 uniform in box = (lo, hi).  The K x period base
    is seeded on the host; the table itself is built on `device`.  The base is redrawn until no two steps are equal rows and no row is constant, so the
    table differs between residues and between steps."""
    assert (n_actions is None) != (box is None)
    rng = np.random.default_rng(seed)
    while True:
        if box is None:
            base = rng.integers(0, n_actions, (K, period)).astype(np.int32)
        else:
            base = rng.uniform(box[0], box[1], (K, period)).astype(np.float32)
        rows = {r.tobytes() for r in base}
        if len(rows) == K and all((r != r[0]).any() for r in base):
            break
    return tile_last(torch.from_numpy(base).to(device), n)


def periodic_bytes(K, n, rate, period=P, seed=0, device="cpu", lead=True):
    """uint8 [K][n] (or [n] with lead = False and K = 1) of 0 / 1 at `rate`, column i = column i mod period"""
    rng = np.random.default_rng(seed)
    base = (rng.random((K, period)) < rate).astype(np.uint8)
    t = tile_last(torch.from_numpy(base).to(device), n)
    return t if lead else t[0]


# ---- the two assertions ---------------------------------------------------------------------------------------------------------------------
def same_words(a, b):
    """equal shapes and equal words, compared in pieces of at most CHUNK elements"""
    if a.shape != b.shape:
        return False
    a, b = words(a), words(b)
    if a.is_contiguous() and b.is_contiguous():
        a, b = a.reshape(-1), b.reshape(-1)
        return all(torch.equal(a[i: i + CHUNK], b[i: i + CHUNK]) for i in range(0, a.numel(), CHUNK))
    if a.dim() <= 1:
        return torch.equal(a, b)
    return all(same_words(x, y) for x, y in zip(a, b))


def count_set(done, trunc):
    """how many elements have done | truncated set, counted in pieces of at most CHUNK elements"""
    d, u = done.reshape(-1), trunc.reshape(-1)
    return sum(int(((d[i: i + CHUNK] != 0) | (u[i: i + CHUNK] != 0)).sum()) for i in range(0, d.numel(), CHUNK))


def assert_periodic(x, period=P, name="x", written=True):
    """The last axis of x equals its first `period` entries tiled (a ragged remainder included), word for word, and (written) no word is the sentinel the
    caller prefilled the output with; written = False is for outputs the call writes in places only, whose first `period` entries the caller compares with
    a reference that holds the sentinel elsewhere.  Reports the first differing (row, index) and the number of differing words."""
    w = words(x)
    n = w.shape[-1]
    w = w.reshape(-1, n)
    head = w[:, :period]
    assert not written or not has_sentinel(head), f"{name}: a word of the first {period} environments was never written"
    step = max(period, CHUNK // max(w.shape[0], 1) // period * period)
    bad, first = 0, None
    for a in range(0, n, step):
        blk = w[:, a: a + step]
        m = blk.shape[1]
        full = m // period * period
        ne = torch.zeros(blk.shape, dtype=torch.bool, device=w.device)
        if full:
            ne[:, :full] = (blk[:, :full].unflatten(1, (m // period, period)) != head.unsqueeze(1)).flatten(1)
        if m > full:
            ne[:, full:] = blk[:, full:] != head[:, : m - full]
        c = int(ne.sum())
        if c and first is None:
            r, i = (int(v) for v in ne.nonzero()[0])
            first = (r, a + i)
        bad += c
    assert bad == 0, (f"{name}: {bad} words differ from the first {period} environments tiled; the first at row {first[0]}, environment {first[1]} "
                      f"(= {first[1] % period} mod {period}): {int(w[first[0], first[1]]) & 0xFFFFFFFF:#x} against {int(w[first[0], first[1] % period]) & 0xFFFFFFFF:#x}")


def windows(n, seed, n_pad=None, columns=1, record_bytes=0, period=P):
    """The index windows [a, b) of a population of n, each at most `period` wide and starting at a multiple of 4 (a lane's four environments stay together):
      1. the first, [0, period);
      2. the last, [floor((n - 1) / period) * period, n): ragged when period does not divide n;
      3. the one centred on n / 2 (with env_id_base = 2^32 - n / 2 it straddles global id 2^32 as well);
      4. for every column c < columns of an engine whose columns lie n_pad words apart, the one centred on the environment i at which the column's byte
         offset 4 (c n_pad + i) reaches 2^31, where 0 <= i < n (a column that starts at or beyond 2^31 has no such i: window 1 is its first word);
      5. for an engine of records (record_bytes > 0: LunarLander), the ones centred on the records whose byte offset reaches 2^31 and 2^32;
      6. N_SEEDED windows at seeded starts.
    Duplicates are dropped; the order is the one above."""
    n_pad = (n + 1023) // 1024 * 1024 if n_pad is None else n_pad

    def centred(i):
        a = max(0, min(i - period // 2, n - period)) // 4 * 4
        return (a, min(a + period, n))

    out = [(0, min(period, n)), ((n - 1) // period * period, n), centred(n // 2)]
    for c in range(columns):
        i, r = divmod((1 << 31) - 4 * c * n_pad, 4)
        if r == 0 and 0 <= i < n:
            out.append(centred(i))
    if record_bytes:
        for edge in (1 << 31, 1 << 32):
            i = edge // record_bytes   # the record that holds byte `edge`
            if 0 < i < n:
                out.append(centred(i))
    rng = np.random.default_rng(seed)
    for _ in range(N_SEEDED):
        a = int(rng.integers(0, max(n - period, 0) // 4 + 1)) * 4
        out.append((a, min(a + period, n)))
    seen, uniq = set(), []
    for w in out:
        if w not in seen:
            seen.add(w)
            uniq.append(w)
    return uniq


def crossing_indices(n, n_pad, columns):
    """the environments of windows() rule 4 (what test_big_population.py checks the windows against)"""
    return [((1 << 31) - 4 * c * n_pad) // 4 for c in range(columns) if 0 <= (1 << 31) - 4 * c * n_pad < 4 * n]


def assert_windows_equal(big_outputs, make_small, wins, what=""):
    """big_outputs: {name: tensor whose last axis is the environment}; make_small(k, a, b) -> {name: tensor with last axis b - a}, the outputs of the
    (b - a)-environment handle of window k (same seed, env_id_base + a, driven by the same action slices).  Every slice big[.., a:b] must equal the small
    handle's tensor word for word; only the slices travel to the host."""
    for k, (a, b) in enumerate(wins):
        small = make_small(k, a, b)
        assert set(small) == set(big_outputs), (sorted(small), sorted(big_outputs))
        for name, big in big_outputs.items():
            g = words(big)[..., a:b].cpu().contiguous()
            e = words(small[name]).cpu().contiguous()
            assert g.shape == e.shape, f"{what} {name} window [{a}, {b}): shapes {tuple(g.shape)} and {tuple(e.shape)}"
            ne = g != e
            if bool(ne.any()):
                idx = [int(v) for v in ne.nonzero()[0]]
                got, exp = int(g[tuple(idx)]) & 0xFFFFFFFF, int(e[tuple(idx)]) & 0xFFFFFFFF
                raise AssertionError(f"{what} {name} window [{a}, {b}): {int(ne.sum())} words differ from the {b - a}-environment handle; the first at "
                                     f"{idx[:-1]} environment {a + idx[-1]}: {got:#x} against {exp:#x}")


# ---- memory ---------------------------------------------------------------------------------------------------------------------------------
LL_BYTES_PER_ENV = 2 * (1152 + 32) + 4 + 16 * 4 + 1   # records and observation (and their reset shadows), next action, 16 work lists, class byte
LL_BYTES_PER_HANDLE = 563 << 20   # whatever the population: the far-constraint slices of the contact kernels' bounded grids (measured: 0.52 GiB a handle)


def engine_bytes(family, n):
    """what mgym_create allocates per handle of n environments, to the leading term"""
    n_pad = (max(n, 1) + 1023) // 1024 * 1024
    if family == "lunar_lander":
        return LL_BYTES_PER_ENV * n_pad + LL_BYTES_PER_HANDLE
    return FAMILIES[family].engine_cols * 4 * n_pad + (0 if family == "cartpole" else 2 * n_pad)   # + the u16 elapsed column


def need_bytes(handles=(), buffers=()):
    """Peak device footprint of a test: handles = [(family, n), ..] alive at the same time, buffers = [(itemsize, dim, ..), ..] the caller's tensors alive
    at the same time, plus SCRATCH for the compares."""
    total = SCRATCH + sum(engine_bytes(f, n) for f, n in handles)
    for itemsize, *dims in buffers:
        total += itemsize * int(np.prod(dims, dtype=np.int64))
    return int(total)


def require_memory(nbytes):
    """Skips only when the device shows less free memory than the need plus 10 %; a need beyond MEMORY_CAP is a mistake in the test."""
    assert nbytes <= MEMORY_CAP, f"a test may need at most {MEMORY_CAP >> 30} GiB, this one declares {nbytes / GIB:.1f}"
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes * 1.1:
        pytest.skip(f"needs {nbytes * 1.1 / GIB:.1f} GiB of free device memory, {free / GIB:.1f} are free")
