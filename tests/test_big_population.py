"""tests/big_population.py on CPU tensors: the helpers of the addressing-bound tests fail when they should — a single wrong word, a word never written and a
one-column shift are each planted and must be caught — windows() holds every window it documents for every family's shape, and the device footprints
test_gpu_addressing_bounds.py declares are those of its shapes."""
import pytest
import torch

import big_population as bp
from big_population import P

PERIOD = 64                     # the helpers at a small period: the same code, a population of a few thousand
N = 37 * PERIOD + 20            # ragged: the period does not divide it


def clean(rows=3, n=N, dtype=torch.float32):
    g = torch.Generator().manual_seed(5)
    base = torch.rand((rows, PERIOD), generator=g) if dtype == torch.float32 else torch.randint(0, 2, (rows, PERIOD), generator=g).to(dtype)
    return bp.tile_last(base, n)


def test_tile_last_and_periodic_actions():
    base = torch.arange(2 * PERIOD, dtype=torch.int32).view(2, PERIOD)
    t = bp.tile_last(base, N)
    assert t.shape == (2, N) and all(torch.equal(t[:, i], base[:, i % PERIOD]) for i in (0, 1, PERIOD - 1, PERIOD, 5 * PERIOD + 3, N - 1))
    a = bp.periodic_actions(9, N, PERIOD, n_actions=3, seed=1)
    assert a.dtype == torch.int32 and a.shape == (9, N) and int(a.min()) == 0 and int(a.max()) == 2
    assert torch.equal(a[:, PERIOD: 2 * PERIOD], a[:, :PERIOD]) and torch.equal(a[:, 37 * PERIOD:], a[:, :20])
    assert len({bytes(r.numpy().tobytes()) for r in a[:, :PERIOD]}) == 9 and all(len(set(r.tolist())) > 1 for r in a[:, :PERIOD])   # differs between steps and residues
    b = bp.periodic_actions(4, N, PERIOD, box=(-2.5, 2.5), seed=1)
    assert b.dtype == torch.float32 and float(b.min()) >= -2.5 and float(b.max()) <= 2.5 and float(b.min()) < -1 and float(b.max()) > 1
    assert torch.equal(b[:, -20:], b[:, :20])
    assert torch.equal(bp.periodic_actions(4, N, PERIOD, box=(-1, 1), seed=2), bp.periodic_actions(4, N, PERIOD, box=(-1, 1), seed=2))
    m = bp.periodic_bytes(1, N, 0.3, PERIOD, seed=2, lead=False)
    assert m.shape == (N,) and m.dtype == torch.uint8 and 0 < int(m[:PERIOD].sum()) < PERIOD and torch.equal(m[PERIOD: 2 * PERIOD], m[:PERIOD])


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8, torch.int32])
def test_assert_periodic_accepts_the_clean_and_catches_each_planted_defect(dtype, monkeypatch):
    x = clean(dtype=dtype)
    bp.assert_periodic(x, PERIOD, "clean")
    bp.assert_periodic(x[0], PERIOD, "one row")
    monkeypatch.setattr(bp, "CHUNK", 5 * PERIOD)   # several chunks, the last ragged
    bp.assert_periodic(x, PERIOD, "clean in chunks")
    for where in ((1, 9 * PERIOD + 5), (2, N - 1), (0, PERIOD)):   # a full period, the ragged remainder, the first word behind the head
        y = x.clone()
        w = bp.words(y)
        w[where] = w[where] ^ 1   # one bit of one word
        with pytest.raises(AssertionError, match=rf"1 words differ.*row {where[0]}, environment {where[1]} "):
            bp.assert_periodic(y, PERIOD, "wrong word")
    y = x.clone()
    bp.fill_sentinel(y[1, 700:701])   # a word the kernel never wrote, behind the head ...
    with pytest.raises(AssertionError, match="environment 700 "):
        bp.assert_periodic(y, PERIOD, "unwritten")
    y = x.clone()
    bp.fill_sentinel(y[:, 3:4])       # ... and inside it: every copy agrees with it, so periodicity alone would pass
    bp.fill_sentinel(y[:, 3 + PERIOD:: PERIOD])
    with pytest.raises(AssertionError, match="never written"):
        bp.assert_periodic(y, PERIOD, "unwritten head")
    bp.assert_periodic(y, PERIOD, "sparse output", written=False)
    y = x.clone()
    y[:, 10 * PERIOD:] = x[:, 10 * PERIOD - 1: -1]   # everything from there on one column late
    with pytest.raises(AssertionError, match=rf"environment {10 * PERIOD} "):
        bp.assert_periodic(y, PERIOD, "shift")


def test_words_are_compared_not_values():
    x = clean()
    y = x.clone()
    x[:, PERIOD + 7:: PERIOD] = 0.0
    x[:, 7] = -0.0
    with pytest.raises(AssertionError, match="words differ"):   # -0.0 == 0.0 as values
        bp.assert_periodic(x, PERIOD, "signed zero")
    y[:, 5:: PERIOD] = float("nan")
    bp.assert_periodic(y, PERIOD, "equal NaN words")               # NaN != NaN as values
    assert bp.same_words(y, y.clone()) and not bp.same_words(torch.zeros(4), -torch.zeros(4)) and not bp.same_words(torch.zeros(4), torch.zeros(5))
    z = torch.zeros((3, 8))[:, :6]
    assert bp.same_words(z, torch.zeros((3, 6))) and not bp.same_words(z, torch.ones((3, 6)))   # a view with a row stride
    assert bp.count_set(torch.tensor([0, 1, 0, 7], dtype=torch.uint8), torch.tensor([0, 0, 1, 1], dtype=torch.uint8)) == 3


def small_handles(big, wins):
    """the outputs of handles that compute the right words: the slices themselves, copied"""
    return lambda k, a, b: {name: x[..., a:b].clone() for name, x in big.items()}


def test_assert_windows_equal_accepts_the_clean_and_catches_each_planted_defect():
    n = 1 << 16
    wins = bp.windows(n, 3, columns=5, period=PERIOD)
    big = dict(obs=clean(4, n), reward=clean(1, n)[0], done=clean(1, n, torch.uint8)[0])
    ref = small_handles({k: v.clone() for k, v in big.items()}, wins)
    bp.assert_windows_equal(big, ref, wins, "clean")
    a, b = wins[4]
    inside, outside = a + 11, next(i for i in range(n) if not any(x <= i < y for x, y in wins))
    y = dict(big, obs=big["obs"].clone())
    bp.words(y["obs"])[2, inside] ^= 1 << 31
    with pytest.raises(AssertionError, match=rf"obs window \[{a}, {b}\): 1 words differ.*environment {inside}:"):
        bp.assert_windows_equal(y, ref, wins, "wrong word")
    y = dict(big, reward=big["reward"].clone())
    bp.fill_sentinel(y["reward"][inside: inside + 1])
    with pytest.raises(AssertionError, match=rf"reward window .*environment {inside}: 0xffffffff against"):
        bp.assert_windows_equal(y, ref, wins, "unwritten")
    y = dict(big, done=big["done"].clone())
    y["done"][a + 1: b] = big["done"][a: b - 1]
    y["done"][a] = 1 - big["done"][a]
    with pytest.raises(AssertionError, match=rf"done window \[{a}, {b}\)"):
        bp.assert_windows_equal(y, ref, wins, "shift")
    y = dict(big, obs=big["obs"].clone())
    bp.words(y["obs"])[0, outside] ^= 1   # outside every window: not this helper's to see (assert_periodic covers the whole population)
    bp.assert_windows_equal(y, ref, wins, "outside")
    with pytest.raises(AssertionError):   # the small handle must deliver every output
        bp.assert_windows_equal(big, lambda k, a, b: {"obs": big["obs"][..., a:b]}, wins, "missing")


def shapes():
    import test_gpu_addressing_bounds as T
    for fam, n in T.STEP_CASES:
        yield fam, n, (n + 1023) // 1024 * 1024, bp.FAMILIES[fam].engine_cols, 0
    yield "lunar_lander", T.LL_N, T.LL_N, 1, T.LL_RECORD_BYTES


def test_windows_hold_every_required_window():
    crossings = 0
    for fam, n, n_pad, columns, record_bytes in shapes():
        wins = bp.windows(n, 17, n_pad, columns, record_bytes)
        assert wins == bp.windows(n, 17, n_pad, columns, record_bytes) and len(set(wins)) == len(wins)
        assert all(0 <= a < b <= n and b - a <= P and a % 4 == 0 for a, b in wins), (fam, n)
        assert wins[0] == (0, P)
        assert any(b == n and a == (n - 1) // P * P for a, b in wins), "the last window, ragged when P does not divide n"
        assert any(a < n // 2 - 1 and n // 2 + 1 < b for a, b in wins), "the window that straddles n / 2"
        for c in range(columns):   # every environment at which a 32-bit byte offset 4 (c n_pad + i) crosses 2^31 has both sides in one window
            i = (1 << 29) - c * n_pad
            if 0 < i < n:
                crossings += 1
                assert 4 * (c * n_pad + i - 1) < 1 << 31 <= 4 * (c * n_pad + i)
                assert any(a <= i - 1 and i < b for a, b in wins), (fam, n, c, i)
        assert bp.crossing_indices(n, n_pad, columns) == [(1 << 29) - c * n_pad for c in range(columns) if 0 <= (1 << 29) - c * n_pad < n]
        for edge in ((1 << 31, 1 << 32) if record_bytes else ()):
            i = edge // record_bytes
            assert any(a <= i - 1 and i + 1 < b for a, b in wins), (fam, edge)
        seeded = [w for w in wins if w not in bp.windows(n, 18, n_pad, columns, record_bytes)]
        assert len(seeded) >= bp.N_SEEDED - 1, "the seeded windows move with the seed"
    assert crossings == 2   # Pendulum at 2^27 + 4 and Acrobot at 2^26 + 4 (n_pad rounds up: a column starts short of 2^31), MountainCar has too few columns
    # at the bounds themselves every column starts on a multiple of 2^29 words, so the 2^31 edge falls between two columns: CartPole's counter column
    # starts exactly there, and window 0 holds its first word
    assert bp.crossing_indices(1 << 27, 1 << 27, 5) == [0] and bp.crossing_indices(1 << 26, 1 << 26, 9) == [0]


def test_declared_footprints_are_those_of_the_shapes():
    import test_gpu_addressing_bounds as T
    assert len(T.FOOTPRINT) == 2 * len(T.STEP_CASES) + len(T.CP_BOUND_CASES) + 2 + len(T.ROLL_CASES) + 3
    for key, gib in T.FOOTPRINT.items():
        need = T.footprint(key) / bp.GIB
        assert gib - 0.1 < need <= gib + 1e-9, (key, gib, need)   # declared to the next tenth of a GiB
        assert gib * bp.GIB <= bp.MEMORY_CAP, key
    n = 1 << 27
    assert bp.engine_bytes("cartpole", n) == 5 * 4 * n and bp.engine_bytes("pendulum", n + 4) == (5 * 4 + 2) * (n + 1024)
    assert bp.need_bytes([("cartpole", n)], [(4, 6, n), (1, n)]) == bp.SCRATCH + 20 * n + 24 * n + n
    with pytest.raises(AssertionError):
        bp.require_memory(bp.MEMORY_CAP + 1)
