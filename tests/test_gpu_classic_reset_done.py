"""mgym_reset_done on MountainCar(+Continuous), Pendulum and Acrobot: the two-mask gather of their reset kernels (reset_mask4, soa4.h) against the
one-mask reset of a twin handle, and the shared elapsed-count kernels (classic_env.hip) with a count above 65535.

n = 1027 is two tiles of lane groups with a ragged last group of three: the smallest population in which the aligned-word branch, the byte branch
and the `i < n` guard of the gather all run."""
import numpy as np
import pytest

import modurl_gym_amd as mg
from families import CLASSIC, KIND

pytestmark = pytest.mark.gpu

N = 1027
NAMES = [name for name in CLASSIC if name != "cartpole"]


def masks(seed):
    """done and trunc bytes, about a quarter set in each (any nonzero byte counts), some envs in both, the last group's three covered"""
    rng = np.random.default_rng(seed)
    done = np.where(rng.random(N) < 0.25, rng.integers(1, 256, N), 0).astype(np.uint8)
    trunc = np.where(rng.random(N) < 0.25, rng.integers(1, 256, N), 0).astype(np.uint8)
    done[[5, N - 2]] = 1
    trunc[[5, N - 1]] = 128
    done[N - 3] = trunc[N - 3] = 0
    assert 0 < np.count_nonzero(done & trunc) and 0 < np.count_nonzero(done) < N // 2 and 0 < np.count_nonzero(trunc) < N // 2
    return done, trunc


@pytest.mark.parametrize("unaligned", [False, True], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("name", NAMES)
def test_reset_done_two_masks_equal_one_mask_reset(name, unaligned):
    a, b = (mg.VecEnv(KIND[name], N, seed=41) for _ in range(2))
    done, trunc = masks(7)
    mask = ((done | trunc) != 0).astype(np.uint8)
    el = np.random.default_rng(8).integers(1, 70000, N).astype(np.uint32)
    el[[0, N - 1, N - 3]] = 70000   # above the 16-bit counter: stored as 65535
    for env in (a, b):
        env.reset()
        env.set_elapsed_steps(el)
    before = a.get_state().view(np.uint32).copy()
    if unaligned:
        import torch
        hold = torch.zeros(2, N + 1, dtype=torch.uint8, device="cuda:0")
        hold[0, 1:] = torch.from_numpy(done).to(hold.device)
        hold[1, 1:] = torch.from_numpy(trunc).to(hold.device)
        torch.cuda.synchronize()
        d_done, d_trunc = hold[0].data_ptr() + 1, hold[1].data_ptr() + 1   # one byte into each row: not 4-byte aligned
        assert d_done % 4 == 1 and d_trunc % 4 == 1
    else:
        d_done, d_trunc = mg.DeviceArray.from_numpy(done), mg.DeviceArray.from_numpy(trunc)
        assert d_done.ptr % 4 == 0 and d_trunc.ptr % 4 == 0
    a.reset_done_device(d_done, d_trunc)
    a.sync()
    b.reset(mask)
    sa, sb = a.get_state().view(np.uint32), b.get_state().view(np.uint32)
    assert np.array_equal(sa, sb)
    changed = (sa != before).any(axis=0)   # the episode column moves with every reset
    assert np.array_equal(changed, mask.astype(bool))
    ea, eb = a.elapsed_steps(), b.elapsed_steps()
    assert np.array_equal(ea, eb)
    assert np.array_equal(ea, np.where(mask.astype(bool), 0, np.minimum(el, 65535)).astype(np.uint32))
