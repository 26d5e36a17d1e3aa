"""The CPU oracle's LunarLander contact steps against the float64 rules of tests/ll_contact_ref.py (no GPU): 608 environments,
landings, crashes, bounces and exits, checked up to each first ending.  The populations, the action tables and the coverage they
must reach are in tests/ll_contact_cases.py; tests/test_gpu_ll_contact.py holds the kernels to the same rules."""
import numpy as np
import pytest

import ll_contact_cases as C
import ll_contact_ref as R
from oracle import oracle as ora


def test_reference_terrain_of_the_deterministic_reset():
    # lunar_lander.rs:1276-1280, :766-774 by hand: heights H / 8, the helipad's five chunks at H / 4, saturating smoothing
    cx, sy = R.terrain(R.deterministic_heights(1))
    h8, h4 = 400.0 / 30.0 / 8.0, 400.0 / 30.0 / 4.0
    assert np.allclose(cx, 2.0 * np.arange(11), atol=1e-6)
    expect = [0.33 * 3 * h8] * 2 + [0.33 * (2 * h8 + h4), 0.33 * (h8 + 2 * h4)] + [0.33 * 3 * h4] * 3 + [0.33 * (h8 + 2 * h4), 0.33 * (2 * h8 + h4)] + [0.33 * 3 * h8] * 2
    assert np.allclose(sy[0], expect, atol=1e-6)


def test_reference_philox_is_the_published_one():
    # Random123's known-answer vectors for philox4x32-10 (kat_vectors): zeros, and pi digits under the all-ones pattern
    assert [int(v[0]) for v in R.philox4x32_10([0], [0], [0], [0], 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    got = R.philox4x32_10([0x243f6a88], [0x85a308d3], [0x13198a2e], [0x03707344], 0xa4093822, 0x299f31d0)
    assert [int(v[0]) for v in got] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    assert np.array_equal(np.array([v[0] for v in got], np.uint32), np.array(ora.philox([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]), np.uint32))


def test_coverage_of_the_populations_and_share_of_declined_steps():
    counts, share = C.coverage()
    print("coverage:", counts, "declined:", {k: f"{v:.2%}" for k, v in share.items()})


@pytest.mark.parametrize("pop", list(C.POPULATIONS))
def test_oracle_contact_steps_obey_the_float64_rules(pop):
    traj = C.build(pop)
    viol, band, fig = C.oracle_rules(pop)
    print(pop, "worst reward error", fig["reward_err"].max(), "of", R.BOUND_REWARD, "lowest vertex", fig["low_pre"].min(), "bound", -R.BOUND_SINK,
          "judged", {k: int(v.sum()) for k, v in fig["judged"].items()})
    lines = C.report(pop, traj, viol, band, fig)
    assert not lines, "\n".join(lines)


def test_terrain_of_the_seeded_reset_is_the_documented_draw():
    """The oracle's own terrain is not exported; what is: a lander that free-falls onto it crashes ON it (R4) and nothing sinks
    into it (R8), which test_oracle_contact_steps_obey_the_float64_rules holds for 320 seeded terrains.  Here the draw itself:
    the reference's heights from the documented counter layout must differ between neighbours, episodes and seeds, stay inside
    [0, H / 2) and equal the oracle's uniform of the oracle's Philox words."""
    g = C.ENV_ID_BASE + np.arange(64)
    a = R.seeded_heights(C.SEED, g, np.zeros(64, int))
    assert a.shape == (12, 64) and (a >= 0).all() and (a < float(R.H) / 2).all()
    w = [ora.philox([int(g[5]) & 0xFFFFFFFF, int(g[5]) >> 32, 0, slot], [C.SEED & 0xFFFFFFFF, C.SEED >> 32]) for slot in range(3)]
    u = np.array([ora.lib().ora_u23(int(x)) for x in sum(w, [])], np.float32)
    assert np.array_equal(a[:, 5], u * (R.H / np.float32(2.0)))
    assert not np.array_equal(a, R.seeded_heights(C.SEED, g, np.ones(64, int))) and not np.array_equal(a, R.seeded_heights(C.SEED + 1, g, np.zeros(64, int)))
    assert not np.array_equal(a[:, 1:], a[:, :-1])
