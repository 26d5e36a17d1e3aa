"""The engine's LunarLander contact steps against the float64 rules of tests/ll_contact_ref.py: the action tables of
tests/ll_contact_cases.py through mgym_step on handles without auto-reset, the state read before and after every step, in the
three launch forms tests/test_gpu_lunar.py reaches (default, MGYM_LL_GENERAL_ONLY=1, MGYM_LL_GENERAL_BLOCK=64).  The rules run on
the engine's OWN blobs and outputs with the bounds measured on the oracle, unchanged; every word must also equal the oracle's,
which is cheap and says on which side a failure is.  One further run steps an auto-reset handle over the seeded population until
every environment is in its second episode: the only place where the terrain of a later episode, and of a staged reset, is
checked.  (mgym_rollout is left out: mgym_rollout == K x mgym_step is tested elsewhere.)"""
import numpy as np
import pytest

import ll_contact_cases as C
import ll_contact_ref as R
import modurl_gym_amd as mg

pytestmark = pytest.mark.gpu

FORMS = {"default": {}, "general_only": {"MGYM_LL_GENERAL_ONLY": "1"}, "block64": {"MGYM_LL_GENERAL_BLOCK": "64"}}


def words(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def handle(pop, form, monkeypatch, **kw):
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    env = mg.VecEnv(mg.LUNARLANDER, C.POPULATIONS[pop]["n"], **C.handle_args(pop), **kw)
    for k in FORMS[form]:
        monkeypatch.delenv(k)
    info = env.info()
    assert form != "block64" or info["contact_block"] == "64", info
    return env


@pytest.mark.parametrize("pop", list(C.POPULATIONS))
@pytest.mark.parametrize("form", list(FORMS))
def test_engine_contact_steps_obey_the_float64_rules(form, pop, monkeypatch):
    exp = C.build(pop)
    env = handle(pop, form, monkeypatch)
    C.start(pop, env)
    got = dict(actions=exp["actions"], blobs=[np.array(env.get_state())], obs=[], reward=[], done=[], trunc=[])
    for t in range(C.T):
        o, r, d, tr = (np.array(v) for v in env.step(exp["actions"][t]))
        got["obs"].append(o), got["reward"].append(r), got["done"].append(d), got["trunc"].append(tr)
        got["blobs"].append(np.array(env.get_state()))
    env.close()
    traj = {k: np.array(v) for k, v in got.items()}
    done = traj["done"].astype(int)
    traj["alive"] = np.cumsum(done, 0) - done == 0
    viol, band, fig = C.run_rules(pop, traj)
    print(form, pop, "worst reward error", fig["reward_err"].max(), "of", R.BOUND_REWARD, "lowest vertex", fig["low_pre"].min())
    lines = C.report(pop, traj, viol, band, fig)
    for rule in viol:                                                 # the engine's words next to the oracle's, where a rule is broken
        inside = ~traj["alive"] if rule.startswith("after") else traj["alive"]
        for t, i in np.argwhere(viol[rule] & ~band[rule] & inside)[:3]:
            lines.append(f"  {rule} step {t} env {i}: engine reward {traj['reward'][t, i]!r} obs {traj['obs'][t, :, i].tolist()} flags / shaping {traj['blobs'][t + 1][18:23, i].tolist()}"
                         f" | oracle reward {exp['reward'][t, i]!r} obs {exp['obs'][t, :, i].tolist()} flags / shaping {exp['blobs'][t + 1][18:23, i].tolist()}")
    assert not lines, "\n".join(lines)
    assert np.array_equal(traj["alive"], exp["alive"]), f"{form} {pop}: the episodes end elsewhere than the oracle's, first at {np.argwhere(traj['alive'] != exp['alive'])[:3].tolist()}"
    al = exp["alive"]
    for name in ("obs", "reward", "done", "trunc"):
        g, e = words(traj[name]), words(exp[name])
        bad = (g != e) & (al[:, None, :] if g.ndim == 3 else al)
        assert not bad.any(), f"{form} {pop}: {name} differs from the oracle's, first at {np.argwhere(bad)[:3].tolist()}"
    seen = np.concatenate([al[:1], al[1:] | al[:-1], al[-1:]])          # blobs[t] is the state before step t and after step t - 1
    bad = (words(traj["blobs"]) != words(exp["blobs"])) & seen[:, None, :]
    assert not bad.any(), f"{form} {pop}: state words differ from the oracle's, first (step, column, env) {np.argwhere(bad)[:3].tolist()}"


def test_auto_reset_episodes_land_on_their_own_terrain(monkeypatch):
    """The seeded population on an auto-reset handle (staged resets), half in free fall and half under random actions, until every
    environment has spent SETTLE steps in its second episode or a later one: long enough to come down on that episode's ground.
    On a step that ends an episode the outputs belong to the old episode and the state to the new one, so only R1 applies there
    (the observation is the new state's); on every other step R1-R3 and R7 apply, and from the second episode on R4, R5 and R8
    too, on terrain(seed, gid, episode) of the blob's own episode column.  A wrong terrain shows as a flag or a crash away from
    the ground (R4, R5a), as a vertex below it (R8) or as a leg on it without its flag (R5c)."""
    pop, SETTLE, LIMIT = "seeded", 90, 300
    n = C.POPULATIONS[pop]["n"]
    env = handle(pop, "default", monkeypatch, auto_reset=True)
    assert env.info()["staged_resets"] == "1"
    env.reset()
    rng = np.random.default_rng(17)
    blobs, outs, acts = [np.array(env.get_state())], [], []
    in_later = np.zeros(n, int)
    while len(outs) < LIMIT and in_later.min() < SETTLE:
        acts.append(np.where(np.arange(n) % 2 == 1, rng.integers(0, 4, n), 0).astype(np.uint32))
        outs.append(tuple(np.array(v) for v in env.step(acts[-1])))
        blobs.append(np.array(env.get_state()))
        in_later += blobs[-1][26].view(np.uint32) >= 2
    env.close()
    ep = np.array([b[26].view(np.uint32) for b in blobs]).astype(np.int64)
    assert in_later.min() >= SETTLE, f"{int((in_later < SETTLE).sum())} environments have not spent {SETTLE} steps in a later episode after {LIMIT} steps"
    fails, judged = [], dict(steps=0, flagged=0, crashes=0)
    for t, (o, r, d, tr) in enumerate(outs):
        pre, post = blobs[t], blobs[t + 1]
        ending = d.astype(bool)
        assert np.array_equal(ep[t + 1] - ep[t], ending.astype(np.int64)), f"step {t}: the episode column does not count the endings"
        terr = C.terrain_of(pop, pre)
        later = ep[t] >= 2
        bad_obs = R.check(pre, post, acts[t], o, r, d, tr, True, terr, contact_rules=False)[0]["R1"]
        if bad_obs.any():
            fails.append(f"step {t} R1: envs {np.nonzero(bad_obs)[0][:5].tolist()}")
        for mask, contact in ((~ending & later, True), (~ending & ~later, False)):
            k = np.nonzero(mask)[0]
            if not len(k):
                continue
            has_prev = ep[t - 1][k] == ep[t][k] if t else np.zeros(len(k), bool)
            v, b, _ = R.check(pre[:, k], post[:, k], acts[t][k], o[:, k], r[k], d[k], tr[k], True, (terr[0], terr[1][k]),
                              prev=blobs[t - 1][:, k] if t else None, has_prev=has_prev, contact_rules=contact)
            fails += [f"step {t} {rule}: envs {k[x & ~b[rule]][:5].tolist()}" for rule, x in v.items() if (x & ~b[rule]).any()]
            if contact:
                judged["steps"] += len(k)
                judged["flagged"] += int((post[18:20, k] > 0.5).any(0).sum())
        # A -100 ending of a later episode well inside the viewport is a crash: the hull touched THAT episode's terrain within the step
        # (the post state is the next episode's, so the pre pose alone is the evidence).  How far it can have come: impacts are
        # inelastic (restitution 0), so the hull's kinetic energy E = m v^2 / 2 + I w^2 / 2 does not grow in the step but for the
        # engines, gravity and wind (together less than 1 m/s); a vertex at r from the centre moves at most at
        # sqrt(2 E / m) + r sqrt(2 E / I).
        k = np.nonzero(ending & later & (r == np.float32(-100.0)) & (np.abs(pre[0].astype(np.float64) - 10.0) < 8.0))[0]
        if len(k):
            g = R.geometry(pre[:, k], (terr[0], terr[1][k]))
            b = pre[:, k].astype(np.float64)
            mass, _, inertia = R.G.polygon_mass(R.G.shape(0), R.G.DENSITY[0])
            v_eq = np.sqrt(b[3] ** 2 + b[4] ** 2 + inertia / mass * b[5] ** 2) + 1.0
            travel = R.STEP_H * v_eq * (1.0 + R._RMAX[0] * np.sqrt(mass / inertia))
            far = g["dist"][0] > R.RADIUS + R.DELTA + travel
            if far.any():
                fails.append(f"step {t}: envs {k[far][:5].tolist()} ended {g['dist'][0][far][:5]} above the terrain of their episode")
            judged["crashes"] += len(k)
    print("auto-reset run:", len(outs), "steps,", judged)
    assert judged["steps"] >= SETTLE * n // 2 and judged["flagged"] >= 32 and judged["crashes"] >= 32
    assert not fails, "\n".join(fails[:12])
