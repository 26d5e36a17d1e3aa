"""The engine's three forms of an airborne LunarLander step against the float64 reference of the step (tests/ll_flight_ref.py):
the register-resident free-flight path of mgym_step (ll_free.h), the general path every env takes under MGYM_LL_GENERAL_ONLY=1
(ll_world.h), and the free-flight mode of the persistent rollout launch (ll_roll.h).  The cases, protocol and bounds are those of
tests/test_ll_flight_oracle.py (tests/ll_flight_cases.py), with the engine in place of the oracle; the number of cases is no
multiple of a wave.  The engine's words are also held equal to the oracle's, which is cheap and says on which side a failure is."""
import numpy as np
import pytest

import ll_flight_cases as FC
import modurl_gym_amd as mg
from oracle import oracle as ora

pytestmark = pytest.mark.gpu

PATHS = {"step": {}, "general_only": {"MGYM_LL_GENERAL_ONLY": "1"}, "rollout": {"MGYM_LL_ROLLOUT": "1", "MGYM_LL_ROLLOUT_MIN_K": "8"}}


def words(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def engine(path, name, monkeypatch, **kw):
    g, wind, wp, tp = FC.PARAMS[name]
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    env = mg.VecEnv(mg.LUNARLANDER, FC.cases()[0].shape[1], gravity=g, enable_wind=wind, wind_power=wp, turbulence_power=tp, **kw)
    for k in PATHS[path]:
        monkeypatch.delenv(k)
    info = env.info()
    assert (info["rollout"] == "persistent_launch" and info["rollout_min_k"] == "8") if path == "rollout" else (path != "general_only" or info["rollout"] == "k_steps")
    return env


_ORACLE = {}


def oracle_steps(name):
    """the oracle's outputs and blobs of protocol (a), computed once per parameter set"""
    if name not in _ORACLE:
        g, wind, wp, tp = FC.PARAMS[name]
        ref = ora.OracleVec(ora.LUNARLANDER, FC.cases()[0].shape[1], gravity=g, enable_wind=wind, wind_power=wp, turbulence_power=tp)
        ref.reset_deterministic()
        ref.set_state(FC.start_blob(ref))
        _ORACLE[name] = [tuple(np.array(x) for x in ref.step(a, nthreads=8)) + (ref.get_state(),) for a in FC.cases()[1]]
    return _ORACLE[name]


@pytest.mark.parametrize("name", list(FC.PARAMS))
@pytest.mark.parametrize("path", list(PATHS))
def test_engine_steps_match_the_float64_reference(path, name, monkeypatch):
    assert FC.T >= 8                               # the rollout path's MGYM_LL_ROLLOUT_MIN_K
    env = engine(path, name, monkeypatch)
    outs = FC.check_against_reference(env, name, f"{path} {name}", rollout=(path == "rollout"))
    for t, (got, exp) in enumerate(zip(outs, oracle_steps(name))):
        for g, e, nm in zip(got, exp, ("obs", "reward", "done", "truncated", "state")):
            if g is not None:
                assert np.array_equal(words(g), words(e)), f"{path} {name} step {t}: {nm} differs from the oracle's at {np.argwhere(words(g) != words(e))[:3].tolist()}"
    env.close()


def test_engine_dispersion_matches_the_float64_reference(monkeypatch):
    n = FC.cases()[0].shape[1]
    g, wind, wp, tp = FC.PARAMS["wind"]
    kw = dict(seed=7, gravity=g, enable_wind=wind, wind_power=wp, turbulence_power=tp)
    got = FC.check_dispersion_differential(lambda: engine("step", "wind", monkeypatch, seed=7), "engine")
    exp = FC.check_dispersion_differential(lambda: ora.OracleVec(ora.LUNARLANDER, n, **kw), "oracle")
    for g_, e_, nm in zip(got, exp, ("after reset", "with dispersion", "without dispersion")):
        assert np.array_equal(words(g_), words(e_)), f"{nm}: the engine's blob differs from the oracle's at {np.argwhere(words(g_) != words(e_))[:3].tolist()}"
