"""The classic families' kernels on the MI355X at the edges of their state spaces: the cases of tests/classic_edge_cases.py (exact clamp and goal
boundaries and their float neighbours, denormals, -0, angles on either side of the |angle| = 120 table reduction, fmodf quotients up to 1e30 / 2 pi,
non-finite imports) imported with mgym_set_state and stepped, every output word against the reference: the CPU oracle for CartPole, MountainCar and
MountainCarContinuous, the numpy restatements of include/mgym.h for Pendulum and Acrobot.  NaNs compare as a class, everything else bit for bit.

The host-compiled headers agree with the same references on the same cases (tests/test_classic_edge_cases.py), so a difference here is the device
build's: denormal flushing, a compare-select turned into a min / max / med3, the device library's fmodf, the divide's fix-up with denormal operands,
the fast and the table branch diverging inside one wave.

Populations are the builders' (at most 65 536, multiples of 1024); each runs in builder order and under one seeded shuffle, so that waves mix the
branches differently.  A reference is computed once per (family, order, run) and shared."""
import numpy as np
import pytest

import acrobot_ref as AR
import classic_edge_cases as E
import modurl_gym_amd as mg
import pendulum_ref as PR
from device_buffers import CallBuffers, FinalBuf
from families import FAMILIES
from mlp_ref import argmax_words
from oracle import oracle as ora
from time_limit_ref import TimeLimitRef
from words import same_words

pytestmark = pytest.mark.gpu

F = np.float32
SEED = 0xED6E5


# ---- families ---------------------------------------------------------------------------------------------------------------------------
class Family:
    """a family of tests/families.py with what is this file's: the edge cases, the configuration and a subset of the cases"""

    def __init__(self, name, cases, cfg=None, subset=None):
        self.name, self._cases, self.cfg, self.subset = name, cases, cfg or {}, subset
        self.table = FAMILIES[name.split("-")[0]]
        self.kind, self.okind, self.f32_cols, self.limit_ok = self.table.kind, self.table.okind, self.table.f32_cols, self.table.limit_ok

    def cases(self):
        blob, a = self._cases()
        if self.subset is not None:
            idx = self.subset()
            blob, a = np.ascontiguousarray(blob[:, idx]), np.ascontiguousarray(a[idx])
        return blob, a


EDGES = [Family(f"cartpole-sb{int(sb)}-euler{int(eu)}", E.cartpole_cases, dict(sutton_barto_reward=sb, is_euler=eu)) for sb, eu in E.CP_CONFIGS]
EDGES += [Family(f"mountain_car-gv{gv}", lambda: E.mountain_car_cases(False), dict(goal_velocity=gv)) for gv in E.MC_GOAL_VELOCITIES]
EDGES += [Family(f"mountain_car_continuous-gv{gv}", lambda: E.mountain_car_cases(True), dict(goal_velocity=gv)) for gv in E.MC_GOAL_VELOCITIES]
EDGES += [Family("pendulum-g10", E.pendulum_cases, dict(gravity=10.0))]
EDGES += [Family(f"pendulum-g{g}", E.pendulum_cases, dict(gravity=g), subset=E.pendulum_gravity_subset) for g in (0.0, -3.5)]
EDGES += [Family("acrobot", E.acrobot_cases)]
NON_FINITE = [Family("pendulum-non_finite", lambda: E.non_finite_cases("pendulum"), dict(gravity=10.0)),
              Family("acrobot-non_finite", lambda: E.non_finite_cases("acrobot")),
              Family("mountain_car_continuous-non_finite", lambda: E.non_finite_cases("mountain_car_continuous"), dict(goal_velocity=0.0))]
BY_NAME = {f.name: f for f in EDGES + NON_FINITE}
NAMES = [f.name for f in EDGES]
ONE_PER_KIND = ["cartpole-sb0-euler1", "mountain_car-gv0.0", "mountain_car_continuous-gv0.03", "pendulum-g10", "acrobot"]


class PdRef(PR.PendulumRef):
    """PendulumRef that keeps the observation a finished environment had before its fused reset"""

    def _reset_where(self, m):
        self.final = self.obs()
        super()._reset_where(m)

    def step(self, a):
        self.final = None
        out = super().step(a)
        if self.final is None:
            self.final = out[0]
        return out


class Ref:
    """the family's reference behind one surface: import, observation, step -> (obs, reward, done, truncated) and the pre-reset observation"""

    def __init__(self, fam, blob, limit, auto):
        n = blob.shape[1]
        self.fam, self.n = fam, n
        if fam.okind is not None:
            # (tests/time_limit_ref.py, for CartPole too, whose own step truncates at 500: its flag is OR-ed in)
            self.r = TimeLimitRef(ora.OracleVec(fam.okind, n, seed=SEED, **fam.cfg), limit, auto, own_truncation=not fam.limit_ok)
            self.r.ref.set_state(np.ascontiguousarray(blob).view(F))
            self._obs0 = np.ascontiguousarray(blob[:fam.f32_cols]).view(F).copy()
        elif fam.kind == mg.PENDULUM:
            self.r = PdRef(n, SEED, 0, fam.cfg["gravity"], limit, auto)
            self.r.set_state(blob)
        else:
            self.r = AR.AcrobotRef(n, SEED, 0, limit, auto)
            self.r.set_state(blob)

    def obs0(self):
        return self._obs0 if self.fam.okind is not None else self.r.obs()

    def step(self, a):
        out = self.r.step(a)
        self.final = self.r.final_obs if self.fam.okind is not None else self.r.final
        return out

    def state(self):
        return (self.r.ref.get_state() if self.fam.okind is not None else self.r.get_state()).view(np.uint32)

    def elapsed(self):
        return np.asarray(self.r.elapsed, np.uint32)

    @property
    def finished(self):
        return self.r.finished


def same_state(fam, got, exp):
    g, e = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(exp).view(np.uint32)
    k = fam.f32_cols
    return same_words(g[:k].view(F), e[:k].view(F)) and np.array_equal(g[k:], e[k:])


def assert_step(got, exp, what):
    for g, e, name in zip(got, exp, ("obs", "reward", "done", "truncated")):
        if e.dtype == np.float32:
            bad = ~((np.ascontiguousarray(g, F).view(np.uint32) == np.ascontiguousarray(e, F).view(np.uint32)) | (np.isnan(g) & np.isnan(e)))
        else:
            bad = g != e
        assert not bad.any(), f"{what}: {name} differs on {int(bad.sum())} words, first at {np.argwhere(bad)[0].tolist()}: got {g[bad][:4]}, expected {e[bad][:4]}"


# ---- cases, orders, action tables and the shared references ---------------------------------------------------------------------------------
_cases, _refs = {}, {}


def cases(name, order, ragged=False):
    """(blob, actions) of the family in builder order or under the seeded shuffle; ragged: without the last case (n - 1 is no multiple of 4)"""
    key = (name, order, ragged)
    if key not in _cases:
        blob, a = BY_NAME[name].cases()
        if order == "shuffled":
            perm = np.random.default_rng(99).permutation(blob.shape[1])
            blob, a = blob[:, perm], a[perm]
        if ragged:
            blob, a = blob[:, :-1], a[:-1]
        _cases[key] = (np.ascontiguousarray(blob), np.ascontiguousarray(a))
        for v in _cases[key]:
            v.setflags(write=False)
    return _cases[key]


def action_table(a, K):
    """the case actions, then rotations of them"""
    return np.stack([np.roll(a, 7 * t) for t in range(K)])


def reference(name, order, ragged, limit, auto, K, policy=None):
    """K reference steps from the imported cases -> dict(obs0, actions [K, n], steps [(obs, reward, done, trunc)], finals [K], state, elapsed, finished).
    policy: None = the action table, else a function of the observation held before the step.  Computed once, never changed."""
    key = (name, order, ragged, limit, auto, K, None if policy is None else policy[0])
    if key not in _refs:
        fam = BY_NAME[name]
        blob, a = cases(name, order, ragged)
        ref = Ref(fam, blob, limit, auto)
        obs = obs0 = ref.obs0()
        table = action_table(a, K)
        acts, steps, finals = [], [], []
        for t in range(K):
            act = table[t] if policy is None else policy[1](obs)
            out = ref.step(act)
            obs = out[0]
            acts.append(act), steps.append(tuple(np.array(x) for x in out)), finals.append(np.array(ref.final))
        _refs[key] = dict(obs0=np.array(obs0), actions=np.stack(acts), steps=steps, finals=finals, state=np.array(ref.state()), elapsed=ref.elapsed().copy(), finished=ref.finished)
    return _refs[key]


def make(fam, n, limit, auto):
    env = mg.VecEnv(fam.kind, n, seed=SEED, auto_reset=auto, max_episode_steps=limit if fam.limit_ok else 0, **fam.cfg)
    env.reset()
    return env


def imported(fam, blob, limit, auto):
    env = make(fam, blob.shape[1], limit, auto)
    env.set_state(blob.view(F))
    return env


def check_end(fam, env, exp, limit, what):
    assert same_state(fam, env.get_state(), exp["state"]), f"{what}: state blob"
    assert same_words(env.observation(), exp["steps"][-1][0]), f"{what}: engine observation"
    if limit and fam.limit_ok:
        assert np.array_equal(env.elapsed_steps(), exp["elapsed"]), f"{what}: elapsed"
    assert env.episode_count() == exp["finished"], f"{what}: episode_count"


# ---- one mgym_step through each launch form ----------------------------------------------------------------------------------------------------
# form: (MGYM_CLASSIC_MAX_BLOCKS, byte offset of the reward buffer, ragged population without obs_out)
FORMS = {"single_pass": (None, 0, False), "grid_stride": ("1", 0, False), "generic_one_per_lane": (None, 4, False), "generic_ragged_no_obs_out": (None, 0, True)}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", NAMES)
def test_one_step_through_each_launch_form(name, form, monkeypatch):
    """After the import: observation() is the reference's (the import kernels' own cos / sin at the edges) and get_state() returns the blob.  Then one
    mgym_step: obs, reward, done, truncated, the state blob, elapsed and episode_count().  max_episode_steps = 5: the instantiation that counts."""
    fam = BY_NAME[name]
    max_blocks, offset, ragged = FORMS[form]
    if max_blocks:
        monkeypatch.setenv("MGYM_CLASSIC_MAX_BLOCKS", max_blocks)   # read when the handle is created
    limit = 5
    for order in ("builder", "shuffled"):
        blob, a = cases(name, order, ragged)
        exp = reference(name, order, ragged, limit if fam.limit_ok else 0, False, 1)
        env = imported(fam, blob, limit, False)
        what = f"{name} {form} {order}"
        assert same_words(env.observation(), exp["obs0"]), f"{what}: observation after the import"
        assert same_state(fam, env.get_state(), blob), f"{what}: get_state after the import"
        buf = CallBuffers(env.n, env.obs_dim, env.action_dtype, 1, offset, not ragged)
        buf.put_actions(a)
        env.step_device(*buf.pointers())
        env.sync()
        o, r, d, t = buf.read()
        assert_step((o[0] if o is not None else env.observation(), r[0], d[0], t[0]), exp["steps"][0], what)
        check_end(fam, env, exp, limit, what)
        env.close()


# ---- mgym_rollout, K = 3: the fused kernel with the state in registers ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_rollout_of_three_steps(name):
    """step 1 is on the edge state, steps 2 and 3 on whatever it produced, under rotations of the case actions; no limit: the instantiation that does
    not count"""
    fam = BY_NAME[name]
    for order in ("builder", "shuffled"):
        blob, a = cases(name, order)
        exp = reference(name, order, False, 0, False, 3)
        env = imported(fam, blob, 0, False)
        got = env.rollout(action_table(a, 3))
        for t in range(3):
            assert_step([x[t] for x in got], exp["steps"][t], f"{name} {order} rollout step {t}")
        check_end(fam, env, exp, 0, f"{name} {order} rollout")
        env.close()


# ---- one policy instantiation of the rollout kernel: mgym_rollout_linear with zero weights --------------------------------------------------------
def constant_policies(fam):
    """-> [(id, host policy floats, reference policy: observation -> actions)]: all-zero weights and a bias that selects a constant action (a zero weight
    times a non-finite observation word is a NaN score: the reference evaluates the text's sum)"""
    D = fam.table.D
    out = []

    def zero_sum(obs):
        with np.errstate(all="ignore"):
            s = F(0) * obs[0]
            for q in range(1, D):
                s = s + F(0) * obs[q]
        return s.astype(F)

    if fam.kind == mg.CARTPOLE:
        for act, b in ((0, -1.0), (1, 1.0)):
            out.append((f"a{act}", np.array([0] * 4 + [b], F), lambda obs, b=b: ((zero_sum(obs) + F(b)) > 0).astype(np.uint32)))
    elif fam.kind in (mg.MOUNTAINCAR, mg.ACROBOT):
        for act in range(3):
            pol = np.zeros((3, D + 1), F)
            pol[act, D] = 1.0
            ref = (lambda obs, pol=pol: argmax_words(np.stack([zero_sum(obs) + pol[j, D] for j in range(3)])))
            out.append((f"a{act}", pol.ravel(), ref))
    else:
        top = fam.table.box[1]
        for b in (F(-top), np.nextafter(F(top), F(3)), F(1e30)):
            out.append((f"b{float(b):g}", np.array([0] * D + [b], F), lambda obs, b=b: (zero_sum(obs) + b).astype(F)))
    return out


@pytest.mark.parametrize("name", ONE_PER_KIND)
def test_linear_policy_rollout_with_a_constant_action(name):
    fam = BY_NAME[name]
    blob, a = cases(name, "builder")
    for pid, pol, ref_policy in constant_policies(fam):
        exp = reference(name, "builder", False, 0, False, 2, policy=(pid, ref_policy))
        env = imported(fam, blob, 0, False)
        got = env._rollout_host(2, lambda *out: env.rollout_linear_device(pol, 2, *out), env.action_dtype)
        what = f"{name} linear {pid}"
        assert np.array_equal(got[0].view(np.uint32), exp["actions"].view(np.uint32)), f"{what}: actions"
        for t in range(2):
            assert_step([x[t] for x in got[1:]], exp["steps"][t], f"{what} step {t}")
        check_end(fam, env, exp, 0, what)
        env.close()


# ---- endings: auto-reset and the final-observation channel ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", ["step", "rollout3"])
@pytest.mark.parametrize("name", ONE_PER_KIND + ["cartpole-sb1-euler0", "mountain_car_continuous-gv0.0"])
def test_endings_with_auto_reset_and_final_observations(name, call):
    """max_episode_steps = 1 (CartPole: the imported counters at 499 and 500 and the threshold cases): the final observation of every finished env-step
    is the observation the step produced before the fused reset — edge, denormal and NaN words alike — obs_out holds the reset observation, and no
    other word of the channel's buffer is written"""
    fam = BY_NAME[name]
    K = 1 if call == "step" else 3
    blob, a = cases(name, "builder")
    exp = reference(name, "builder", False, 1 if fam.limit_ok else 0, True, K)
    fin = [(s[2] | s[3]).astype(bool) for s in exp["steps"]]
    assert fin[0].sum() >= blob.shape[1] // 4 and (fam.limit_ok or not fin[0].all())
    env = imported(fam, blob, 1, True)
    fb = FinalBuf(K, env.obs_dim, env.n)
    env.set_final_obs_out_device(fb.ptr, K)
    if call == "step":
        got = [x[None] for x in env.step(a)]
    else:
        got = env.rollout(action_table(a, K))
    for t in range(K):
        assert_step([x[t] for x in got], exp["steps"][t], f"{name} {call} step {t}")
    fb.check(exp["finals"], fin, f"{name} {call}", same_words)
    check_end(fam, env, exp, 1, f"{name} {call}")
    env.set_final_obs_out_device(None)
    env.close()


# ---- a NaN torque or force on a step that truncates and auto-resets ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pendulum-g10", "mountain_car_continuous-gv0.0"])
def test_nan_action_on_a_truncating_step(name):
    """The refused step leaves the state and gives reward 0 and done 0, but the elapsed count advances: with max_episode_steps = 1 the environment is
    truncated and reset, and its final observation is the untouched imported one.  The other environments of its lane equal the reference, and the
    sticky MGYM_ERR_INVALID_ACTION is reported at the sync."""
    fam = BY_NAME[name]
    blob, a = (np.array(x) for x in cases(name, "builder"))
    n = blob.shape[1]
    bad = np.array([1, 6, 1027, n - 1])   # lanes 0, 1, 256 and the last one: each shares its lane with three cases
    rest = (F(0), F(0)) if fam.kind == mg.PENDULUM else (F(-0.5), F(0))   # (the oracle refuses a NaN: there the bad environments step from rest with force 0)
    blob[0, bad], blob[1, bad] = E.words(rest[0]), E.words(rest[1])
    a_ref = a.copy()
    a_ref[bad] = 0
    a[bad] = np.nan
    ref = Ref(fam, blob, 1, True)
    obs0 = np.array(ref.obs0())
    eo, er, ed, et = (np.array(x) for x in ref.step(a if fam.kind == mg.PENDULUM else a_ref))
    finals = np.array(ref.final)
    finals[:, bad], er[bad], ed[bad] = obs0[:, bad], 0, 0
    assert np.all(et == 1)
    env = imported(fam, blob, 1, True)
    fb = FinalBuf(1, env.obs_dim, env.n)
    env.set_final_obs_out_device(fb.ptr, 1)
    buf = CallBuffers(env.n, env.obs_dim, env.action_dtype)
    buf.put_actions(a)
    env.step_device(*buf.pointers())
    with pytest.raises(mg.InvalidActionError):
        env.sync()
    o, r, d, t = buf.read()
    assert_step((o[0], r[0], d[0], t[0]), (eo, er, ed, et), f"{name} NaN action")
    fb.check([finals], [np.ones(n, bool)], f"{name} NaN action", same_words)
    assert not env.elapsed_steps().any() and env.episode_count() == n   # every environment was truncated and reset, the refused ones too
    assert same_state(fam, env.get_state(), ref.state())
    env.sync()   # the status was cleared
    env.set_final_obs_out_device(None)
    env.close()


# ---- non-finite imported states --------------------------------------------------------------------------------------------------------------------
def non_finite_run(name):
    """one mgym_step through the 16-byte kernel, then (on a second handle) a table rollout of two steps: every word as the reference's, NaNs as a
    class, and the call returns"""
    fam = BY_NAME[name]
    blob, a = cases(name, "builder")
    exp = reference(name, "builder", False, 0, False, 2)
    nan_results = np.isnan(exp["steps"][0][0]).any(axis=0) | np.isnan(exp["steps"][0][1])
    assert nan_results.sum() >= 32   # the reference really produces NaNs here (the builder asserts its own minimum)
    env = imported(fam, blob, 0, False)
    assert same_words(env.observation(), exp["obs0"]) and same_state(fam, env.get_state(), blob)
    assert_step(env.step(a), exp["steps"][0], f"{name} step")
    env.close()
    env = imported(fam, blob, 0, False)
    got = env.rollout(action_table(a, 2))
    for t in range(2):
        assert_step([x[t] for x in got], exp["steps"][t], f"{name} rollout step {t}")
    check_end(fam, env, exp, 0, f"{name} rollout")
    env.close()


def test_non_finite_states_pendulum():
    """+-inf and NaN in th and in thdot.  Read in the device assembly of the build under test before this first ran: every loop of pendulum_step4_kernel,
    pendulum_step_kernel and the pendulum_rollout_kernel instantiations is counted by integers — the grid-stride and K loops by scalar integer compares,
    and the fmodf expansion's only loop by an exponent difference (v_frexp_exp_i32_f32, which gives 0 for an infinity or a NaN; 12 is taken off per pass
    and the pass ends on an integer compare with 13): at most 11 passes whatever the float holds.  No branch is fed by a float compare of a loop-carried
    value."""
    non_finite_run("pendulum-non_finite")


def test_non_finite_states_acrobot():
    """+-inf and NaN in th1, th2, w1 and w2: NaNs, done = 0, and the call returns (include/mgym.h).  The loops of the acrobot step and rollout kernels
    are those of Pendulum's (the two wraps' fmodf expansions, integer-counted by the exponent difference; grid-stride and K loops on scalar integer
    compares), read in the device assembly of the build under test."""
    non_finite_run("acrobot-non_finite")


def test_non_finite_states_mountain_car_cont():
    """+-inf and NaN in position and in velocity.  The MountainCarContinuous step has no fmodf and no data-dependent loop at all: the device assembly
    holds only the grid-stride and K loops, on scalar integer compares."""
    non_finite_run("mountain_car_continuous-non_finite")
