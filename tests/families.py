"""What a family is, once: the engine's kind and the CPU oracle's, the observation width D, the number of policy scores A (a box family has one, and its
score is the action), the action space, the floats of a linear policy, the columns of the state blob and of the engine, and whether max_episode_steps may
be set.  One spelling per family, the keys below.  tests/test_support.py checks the table against mgym_get_spec.  No test here."""
from collections import namedtuple

import modurl_gym_amd as mg
from oracle import oracle as ora

# okind: None where the CPU oracle has no such family.  box: the action bounds, None for a discrete family of n_actions actions.  lin: the floats of
# mgym_rollout_linear's policy.  f32_cols of the state_cols of the state blob are float32, the rest uint32 counters.  engine_cols: f32 / u32 columns the
# engine allocates, n_pad words apart (LunarLander keeps records, not columns, and its blob is not split here).  limit_ok: CartPole keeps its own 500 steps.
Family = namedtuple("Family", "kind okind D A n_actions box lin f32_cols state_cols engine_cols limit_ok")

FAMILIES = {
    "cartpole": Family(mg.CARTPOLE, ora.CARTPOLE, 4, 2, 2, None, 5, 4, 7, 5, False),
    "mountain_car": Family(mg.MOUNTAINCAR, ora.MOUNTAINCAR, 2, 3, 3, None, 9, 2, 3, 3, True),
    "mountain_car_continuous": Family(mg.MOUNTAINCAR_CONT, ora.MOUNTAINCAR_CONT, 2, 1, 0, (-1.0, 1.0), 3, 2, 3, 3, True),
    "pendulum": Family(mg.PENDULUM, None, 3, 1, 0, (-2.0, 2.0), 4, 2, 3, 5, True),
    "acrobot": Family(mg.ACROBOT, None, 6, 3, 3, None, 21, 4, 5, 9, True),
    "lunar_lander": Family(mg.LUNARLANDER, ora.LUNARLANDER, 8, 4, 4, None, 36, None, 27, None, True),
}
CLASSIC = [name for name in FAMILIES if name != "lunar_lander"]
KIND = {name: f.kind for name, f in FAMILIES.items()}
BY_KIND = {f.kind: f for f in FAMILIES.values()}
