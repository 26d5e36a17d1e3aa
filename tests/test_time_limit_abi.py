"""No-GPU checks of the episode time limit's public surface (include/mgym.h: mgym_config::max_episode_steps,
mgym_get_elapsed_steps / mgym_set_elapsed_steps): the field and the two calls exist in the header, the ctypes table, the Rust FFI
and the library; the default is 0 (the reference's behaviour); and out-of-range limits are rejected by mgym_create before any HIP
call, so also on a machine without a GPU."""
import ctypes as C
import os
import re

import pytest

import modurl_gym_amd as mg
from modurl_gym_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("mgym_get_elapsed_steps", "mgym_set_elapsed_steps")


def test_config_field_is_renamed_in_place():
    names = [f[0] for f in _lib.Config._fields_]
    assert names[-1] == "max_episode_steps" and "reserved" not in names
    assert C.sizeof(_lib.Config) == 72 and _lib.Config.max_episode_steps.offset == 68   # size and layout unchanged: ABI stays version 4
    assert _lib.load().mgym_abi_version() == 4
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mgym.h")).read(), flags=re.S)
    body = re.search(r"typedef struct mgym_config \{(.*?)\}", header, re.S).group(1)
    assert re.search(r"uint32_t\s+max_episode_steps;\s*$", body.strip()) and "reserved" not in body
    sys_rs = open(os.path.join(ROOT, "rust", "modurl_gym_mgym", "src", "sys.rs")).read()
    assert "pub max_episode_steps: u32," in sys_rs and "pub reserved" not in sys_rs


def test_elapsed_step_calls_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "mgym.h")).read()
    sys_rs = open(os.path.join(ROOT, "rust", "modurl_gym_mgym", "src", "sys.rs")).read()
    lib = C.CDLL(_lib.LIB_PATH)
    for name in CALLS:
        assert re.search(r"\bint %s\(mgym_env \*env, (const )?uint32_t \*(out|in)\);" % name, header), name
        assert hasattr(lib, name), f"libmgym.so does not export {name}"
        assert name in _lib.PROTOTYPES
        assert re.search(r"pub fn %s\(" % name, sys_rs), name


@pytest.mark.parametrize("kind", [mg.CARTPOLE, mg.MOUNTAINCAR, mg.MOUNTAINCAR_CONT, mg.LUNARLANDER])
def test_default_config_leaves_the_limit_off(kind):
    cfg = _lib.Config()
    cfg.max_episode_steps = 12345
    assert _lib.load().mgym_default_config(kind, C.byref(cfg)) == _lib.OK
    assert cfg.max_episode_steps == 0


def _status_of_create(kind, limit):
    """mgym_create's status for this limit: on a machine without a GPU an accepted configuration gets as far as ERR_NO_DEVICE"""
    try:
        mg.VecEnv(kind, 4, max_episode_steps=limit).close()
        return _lib.OK
    except mg.MgymError as e:
        return e.status


def test_bad_limits_are_rejected_before_touching_the_gpu():
    with pytest.raises(mg.BadConfigError):      # CartPole keeps the reference's 500 (cartpole.rs:297)
        mg.VecEnv(mg.CARTPOLE, 4, max_episode_steps=7)
    with pytest.raises(mg.BadConfigError):
        mg.VecEnv(mg.CARTPOLE, 4, max_episode_steps=499)
    for kind in (mg.MOUNTAINCAR, mg.MOUNTAINCAR_CONT, mg.LUNARLANDER):
        with pytest.raises(mg.BadConfigError):  # the count is kept in 16 bits
            mg.VecEnv(kind, 4, max_episode_steps=65536)
        with pytest.raises(mg.BadConfigError):
            mg.VecEnv(kind, 4, max_episode_steps=0xFFFFFFFF)
    with pytest.raises(mg.BadConfigError):
        mg.VecEnv(mg.MOUNTAINCAR, 4, max_episode_steps=-1)


def test_good_limits_pass_the_configuration_check():
    ok = (_lib.OK, _lib.ERR_NO_DEVICE)   # accepted: created, or (no GPU here) refused only for the missing device
    assert _status_of_create(mg.CARTPOLE, 0) in ok and _status_of_create(mg.CARTPOLE, 500) in ok
    for kind in (mg.MOUNTAINCAR, mg.MOUNTAINCAR_CONT, mg.LUNARLANDER):
        for limit in (0, 1, 200, 65535):
            assert _status_of_create(kind, limit) in ok, (kind, limit)


def test_single_env_classes_take_the_argument():
    import inspect
    for cls in (mg.MountainCarV0, mg.MountainCarContinuousV0, mg.LunarLanderV3):
        assert inspect.signature(cls.__init__).parameters["max_episode_steps"].default == 0
    assert "max_episode_steps" not in inspect.signature(mg.CartPoleV1.__init__).parameters
    shim = open(os.path.join(ROOT, "rust", "modurl_gym_mgym", "src", "lib.rs")).read()
    for name in ("MountainCarV0", "LunarLanderV3"):
        body = re.search(r"#\[bon\]\s*impl %s \{(.*?)\n\}" % name, shim, re.S).group(1)
        assert re.search(r"#\[builder\(default = 0\)\]\s*max_episode_steps: u32,", body), name
    hpp = open(os.path.join(ROOT, "include", "mgym.hpp")).read()
    assert hpp.count("Builder& max_episode_steps(uint32_t k)") == 2
