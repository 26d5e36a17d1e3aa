"""No-GPU twin of tests/test_gpu_sincos_mid_range.py: the kernel source compiled for the host, stepped at the 34 angles where
mgym_math.h's sin / cos once differed from glibc (tests/sincos_mid_range.py), word for word against the CPU oracle, which calls
the host's glibc.  CartPole: tests/native/cartpole_mid_check.cpp, all four <is_euler, sutton_barto> variants.  LunarLander:
tests/native/ll_host_check.cpp in its `mid` form, free-flight and general paths."""
import re
import subprocess

import pytest

import native_build
from oracle import oracle as ora
from sincos_mid_range import HEX


pytestmark = pytest.mark.skipif(not native_build.host_has_fma(), reason="host CPU has no FMA: glibc runs its non-FMA sinf/cosf build, "
                                                            "which mgym_math.h does not restate")


def _build(src, out):
    ora.build()
    return native_build.program(src, out, extra=("-mfma",), link=(*native_build.ORACLE_LINK, "-lm"))


def test_cartpole_kernel_source_at_the_mid_range_angles_equals_oracle():
    exe = _build("cartpole_mid_check.cpp", "cartpole_mid_check")
    r = subprocess.run([exe, "6", *HEX], capture_output=True, text=True)
    m = re.search(r"checked=(\d+) mismatches=(\d+)", r.stdout)
    assert m, r.stdout + r.stderr
    assert int(m.group(1)) >= 4 * len(HEX) * 8 and int(m.group(2)) == 0, r.stdout
    assert r.returncode == 0, r.stdout


@pytest.mark.parametrize("general_only", [0, 1])
def test_lunar_lander_kernel_source_at_the_mid_range_angles_equals_oracle(general_only):
    exe = _build("ll_host_check.cpp", "ll_host_check_mid")
    r = subprocess.run([exe, "mid", "8", str(general_only), *HEX], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    m = re.search(r"envs=(\d+) .*mismatches=(\d+) exact_words=(\d+)/(\d+) episodes_done=(\d+) overflow=(\d+)", r.stdout)
    assert m, r.stdout
    envs, mism, exact, total, done, overflow = map(int, m.groups())
    assert envs == 4 * len(HEX) and mism == 0 and overflow == 0
    assert exact == total                      # every observation word bit-identical
    assert done == 0                           # all landers stayed in free flight
    f = re.search(r"fast-path steps (\d+), general-path steps (\d+)", r.stdout)
    fast, general = map(int, f.groups())
    assert (fast, general) == ((0, envs * 8) if general_only else (envs * 8, 0)), r.stdout
