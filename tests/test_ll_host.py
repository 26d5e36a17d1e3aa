"""No-GPU check of the LunarLander KERNEL SOURCE: modurl_gym_amd/csrc/ll_{b2,world,env}.h are compiled
for the host (tests/native/ll_host_check.cpp supplies a shim for the HIP qualifiers) and stepped
side by side with the CPU oracle on identical seeds, actions and Philox dispersion draws.
Also covers the device math header against the host's glibc (tests/native/math_host_check.cpp, sampled, and
tests/native/math_glibc_exhaustive.cpp, every bit pattern)."""
import os
import re
import subprocess

import pytest

import native_build
from oracle import oracle as ora


@pytest.fixture(scope="module")
def ll_host():
    ora.build()
    return native_build.program("ll_host_check.cpp", link=(*native_build.ORACLE_LINK, "-lm"))


@pytest.mark.parametrize("n,steps,wind,det,toi_staged,physics", [(64, 300, 0, 1, 1, ()), (256, 400, 0, 0, 1, ()), (256, 400, 1, 0, 1, ()), (256, 300, 1, 0, 0, ()),
                                                                  (192, 500, 1, 0, 1, (-3.5, 19.5, 1.95)), (192, 300, 1, 0, 1, (-11.9, 0.5, 0.1))])
def test_kernel_source_matches_oracle_on_cpu(ll_host, n, steps, wind, det, toi_staged, physics):
    """toi_staged = 0: the contact cache's TOI word stays in its column (the 64-lane blocks' layout); in every case the
    velocity constraints beyond the fourth go through the far-workspace path.  physics = (gravity, wind_power, turbulence_power) near the
    ends of the ranges the builder accepts: the sweep loops' early exits (fixed point, cycle, settled velocity) are proofs about the
    constraint arithmetic and must give the full 180 / 60 iterations' words — which the oracle runs — under any of them."""
    r = subprocess.run([ll_host, str(n), str(steps), str(wind), str(det), str(toi_staged), *map(str, physics)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    m = re.search(r"mismatches=(\d+) exact_words=(\d+)/(\d+) episodes_done=(\d+) overflow=(\d+)", r.stdout)
    assert m, r.stdout
    mism, exact, total, done, overflow = map(int, m.groups())
    assert mism == 0 and overflow == 0
    assert exact == total          # same operation order: every observation word is bit-identical
    assert done > n                # the contact / TOI / crash paths ran many times


def test_device_math_header_matches_glibc():
    exe = native_build.program("math_host_check.cpp")
    out = subprocess.run([exe, "997"], capture_output=True, text=True, check=True).stdout
    rows = {l.split()[0]: dict(kv.split("=") for kv in l.split()[1:]) for l in out.strip().splitlines()}
    for fn in ("sinf", "cosf", "tanhf", "sincosf_self", "sincosf_uniform_vs_sincosf"):
        assert int(rows[fn]["bad_fast"]) == 0, out      # |x| <= 16: every angle the environments produce
    assert int(rows["sinf"]["bad_large"]) == 0 and int(rows["cosf"]["bad_large"]) == 0
    # 16 < |x| < 120: reduce_fast fuses x - n*pi/2 as glibc's FMA build does (mgym_math.h), so no input may differ here either
    assert int(rows["sinf"]["bad_mid"]) + int(rows["cosf"]["bad_mid"]) <= 8, out
    if native_build.host_has_fma():
        assert int(rows["sinf"]["bad_mid"]) == 0 and int(rows["cosf"]["bad_mid"]) == 0, out
    assert int(rows["tanhf"]["bad_mid"]) == 0 and int(rows["tanhf"]["bad_large"]) == 0


def test_device_math_header_matches_glibc_on_every_pattern():
    """All 2^32 f32 bit patterns, both signs, through every sin/cos entry point of mgym_math.h (mg_sinf, mg_cosf, mg_sincosf,
    mg_sincosf_u, mg_cosf_u) and mg_tanhf against the host's glibc: no mismatch in any range (NaN results compared as a class).
    Before reduce_fast fused its subtraction, 34 inputs with 16 < |x| < 120 differed by one ulp (12 sin, 22 cos)."""
    if not native_build.host_has_fma():
        pytest.skip("host CPU has no FMA: glibc runs its non-FMA sinf/cosf build, which mgym_math.h does not restate")
    exe = native_build.program("math_glibc_exhaustive.cpp", extra=("-mfma", "-fopenmp"))
    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    r = subprocess.run([exe, str(threads)], capture_output=True, text=True)
    rows = {l.split()[0]: dict(kv.split("=") for kv in l.split()[1:]) for l in r.stdout.strip().splitlines()}
    assert sorted(rows) == sorted(["sinf", "cosf", "sincosf.sin", "sincosf.cos", "sincosf_u.sin", "sincosf_u.cos", "cosf_u", "tanhf"]), r.stdout + r.stderr
    for fn, row in rows.items():
        assert int(row["total"]) == 1 << 32, r.stdout
        for cls in ("bad_fast", "bad_mid", "bad_large", "bad_nonfinite"):
            assert int(row[cls]) == 0, f"{fn} {cls}: {r.stdout}"
    assert r.returncode == 0, r.stdout + r.stderr


def test_kernel_source_is_clean_under_asan_and_ubsan():
    """GPU AddressSanitizer is not available on the pool, and an out-of-bounds index in a kernel can take a GPU
    down: run the same kernel source on the host under ASan + UBSan (contact cache, constraint tables, worklists)."""
    ora.build()
    exe = native_build.program("ll_host_check.cpp", "ll_host_check_san", base=(), link=(*native_build.ORACLE_LINK, "-lm"),
                               extra=("-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe, "128", "350", "1", "0"], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert re.search(r"mismatches=0 ", r.stdout), r.stdout[-2000:]
