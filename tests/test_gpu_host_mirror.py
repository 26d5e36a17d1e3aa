"""The C++ host-side mirror of the reference interface (include/mgym.hpp) run through the reference's
own unit tests (tests/native/host_mirror_test.cpp); needs a GPU."""
import subprocess

import pytest

import native_build

pytestmark = pytest.mark.gpu


def test_cpp_host_mirror_passes_reference_unit_tests():
    exe = native_build.program("host_mirror_test.cpp", base=(), extra=("-O1", "-std=c++17"), link=native_build.MGYM_LINK)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all reference unit tests passed" in r.stdout
