import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# The suite runs the hardware-queue configuration the package asks for (modurl_gym_amd/__init__.py), whatever the calling
# environment presets: the package lets an embedder's own value win (setdefault), and with fewer queues LunarLander's helper
# streams share them, so the multi-stream launch order and its graph replays would be tested in a configuration that was never
# validated.  Set before any test module initialises HIP; the embedder-wins rule itself is checked in child processes
# (tests/test_bench_helpers.py).
os.environ["GPU_MAX_HW_QUEUES"] = "8"


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def golden():
    import json

    def load(name):
        with open(os.path.join(ROOT, "tests", "golden", f"{name}.json")) as f:
            return json.load(f)

    return load
