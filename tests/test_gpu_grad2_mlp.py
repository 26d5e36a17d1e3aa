"""mgym_ppo_grad_mlp2 and mgym_value_grad_mlp2 on the device: the tests of tests/test_gpu_grad_mlp.py at two hidden layers (its docstring gives the bounds and
the shapes)."""
import pytest

from test_gpu_grad_mlp import checks

pytestmark = pytest.mark.gpu
globals().update(checks(2))
