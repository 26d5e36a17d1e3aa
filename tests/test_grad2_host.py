"""No-GPU checks of the words of mgym_ppo_grad_mlp2 and mgym_value_grad_mlp2: the tests of tests/test_grad_host.py at two hidden layers (its docstring says
what they check and where the bounds come from)."""
from test_grad_host import checks

globals().update(checks(2))
