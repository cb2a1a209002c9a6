"""Progressive rendering (rtiow_accumulate): the parts that need no GPU.
The checks themselves are the rows of tests/test_abi.py and tests/test_kernel_inventory.py; this module keeps its test ids and runs
its feature's rows through tests/kept_abi_ids.py."""
from tests import kept_abi_ids as kept
from tests import test_kernel_inventory as inventory

SYMBOLS = ("rtiow_accumulate", "rtiow_accumulate_reset", "rtiow_accumulated_samples")
MEMBERS = ("accumulate", "reset_accumulation", "accumulated_samples")


def test_accumulate_symbols_are_declared_listed_and_exported(native):
    kept.symbols(SYMBOLS)


def test_renderer_has_the_progressive_interface(native):
    kept.wrappers(SYMBOLS, MEMBERS)


def test_accumulate_kernels_meet_the_main_launch_register_budget(native):
    inventory.check_budget("render_accumulate_kernel")
