"""Adaptive progressive rendering (rtiow_accumulate_adaptive): the parts that need no GPU.
The checks themselves are the rows of tests/test_abi.py and tests/test_kernel_inventory.py; this module keeps its test ids and runs
its feature's rows through tests/kept_abi_ids.py."""
from tests import kept_abi_ids as kept
from tests import test_kernel_inventory as inventory

SYMBOLS = ("rtiow_accumulate_adaptive", "rtiow_read_adaptive_state")
MEMBERS = ("accumulate_adaptive", "adaptive_state")


def test_adaptive_symbols_are_declared_listed_and_exported(native):
    kept.symbols(SYMBOLS)


def test_renderer_has_the_adaptive_interface(native):
    kept.wrappers(SYMBOLS, MEMBERS)


def test_bad_arguments_need_no_gpu(native):
    kept.null_handles(SYMBOLS)


def test_adaptive_kernels_meet_the_main_launch_register_budget(native):
    inventory.check_budget("render_adaptive_kernel")
    inventory.check_row("adaptive_select_kernel<")              # these two: no SGPR spills either
    inventory.check_row("adaptive_finish_kernel<")
