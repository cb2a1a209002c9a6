"""Temporal history (rtiow_history_*, rtiow_denoise_history): the parts that need no GPU.
The checks themselves are the rows of tests/test_abi.py and tests/test_kernel_inventory.py; this module keeps its test ids and runs
its feature's rows through tests/kept_abi_ids.py."""
from tests import kept_abi_ids as kept

SYMBOLS = ("rtiow_history_reset",
           "rtiow_history_update",
           "rtiow_history_commit",
           "rtiow_read_history",
           "rtiow_history_device_ptr",
           "rtiow_denoise_history")
MEMBERS = ("history_reset", "history_update", "history_commit", "history", "history_device_ptr", "denoise_history")


def test_history_symbols_are_declared_listed_and_exported(native):
    kept.symbols(SYMBOLS)


def test_renderer_has_the_history_interface(native):
    kept.wrappers(SYMBOLS, MEMBERS)


def test_null_handle_needs_no_gpu(native):
    kept.null_handles(SYMBOLS)


def test_history_kernel_has_no_scratch_and_no_vgpr_spills(native):
    kept.kernels("history_reproject_kernel<")
