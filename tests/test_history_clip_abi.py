"""History clipped to the neighbourhood colours (rtiow_history_update_clipped): the parts that need no GPU.
The checks themselves are the rows of tests/test_abi.py and tests/test_kernel_inventory.py; this module keeps its test ids and runs
its feature's rows through tests/kept_abi_ids.py."""
from tests import kept_abi_ids as kept

SYMBOLS = ("rtiow_history_update_clipped",)
MEMBERS = ("history_update_clipped", "history_update")


def test_symbol_is_declared_listed_and_exported(native):
    kept.symbols(SYMBOLS)


def test_renderer_has_the_clipped_update(native):
    kept.wrappers(SYMBOLS + ("rtiow_history_update",), MEMBERS)


def test_null_handle_needs_no_gpu(native):
    kept.null_handles(SYMBOLS)


def test_clip_kernel_has_no_scratch_and_no_vgpr_spills(native):
    kept.kernels("history_clip_kernel<")
