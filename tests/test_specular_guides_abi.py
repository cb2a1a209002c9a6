"""Filter guides through mirrors and glass (rtiow_set_guide_mode, rtiow_read_filter_guides): the parts that need no GPU.
The checks themselves are the rows of tests/test_abi.py and tests/test_kernel_inventory.py; this module keeps its test ids and runs
its feature's rows through tests/kept_abi_ids.py."""
from tests import kept_abi_ids as kept

SYMBOLS = ("rtiow_set_guide_mode", "rtiow_read_filter_guides")
MEMBERS = ("set_guide_mode", "filter_guides")


def test_guide_mode_symbols_are_declared_listed_and_exported(native):
    kept.symbols(SYMBOLS)


def test_renderer_has_the_guide_mode_interface(native):
    kept.wrappers(SYMBOLS, MEMBERS, constants=("GUIDE_MAX_BOUNCES", "GUIDE_MAX_FUZZ"))


def test_null_handle_needs_no_gpu(native):
    kept.null_handles(SYMBOLS)


def test_guide_chain_kernel_has_no_scratch_and_no_vgpr_spills(native):
    kept.kernels("guide_chain_kernel<")
