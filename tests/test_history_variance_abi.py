"""Variance-guided filtering of the temporal image (rtiow_denoise_history_variance, rtiow_read_history_variance): the parts that need no GPU.
The checks themselves are the rows of tests/test_abi.py and tests/test_kernel_inventory.py; this module keeps its test ids and runs
its feature's rows through tests/kept_abi_ids.py."""
from tests import kept_abi_ids as kept

SYMBOLS = ("rtiow_denoise_history_variance", "rtiow_read_history_variance")
MEMBERS = ("denoise_history_variance", "history_variance", "denoise_variance")


def test_symbols_are_declared_listed_and_exported(native):
    kept.symbols(SYMBOLS)


def test_renderer_has_the_calls(native):
    kept.wrappers(SYMBOLS + ("rtiow_denoise_variance", "rtiow_denoise_history"), MEMBERS)


def test_null_handle_needs_no_gpu(native):
    kept.null_handles(SYMBOLS)


def test_noise_kernel_has_no_scratch_and_no_vgpr_spills(native):
    kept.kernels("temporal_noise_kernel<")
