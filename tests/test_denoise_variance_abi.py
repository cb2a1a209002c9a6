"""Variance-guided denoising (rtiow_read_variance, rtiow_denoise_variance): the parts that need no GPU.
The checks themselves are the rows of tests/test_abi.py and tests/test_kernel_inventory.py; this module keeps its test ids and runs
its feature's rows through tests/kept_abi_ids.py."""
from tests import kept_abi_ids as kept

SYMBOLS = ("rtiow_read_variance", "rtiow_denoise_variance")
MEMBERS = ("variance", "denoise_variance", "accumulate_with_variance")


def test_variance_symbols_are_declared_listed_and_exported(native):
    kept.symbols(SYMBOLS)


def test_renderer_has_the_variance_interface(native):
    kept.wrappers(SYMBOLS, MEMBERS)


def test_null_handle_needs_no_gpu(native):
    kept.null_handles(SYMBOLS)


def test_variance_kernels_have_no_scratch_and_no_vgpr_spills(native):
    kept.kernels("variance_plane_kernel<", "variance_filter_kernel<", "variance_tile_kernel<")
