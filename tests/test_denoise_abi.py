"""Denoised previews (rtiow_read_linear, rtiow_render_guides, rtiow_denoise, ...): the parts that need no GPU.
The checks themselves are the rows of tests/test_abi.py and tests/test_kernel_inventory.py; this module keeps its test ids and runs
its feature's rows through tests/kept_abi_ids.py."""
from tests import kept_abi_ids as kept

SYMBOLS = ("rtiow_read_linear",
           "rtiow_render_guides",
           "rtiow_read_guides",
           "rtiow_denoise",
           "rtiow_read_denoised",
           "rtiow_denoised_device_ptr")
MEMBERS = ("read_linear", "render_guides", "guides", "denoise", "read_denoised", "denoised_device_ptr")


def test_denoise_symbols_are_declared_listed_and_exported(native):
    kept.symbols(SYMBOLS)


def test_renderer_has_the_denoise_interface(native):
    kept.wrappers(SYMBOLS, MEMBERS)


def test_null_handle_needs_no_gpu(native):
    kept.null_handles(SYMBOLS)


def test_denoise_kernels_have_no_scratch_and_no_vgpr_spills(native):
    kept.kernels("guide_kernel<", "denoise_level_kernel<", "linear_kernel<")
