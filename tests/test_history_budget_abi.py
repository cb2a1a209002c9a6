"""History-guided sample budgets (rtiow_history_plan, rtiow_read_history_plan, rtiow_accumulate_budget): the parts that need no GPU.
The checks themselves are the rows of tests/test_abi.py and tests/test_kernel_inventory.py; this module keeps its test ids and runs
its feature's rows through tests/kept_abi_ids.py."""
from tests import kept_abi_ids as kept

SYMBOLS = ("rtiow_history_plan", "rtiow_read_history_plan", "rtiow_accumulate_budget")
MEMBERS = ("history_plan", "history_plan_lengths", "accumulate_budget", "history_update")


def test_budget_symbols_are_declared_listed_and_exported(native):
    kept.symbols(SYMBOLS)


def test_renderer_has_the_budget_interface(native):
    kept.wrappers(SYMBOLS, MEMBERS)


def test_null_handle_needs_no_gpu(native):
    kept.null_handles(SYMBOLS)


def test_budget_kernels_have_no_scratch_and_no_vgpr_spills(native):
    kept.kernels("history_length_kernel<", "budget_select_kernel<")
