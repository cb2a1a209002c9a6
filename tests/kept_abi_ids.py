"""For the per-feature modules tests/test_*_abi.py only.  Their checks now live, one case per row, in tests/test_abi.py and
tests/test_kernel_inventory.py; the modules keep their test ids and run, through the functions here, the rows of their feature with
the very check_* functions of those two modules.  Nothing new belongs here or there: a new call adds rows to tests/abi_table.py and
the inventory, and these modules go, with this file, as their ids are retired."""
from tests import abi_table as T
from tests import test_abi as abi
from tests import test_kernel_inventory as inventory


def symbols(names):
    for s in names:
        abi.check_symbol(s)
    abi.check_abi_version()


def null_handles(names):
    for s in names:
        abi.check_null_handle(s)


def wrappers(names, members, constants=()):
    """names: the symbols whose number of parameters the module pinned; members: the Renderer members; constants: api constants it pinned
    besides the defaults of those members."""
    for s in names:
        abi.check_arity(s)
    for m in members:
        abi.check_member(m)
    defaults = [d for d in T.DEFAULTS if d[0] in members]
    for d in defaults:
        abi.check_default(*d)
    for c in sorted(set(constants) | {d[2] for d in defaults if d[2] in T.RANGES}):
        abi.check_range(c)
    for s in T.SAME_AS:
        if s[0] in members:
            abi.check_same_as(*s)
    abi.check_abi_version()


def kernels(*own):
    """The module's own rows first, so a failure names them; then, as the modules did by hand-copied lists, that nothing else was
    instantiated or renamed: every row, and the counting substrings disjoint."""
    for name in own + tuple(inventory.KERNELS):
        inventory.check_row(name)
    inventory.check_disjoint()
