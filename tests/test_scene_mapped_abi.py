"""Scene edits that add and remove spheres (rtiow_edit_scene_mapped, rtiow_read_scene_origin): the parts that
need no GPU.  The rows of this feature live here, not in tests/abi_table.py; the checks are tests/test_abi.py's check_* functions wherever
those take their row as arguments, and the two that read tests/abi_table.py (arity, NULL handle) are restated over the table below.  The
feature adds no kernel and changes none: the kernel set of the code object is held to the names and counts it had.  The plain-C++ parts
are tests/native/scene_mapped_list_main.cpp (csrc/library/edit_list.h against tests/scene_mapped_model.py) and
tests/native/scene_mapped_state_main.cpp (csrc/library/preview_state.h), stand-alone programs built here with AddressSanitizer + UBSan
and run directly."""
import collections
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import edit_influence_model as E
from tests import scene_mapped_model as S
from tests import scene_motion_model as M
from tests import test_abi as abi
from tests.conftest import ROOT

# symbol -> (number of parameters, the arguments of a call with a NULL handle: it answers -1 before any device work)
SYMBOLS = {"rtiow_edit_scene_mapped": (8, (None, 3, None, None, None, None, None, None)), "rtiow_read_scene_origin": (3, (None, None, 0))}
METHODS = {"edit_scene_mapped": ("scene", "origin"), "scene_origin": ()}
# every kernel name of the code object with its instantiations, as they were before this feature ("": the seven plain functions)
KERNEL_SET = {
    "render_persistent_kernel": 12, "render_prepass_kernel": 12, "render_kernel": 8, "render_solo_kernel": 4, "place_pixels_kernel": 2,
    "render_accumulate_kernel": 6, "render_adaptive_kernel": 6, "budget_select_kernel": 2, "adaptive_select_kernel": 2, "adaptive_finish_kernel": 2,
    "guide_kernel": 4, "guide_lens_kernel": 4, "guide_chain_kernel": 4, "surface_motion_kernel": 4, "edit_influence_kernel": 2, "linear_kernel": 2,
    "denoise_level_kernel": 2, "variance_plane_kernel": 2, "temporal_noise_kernel": 2, "variance_tile_kernel": 2, "variance_filter_kernel": 2,
    "motion_clip_kernel": 2, "motion_reproject_kernel": 2, "history_clip_kernel": 2, "history_reproject_kernel": 2, "motion_length_kernel": 2,
    "history_length_kernel": 2, "feedback_filter_kernel": 2, "coverage_kernel": 4, "edge_resolve_kernel": 2, "quantise_kernel": 2,
}
PLAIN_KERNELS = 7
LIBRARY = os.path.join(ROOT, "raytracingincuda_amd", "csrc", "library")


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_symbol_is_declared_listed_and_exported(native, symbol):
    abi.check_symbol(symbol)
    abi.check_abi_version()                                  # functions were added, no struct moved: still 6


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_declaration_has_the_headers_arity(native, symbol):
    from raytracingincuda_amd import api
    argtypes = getattr(api.load_hip_library(), symbol).argtypes
    assert argtypes is not None and len(argtypes) == SYMBOLS[symbol][0] == len(SYMBOLS[symbol][1]), symbol
    declared = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % symbol, abi._sources()[0]).group(1)
    assert len(declared.split(",")) == SYMBOLS[symbol][0], (symbol, declared)


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_null_handle_needs_no_gpu(native, symbol):
    from raytracingincuda_amd import api
    assert getattr(api.load_hip_library(), symbol)(*SYMBOLS[symbol][1]) == -1, symbol


@pytest.mark.parametrize("member", METHODS)
def test_renderer_has_the_member(native, member):
    from raytracingincuda_amd import api
    assert callable(getattr(api.Renderer, member, None)), member
    assert list(abi._parameters(member)) == ["self"] + list(METHODS[member]), member
    assert list(abi._parameters("edit_scene")) == ["self", "scene"]          # the call it extends keeps its parameters


def test_the_kernel_set_is_what_it_was(native):
    from raytracingincuda_amd.kernel_metadata import device_metadata
    from tests import test_kernel_inventory as inventory
    meta, _ = device_metadata()
    names = collections.Counter(re.sub(r"^void ", "", k).replace("(anonymous namespace)::", "", 1).split("(")[0].split("<")[0] if "<" in k else "" for k in meta)
    assert names.pop("") == PLAIN_KERNELS
    assert dict(names) == KERNEL_SET, (sorted(set(names) - set(KERNEL_SET)), sorted(set(KERNEL_SET) - set(names)))
    for row in inventory.KERNELS:                                # every frozen name keeps the count the inventory gives it
        assert len([k for k in meta if row in k]) == inventory.KERNELS[row][0] == KERNEL_SET[row[:-1]], row
    inventory.check_disjoint()


def _build(tmp_path, name):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + LIBRARY, "-o", exe, os.path.join(ROOT, "tests", "native", name + ".cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def _run(exe, text):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], input=text, capture_output=True, text=True, env=env)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-1000:])
    return r.stdout.splitlines()


def test_scene_mapped_state_under_asan_ubsan(tmp_path):
    out = _run(_build(tmp_path, "scene_mapped_state_main"), "")
    assert out == ["0 scene-mapped rule failure(s)"], out


# ---- the tables and the list: the stand-alone program against the model
def _hex(a):
    a = np.ascontiguousarray(a)
    return ["%x" % int(w) for w in a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64).ravel()]


def _tables(dt, n, shift=0.0):
    return {"cr": np.array([[k + shift, 0.5, -k, 0.5 + k] for k in range(n)], dt), "af": np.array([[0.1 * k, 0.2, 0.3, 0.0] for k in range(n)], dt),
            "ri": np.full(n, 1.5, dt), "ty": (np.arange(n) % 3).astype(np.int32)}


def _rows(t, idx):
    return {key: np.ascontiguousarray(t[key][np.asarray(idx, np.int64)]) for key in t}


def _records(t):
    return [" ".join(_hex(t["cr"][k]) + ["%x" % (int(t["ty"][k]) & 0xffffffff)] + _hex(t["af"][k]) + _hex(t["ri"][k:k + 1])) for k in range(len(t["ty"]))]


def _program_input(cur, snap, fs, compositions=()):
    lines = ["%d %d %d" % (cur["cr"].dtype.itemsize, len(cur["ty"]), len(snap["ty"])), " ".join(str(int(j)) for j in fs)] + _records(cur) + _records(snap)
    for valid, origin, kept, before in compositions:
        lines += ["compose %d %d" % (len(valid), len(kept))] + [" ".join(str(int(v)) for v in row) for row in (valid, origin, kept, before)]
    return "\n".join(lines) + "\n"


def _expected(cur, snap, fs):
    entries, owners = S.edit_list(cur, snap, fs)
    return (["flags " + " ".join(str(int(f)) for f in S.flags(cur, snap, fs))] + ["snap " + " ".join(_hex(row)) for row in S.snap_table(cur, snap, fs)]
            + ["%d %s" % (o, " ".join(_hex(e))) for e, o in zip(entries, owners)] + ["entries %d" % len(owners)])


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_tables_and_list_under_asan_ubsan_against_the_model(tmp_path, dt):
    exe = _build(tmp_path, "scene_mapped_list_main")
    snap = _tables(dt, 6)
    cases = {}
    # the identity: section 20's list (the program also holds the functions without a map to it)
    cur = _tables(dt, 6)
    cur["cr"][1, 0] += 0.25; cur["af"][3, 2] = 0.75; cur["cr"][4, 3] *= 1.5; cur["ty"][4] = 0
    cases["identity"] = (cur, np.arange(6))
    assert S.edit_list(cur, snap, np.arange(6))[1].tolist() == E.edit_list(cur, snap)[1].tolist() == [1, 1, 3, 4, 4]
    # removed only: spheres 1 and 4 gone, the rest renumbered
    cases["removed"] = (_rows(snap, [0, 2, 3, 5]), np.array([0, 2, 3, 5]))
    # added only, one of them a bit-for-bit twin of a snapshot sphere
    cur = _rows(snap, [0, 1, 2, 3, 4, 5, 2, 0])
    cur["cr"][7] = [7, 7, 7, 0.25]
    cases["added"] = (cur, np.array([0, 1, 2, 3, 4, 5, -1, -1]))
    # a permutation: no flags, no entries
    cases["permuted"] = (_rows(snap, [5, 3, 1, 0, 2, 4]), np.array([5, 3, 1, 0, 2, 4]))
    # everything at once: moved, recoloured, both, removed, added, in another order
    cur = _rows(snap, [4, 0, 0, 5, 2])
    cur["cr"][0, 2] = -0.0 + 1.0; cur["af"][1, 0] = 0.5; cur["cr"][2] = [1, 2, 3, 4]; cur["cr"][3, 3] = 9; cur["ty"][3] = 1
    cases["all"] = (cur, np.array([4, 0, -1, 5, 2]))
    assert S.edit_list(cur, snap, cases["all"][1])[1].tolist() == [0, 0, 1, 2, 3, 3, -2, -2]
    for name, (cur, fs) in cases.items():
        assert _run(exe, _program_input(cur, snap, fs)) == _expected(cur, snap, fs), name
    assert _expected(*cases["permuted"][:1], snap, cases["permuted"][1])[-1] == "entries 0"
    assert _expected(cases["removed"][0], snap, cases["removed"][1])[-3:] == ["-2 " + " ".join(_hex(snap["cr"][1])), "-2 " + " ".join(_hex(snap["cr"][4])), "entries 2"]
    # a list that crosses the kernel's chunk in both passes: 40 spheres, 12 moved (24 entries), 6 added, 10 removed
    big = _tables(dt, 40)
    keep = [k for k in range(40) if k % 4 != 1]
    cur = _rows(big, keep + [0] * 6)
    cur["cr"][:12, 1] += 0.125
    cur["cr"][len(keep):, 0] += 100
    fs = np.array(keep + [-1] * 6)
    entries, owners = S.edit_list(cur, big, fs)
    assert len(owners) == 24 + 6 + 10 > E.CHUNK and (owners[:24] >= 0).all() and (owners[-10:] == -2).all()
    assert _run(exe, _program_input(cur, big, fs)) == _expected(cur, big, fs)
    # the composition, as tests/test_scene_mapped_model.py walks it
    kept0, kept1, kept2 = [1, 1, 0, 1, 1, 1], [1, 1, 1, 0, 1], [1, 1, 1]
    origin1, origin2 = [5, -1, 0, 99, 3], [1, 4, -1]
    fs1 = S.compose(S.identity(5), kept0, kept1, origin1)
    fs2 = S.compose(fs1, kept1, kept2, origin2)
    out = _run(exe, _program_input(cases["identity"][0], snap, np.arange(6), [(kept1, origin1, kept0, S.identity(5)), (kept2, origin2, kept1, fs1)]))
    assert out[-2:] == ["map " + " ".join(str(v) for v in fs1), "map " + " ".join(str(v) for v in fs2)] == ["map 4 -1 0 2", "map -1 2 -1"]


def test_the_models_constants_are_the_headers():
    text = open(os.path.join(LIBRARY, "edit_list.h")).read()
    assert int(re.search(r"EDIT_NO_ORIGIN = (-?\d+)", text).group(1)) == S.NO_ORIGIN
    assert int(re.search(r"EDIT_OWNER_REMOVED = (-?\d+)", text).group(1)) == S.OWNER_REMOVED
    assert M.MOVED == int(re.search(r"EDIT_MOVED = (\d+)", text).group(1)) and M.CHANGED == int(re.search(r"EDIT_CHANGED = (\d+)", text).group(1))
