"""Edit influence (rtiow_set_edit_influence, rtiow_read_edit_influence, edit_influence_kernel): the parts that need no GPU.  The rows of
this feature live here, not in tests/abi_table.py and tests/test_kernel_inventory.py; the checks are tests/test_abi.py's check_* functions
wherever those take their row as arguments, and the two that read tests/abi_table.py (arity, NULL handle) are restated over the table
below.  The policy's share is tests/native/edit_influence_state_main.cpp and the edit list's tests/native/edit_list_main.cpp, stand-alone
programs over csrc/library/preview_state.h and csrc/library/edit_list.h alone, built here with AddressSanitizer + UBSan and run directly."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import edit_influence_model as E
from tests import preview_refusals as table
from tests import test_abi as abi
from tests.conftest import ROOT

# symbol -> (number of parameters, the arguments of a call with a NULL handle: it answers -1 before any device work)
SYMBOLS = {"rtiow_set_edit_influence": (2, (None, 0.5)), "rtiow_read_edit_influence": (3, (None, None, 0))}
METHODS = {"set_edit_influence": ("kappa",), "edit_influence": ()}
# counting substring of the demangled name -> instantiations: fp32 / fp64
KERNELS = {"edit_influence_kernel<": 2}
FROZEN_NAMES = ("render_", "variance_", "guide_kernel<", "guide_chain_kernel<", "history_reproject_kernel<", "history_length_kernel<", "history_clip_kernel<",
                "surface_motion_kernel<", "motion_reproject_kernel<", "motion_length_kernel<", "motion_clip_kernel<")
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


def test_wrapper_default_is_a_kappa_the_call_accepts(native):
    from raytracingincuda_amd import api
    abi.check_default("set_edit_influence", "kappa", "EDIT_INFLUENCE_KAPPA")
    assert api.EDIT_INFLUENCE_KAPPA > 0                      # the wrapper called without an argument turns the knob on


@pytest.mark.parametrize("name", KERNELS)
def test_kernel_count_and_resources(native, name):
    from raytracingincuda_amd.kernel_metadata import device_metadata
    meta, _ = device_metadata()
    ks = {k: v for k, v in meta.items() if name in k}
    assert len(ks) == KERNELS[name], (name, sorted(ks))
    for k, v in ks.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, (k, v)
        for frozen in FROZEN_NAMES:
            assert frozen not in k, (k, frozen)              # the names other tests count by
    for prec in ("float", "double"):
        assert [k for k in ks if "%s%s>" % (name, prec) in k], prec
    from tests import test_kernel_inventory as inventory
    assert not [row for row in inventory.KERNELS for k in ks if row in k]
    for family in inventory.FAMILIES:
        assert not [k for k in ks if family in k], family
    inventory.check_disjoint()
    # the three motion kernels gained one multiply: still no scratch and no spills
    for row in ("motion_reproject_kernel<", "motion_length_kernel<", "motion_clip_kernel<"):
        for k, v in meta.items():
            if row in k:
                assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)


def test_the_models_chunk_is_the_headers():
    text = open(os.path.join(LIBRARY, "edit_list.h")).read()
    assert int(re.search(r"constexpr int EDIT_LIST_CHUNK = (\d+);", text).group(1)) == E.CHUNK
    assert "CHUNK = %d" % E.CHUNK in E.__doc__


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


# ---- the policy: what rtiow_read_edit_influence answers in every state of tests/preview_refusals.py, and in edited ones
NOT_IN_EFFECT = "rtiow_read_edit_influence: motion is not in effect (rtiow_edit_scene on a handle with a history base)"
OFF = "rtiow_read_edit_influence: edit influence is off (rtiow_set_edit_influence with kappa > 0)"
STALE = "rtiow_read_edit_influence: no influence plane for the current scene, camera and shard (rtiow_render_guides)"
_EDITED = table.STATES["committed"] + ("edit",)
EDITED_STATES = {
    "edited": (_EDITED, (table.E_STATE, OFF)),
    "edited_guides": (_EDITED + ("guides",), (table.E_STATE, OFF)),
    "edited_on": (_EDITED + ("kappa_on",), (table.E_STATE, STALE)),
    "on_edited": (("kappa_on",) + _EDITED, (table.E_STATE, STALE)),
    "edited_on_guides": (_EDITED + ("kappa_on", "guides"), (0, "")),
    "edited_on_planned": (_EDITED + ("kappa_on", "rng", "plan"), (0, "")),
    "edited_on_updated": (_EDITED + ("kappa_on", "rng", "plain", "update"), (0, "")),
    "edited_guides_on": (_EDITED + ("guides", "kappa_on"), (table.E_STATE, STALE)),
    "edited_on_guides_off": (_EDITED + ("kappa_on", "guides", "kappa_off"), (table.E_STATE, OFF)),
    "edited_on_guides_same": (_EDITED + ("kappa_on", "guides", "kappa_on"), (0, "")),
    "edited_on_guides_moved": (_EDITED + ("kappa_on", "guides", "move"), (table.E_STATE, STALE)),
    "edited_on_guides_edited": (_EDITED + ("kappa_on", "guides", "edit"), (table.E_STATE, STALE)),
    "edited_on_committed": (_EDITED + ("kappa_on", "rng", "plain", "update", "commit"), (table.E_STATE, NOT_IN_EFFECT)),
    "uncommitted_edit_on_guides": (table.STATES["updated"] + ("edit", "kappa_on", "guides"), (table.E_STATE, NOT_IN_EFFECT)),
    "sharded_edit_on_guides": (table.STATES["sharded_chunk"] + ("edit", "kappa_on", "guides"), (table.E_STATE, NOT_IN_EFFECT)),
}


def test_edit_influence_state_under_asan_ubsan(tmp_path):
    exe = _build(tmp_path, "edit_influence_state_main")
    names = list(table.STATES) + ["on:" + s for s in table.STATES] + list(EDITED_STATES)
    steps = [table.STATES[s] for s in table.STATES] + [table.STATES[s] + ("kappa_on", "guides") for s in table.STATES] + [EDITED_STATES[s][0] for s in EDITED_STATES]
    # no state of the table has edited: motion is not in effect, with the knob on or off
    want = [(table.E_STATE, NOT_IN_EFFECT)] * (2 * len(table.STATES)) + [EDITED_STATES[s][1] for s in EDITED_STATES]
    out = _run(exe, "".join(" ".join(s) + " \n" if s else "kappa_off\n" for s in steps))
    assert out[-1] == "0 edit-influence rule failure(s)", out
    assert not [l for l in out if l.startswith("RULE BROKEN")], out
    answers = out[-1 - len(names):-1]
    for name, line, (code, text) in zip(names, answers, want):
        assert line == "%d | %s" % (code, text), (name, line)


# ---- the edit list: the stand-alone program against the model
def _hex(a):
    a = np.ascontiguousarray(a)
    return ["%x" % int(w) for w in a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64).ravel()]


def _tables(dt, cr, af, ri, ty):
    return {"cr": np.array(cr, dt).reshape(-1, 4), "af": np.array(af, dt).reshape(-1, 4), "ri": np.array(ri, dt), "ty": np.array(ty, np.int32)}


def _program_input(cur, snap):
    dt = cur["cr"].dtype
    lines = ["%d %d" % (dt.itemsize, len(cur["ty"]))]
    for k in range(len(cur["ty"])):
        for t in (cur, snap):
            lines.append(" ".join(_hex(t["cr"][k]) + ["%x" % (int(t["ty"][k]) & 0xffffffff)] + _hex(t["af"][k]) + _hex(t["ri"][k:k + 1])))
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_edit_list_under_asan_ubsan_against_the_model(native, tmp_path, dt):
    from tests.conftest import compact
    exe = _build(tmp_path, "edit_list_main")
    n = 6
    cr = [[k, 0.5, -k, 0.5 + k] for k in range(n)]
    af = [[0.1 * k, 0.2, 0.3, 0.0] for k in range(n)]
    ri, ty = [1.5] * n, [0, 1, 2, 0, 1, 2]
    snap = _tables(dt, cr, af, ri, ty)
    cases = {"none": _tables(dt, cr, af, ri, ty)}
    moved = _tables(dt, cr, af, ri, ty)
    moved["cr"][1, 0] += 0.25                                # moved only: a centre ...
    moved["cr"][4, 3] *= 1.5                                 # ... and a radius
    cases["moved only"] = moved
    changed = _tables(dt, cr, af, ri, ty)
    changed["af"][0, 2] = 0.75
    changed["ri"][2] = 1.25
    changed["ty"][5] = 0
    cases["changed only"] = changed
    both = _tables(dt, cr, af, ri, ty)
    both["cr"][3, 1] = -0.0 + 0.5 * 3                        # sphere 3: moved and changed
    both["af"][3, 3] = 0.5
    both["cr"][0, 2] = -0.0                                  # sphere 0: -0 for 0 is a move, bits against bits
    both["ty"][5] = 1                                        # sphere 5: changed only
    cases["both"] = both
    for name, cur in cases.items():
        out = _run(exe, _program_input(cur, snap))
        entries, owners = E.edit_list(cur, snap)
        from tests import scene_motion_model as M
        assert out[0] == "flags " + " ".join(str(int(f)) for f in M.flags(cur, snap)), name
        assert out[-1] == "entries %d" % len(owners), name
        want = ["%d %s" % (o, " ".join(_hex(e))) for e, o in zip(entries, owners)]
        assert out[1:-1] == want, (name, out, want)
    assert len(E.edit_list(cases["none"], snap)[1]) == 0 and E.edit_list(cases["moved only"], snap)[1].tolist() == [1, 1, 4, 4]
    assert E.edit_list(cases["changed only"], snap)[1].tolist() == [0, 2, 5] and E.edit_list(cases["both"], snap)[1].tolist() == [0, 0, 3, 3, 5]
    # invalid slots dropped: the tables of a scene with a `valid` pattern are numbered by kept sphere, as the library numbers them
    from tests import scene_motion_model as M
    rt = native
    prec = 32 if dt == np.float32 else 64
    scene = rt.build_scene(3, prec)
    if scene.get("valid") is None or (np.asarray(scene["valid"]) != 0).all():
        valid = np.ones(len(scene["type"]), np.int32)
        valid[[1, 5, 6]] = 0
        scene = dict(scene, valid=valid)
    kept = [int(s) for s in M.kept_slots(scene)]
    edit = M.recolour(M.translate(scene, [kept[2], kept[7]], (0.5, 0.0, 0.25)), [kept[7], kept[9]])
    cur, snap = M.tables(edit, prec), M.tables(scene, prec)
    assert len(cur["ty"]) == len(kept) < len(scene["type"])
    out = _run(exe, _program_input(cur, snap))
    entries, owners = E.edit_list(cur, snap)
    assert owners.tolist() == [2, 2, 7, 7, 9]
    assert out[1:-1] == ["%d %s" % (o, " ".join(_hex(e))) for e, o in zip(entries, owners)] and out[-1] == "entries 5"
    assert compact(scene)["type"].shape[0] == len(kept)
