"""History-guided sample budgets (rtiow_history_plan, rtiow_read_history_plan, rtiow_accumulate_budget), the parts that need no GPU: the
C-ABI is declared, listed and exported, the Python wrapper has it, a NULL handle is refused before device work, the two new kernels have
no scratch and no VGPR spills (compiler metadata; hipcc cross-compiles gfx950), and the view pairs of tests/test_history_budget.py hold
every class of pixel the plan can give (the CPU oracle's guides through the numpy restatement of section 11)."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.preview_drive import BUDGET_PAIRS, CAP_LOW, budget_moves
from tests.preview_model import guides_np, update_np

BUDGET_SYMBOLS = ["rtiow_history_plan", "rtiow_read_history_plan", "rtiow_accumulate_budget"]


def test_budget_symbols_are_declared_listed_and_exported(native):
    from raytracingincuda_amd import api
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtiow.h")).read(), flags=re.S)
    version_script = open(os.path.join(ROOT, "raytracingincuda_amd", "csrc", "librtiow_hip.map")).read()
    globs = re.search(r"global:\s*([^;]*);", version_script).group(1).split()
    paths = native.lib_paths()
    for s in BUDGET_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert any(re.fullmatch(g.replace("*", ".*"), s) for g in globs), s
        assert s in api.HIP_SYMBOLS, s
    for lib in (paths["hip"], paths["hip_debug"]):
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        for s in BUDGET_SYMBOLS:
            assert re.search(r"\bT %s\b" % s, syms), (lib, s)


def test_renderer_has_the_budget_interface(native):
    from raytracingincuda_amd import api
    for m in ("history_plan", "history_plan_lengths", "accumulate_budget"):
        assert callable(getattr(api.Renderer, m, None)), m
    p = inspect.signature(api.Renderer.history_plan).parameters
    u = inspect.signature(api.Renderer.history_update).parameters
    assert list(p) == list(u) == ["self", "depth_tol", "normal_cos", "max_history", "sync"]
    for name in list(u)[1:]:
        assert p[name].default == u[name].default, name             # the plan of the update that follows
    b = inspect.signature(api.Renderer.accumulate_budget).parameters
    assert list(b)[1:] == ["samples", "target", "min_samples", "max_samples", "sync"]
    assert b["samples"].default == api.BUDGET_CHUNK >= 1
    assert b["target"].default == api.BUDGET_TARGET > 0
    assert b["min_samples"].default == api.BUDGET_MIN_SAMPLES >= 0
    lib = native.load_hip_library()
    assert [len(getattr(lib, s).argtypes) for s in BUDGET_SYMBOLS] == [6, 3, 7]
    assert lib.rtiow_abi_version() == native.ABI_VERSION == 6       # functions were added, nothing moved


def test_null_handle_needs_no_gpu(native):
    lib = native.load_hip_library()
    assert lib.rtiow_history_plan(None, 0.1, 0.9, 16.0, None, None) == -1
    assert lib.rtiow_read_history_plan(None, None, 0) == -1
    assert lib.rtiow_accumulate_budget(None, 2, 1, 16.0, 100, None, None) == -1


@pytest.fixture(scope="module")
def metadata(native):
    from raytracingincuda_amd.kernel_metadata import device_metadata
    return device_metadata()


def test_budget_kernels_have_no_scratch_and_no_vgpr_spills(metadata):
    meta, listing = metadata
    for name in ("history_length_kernel<", "budget_select_kernel<"):
        ks = {k: v for k, v in meta.items() if name in k}
        assert len(ks) == 2, (name, sorted(ks))                      # fp32 and fp64
        for k, v in ks.items():
            assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)
            # the names stay apart from the kernels other tests count by substring
            for other in ("render_", "guide_kernel<", "history_reproject_kernel<", "adaptive_select_kernel<", "adaptive_finish_kernel<"):
                assert other not in k, (k, other)
    for name, count in (("history_reproject_kernel<", 2), ("adaptive_select_kernel<", 2), ("adaptive_finish_kernel<", 2)):
        assert len([k for k in meta if name in k]) == count, name
    # fp32: per tap {N', depth'} is one 16-byte vector load and M one dword -- the plan moves less than the update, whose taps are two
    # vector loads each: at most the four taps' four plus the pixel's own guides
    sym = next(v["symbol"] for k, v in meta.items() if "history_length_kernel<float>" in k)
    body = listing[listing.index("\n%s:" % sym):]
    body = body[:body.index(".Lfunc_end")]
    assert 1 <= len(re.findall(r"\bglobal_load_dwordx4\b", body)) <= 5, re.findall(r"\bglobal_load_\w+", body)
    assert len(re.findall(r"\bglobal_load_dword\b", body)) >= 1, re.findall(r"\bglobal_load_\w+", body)


# ---- the classes of pixel in the view pairs of tests/test_history_budget.py

@pytest.mark.parametrize("scene_id", [1, 3])
@pytest.mark.parametrize("size", [(67, 41), (203, 117)])
def test_the_view_pairs_hold_every_class_of_pixel(native, oracle, scene_id, size):
    """The plan's three classes -- m = 0 (no history: disoccluded, or outside the base's frame), 0 < m < cap, m at the cap -- each hold at
    least 1 % of the frame for every (base view, current view) of tests/test_history_budget.py (BUDGET_PAIRS), from the CPU oracle's
    first-hit guides alone.  The GPU tests commit the base after tests/preview_drive.py's adaptive sample(), which leaves every pixel 4 or
    8 samples, so a gathered length is 0 or lies in [4, 8] whatever the mix; here the base is given 4 everywhere and 8 everywhere in
    turn.  The covered pixels are the same in both, so under CAP_LOW = 2.5 every covered pixel is at the cap and under the default cap
    of 16 every covered pixel is below it; the GPU tests use both caps (and CAP_MIX = 6, between the two counts, where all three classes
    share one plan: that mix depends on the noise and is asserted on the GPU).  Counted here, fp32, pixels with m = 0 of W x H:
                         home->orbit  home->dolly  home->roll  orbit->home  roll->home
      scene 1   67 x  41         192          278         217          185         213      of  2747
      scene 3   67 x  41         112          176         129           88         135
      scene 1  203 x 117        1372         2006        1149         1300        1130      of 23751
      scene 3  203 x 117         990         1815        1120          900        1124"""
    from raytracingincuda_amd import api
    W, H = size
    prec, dt = 32, np.float32
    cams = budget_moves(native, prec, W, H)
    rows = np.arange(H)
    guides = {}
    for view in {v for pair in BUDGET_PAIRS for v in pair}:
        normal, _, depth, _ = guides_np(native, oracle, prec, scene_id, cams[view], rows)
        guides[view] = (normal, depth)
    zero = np.zeros((H, W, 3), dt)
    floor = 0.01 * W * H
    for first, then in BUDGET_PAIRS:
        cur = {"c": zero, "n": np.zeros((H, W), np.int32), "N": guides[then][0], "t": guides[then][1]}
        covered = None
        for count in (4, 8):
            base = {"cam": cams[first], "H": zero, "M": np.full((H, W), count, dt), "N": guides[first][0], "z": guides[first][1]}
            for cap in (CAP_LOW, api.HISTORY_MAX):
                _, m, carried = update_np(cams[then], cur, base, api.HISTORY_DEPTH_TOL, api.HISTORY_NORMAL_COS, cap)
                assert carried == int((m > 0).sum())
                if covered is None:
                    covered = m > 0
                    print("scene %d %dx%d %s -> %s: m = 0 in %d" % (scene_id, W, H, first, then, int((~covered).sum())))
                assert np.array_equal(m > 0, covered), (first, then, count, cap)       # coverage is geometry alone
                if cap == CAP_LOW:
                    assert (m[covered] == dt(cap)).all(), (first, then, count)
                else:
                    assert (m[covered] < dt(cap)).all() and (m[covered] >= dt(count) * dt(1 - 1e-6)).all(), (first, then, count)
        assert (~covered).sum() >= floor, (first, then, int((~covered).sum()), floor)  # m = 0
        assert covered.sum() >= floor, (first, then, int(covered.sum()), floor)        # at CAP_LOW: at the cap; at the default cap: below it
