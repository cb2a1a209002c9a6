"""The kernels behind the progressive-preview calls, from the compiler's own metadata and listing (no GPU needed: hipcc cross-compiles
gfx950 here): how many instantiations each has, that none uses scratch or spills a VGPR, and the few facts about their code the
documents quote.  One table; a new kernel adds one row.  The render kernels' budgets proper: tests/test_kernel_resources.py."""
import functools
import re

import pytest

DWORDX4, DWORD = r"\bglobal_load_dwordx4\b", r"\bglobal_load_dword\b"
LDS_READ, BARRIER = r"\bds_(?:read|load)_\w+", r"\bs_barrier\b"
MANY = 10 ** 9

# counting substring of the demangled name -> (instantiations, SGPR spills allowed, listing facts)
# a listing fact: (which instantiations: what follows the substring, "" for all; instruction pattern; fewest; most)
KERNELS = {
    "render_accumulate_kernel<": (6, None, ()),                # the budgets: test_progressive_render_kernels_meet_the_main_launch_register_budget
    "render_adaptive_kernel<": (6, None, ()),
    "adaptive_select_kernel<": (2, 0, ()),
    "adaptive_finish_kernel<": (2, 0, ()),
    # guide_kernel and guide_chain_kernel: fp32 / fp64 x LDS / scalar scene source; everything below: fp32 / fp64
    "guide_kernel<": (4, None, ()),
    "guide_chain_kernel<": (4, None, ()),
    "denoise_level_kernel<": (2, None, ()),
    "linear_kernel<": (2, None, ()),
    "variance_plane_kernel<": (2, None, ()),
    "variance_filter_kernel<": (2, None, ()),
    "variance_tile_kernel<": (2, None, ()),
    # fp32: every tap is two 16-byte vector loads -- the four taps' eight plus the pixel's own guides
    "history_reproject_kernel<": (2, None, (("float>", DWORDX4, 9, MANY),)),
    # fp32: per tap {N', depth'} is one 16-byte vector load and M one dword -- the plan moves less than the update: at most the four
    # taps' four plus the pixel's own guides
    "history_length_kernel<": (2, None, (("float>", DWORDX4, 1, 5), ("float>", DWORD, 1, MANY))),
    "budget_select_kernel<": (2, None, ()),
    # fp32: the gather is the plain update's, and the window comes from LDS
    "history_clip_kernel<": (2, None, (("float>", DWORDX4, 9, MANY), ("float>", LDS_READ, 1, MANY))),
    "temporal_noise_kernel<": (2, None, (("", LDS_READ, 1, MANY),)),                               # the window comes from LDS
    "feedback_filter_kernel<": (2, None, (("", LDS_READ, 1, MANY), ("", BARRIER, 1, 1))),           # taps from LDS; the tile is staged once
}
# name families other tests count by ("render_": tests/test_kernel_resources.py): a row outside a family matches no kernel of it
FAMILIES = ("render_", "variance_")


@functools.lru_cache(maxsize=None)
def _metadata():
    from raytracingincuda_amd.kernel_metadata import device_metadata
    return device_metadata()


def _one(meta, part):
    hits = [k for k in meta if part in k]
    assert len(hits) == 1, (part, hits)
    return meta[hits[0]]


def check_disjoint():
    meta, _ = _metadata()
    for k in meta:
        rows = [name for name in KERNELS if name in k]
        assert len(rows) <= 1, (k, rows)
        for name in rows:
            for family in FAMILIES:
                assert name.startswith(family) or family not in k, (k, name, family)


def check_row(name):
    meta, listing = _metadata()
    count, sgpr_spills, facts = KERNELS[name]
    ks = {k: v for k, v in meta.items() if name in k}
    assert len(ks) == count, (name, sorted(ks))
    for k, v in ks.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)
        if sgpr_spills is not None:
            assert v["sgpr_spill"] <= sgpr_spills, (k, v)
        body = listing[listing.index("\n%s:" % v["symbol"]):]
        body = body[:body.index(".Lfunc_end")]
        for which, pattern, fewest, most in facts:
            if name + which in k:
                found = len(re.findall(pattern, body))
                assert fewest <= found <= most, (k, pattern, found, re.findall(r"\b(?:global_load|ds)_\w+", body))


def check_budget(kernel):
    meta, _ = _metadata()
    render = {k: v for k, v in meta.items() if kernel + "<" in k}
    # the six instantiations: fp32 / fp64 x LDS (the screened / grid sources run this one too) / scalar, plus the fp32 bounded loop
    for prec, src, bound in (("float", 0, "false"), ("float", 1, "false"), ("float", 0, "true"), ("float", 1, "true"),
                             ("double", 0, "false"), ("double", 1, "false")):
        assert [k for k in render if "%s<%s, %d, %s>" % (kernel, prec, src, bound) in k], (prec, src, bound)
    assert len(render) == 6, sorted(render)
    for k, v in render.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)
        if "<float" in k:
            assert v["vgpr"] <= 96, (k, v)        # five waves per SIMD
        else:
            assert v["vgpr"] <= 128, (k, v)       # four waves per SIMD
        prec, src = re.search(kernel + r"<(\w+), (\d)", k).groups()
        plain = _one(meta, "render_persistent_kernel<%s, %s, false, false>" % (prec, src))
        assert v["sgpr_spill"] <= plain["sgpr_spill"], (k, v, plain)


def test_counting_substrings_are_disjoint(native):
    check_disjoint()


@pytest.mark.parametrize("name", KERNELS)
def test_kernel_count_resources_and_listing(native, name):
    check_row(name)


@pytest.mark.parametrize("kernel", ["render_accumulate_kernel", "render_adaptive_kernel"])
def test_progressive_render_kernels_meet_the_main_launch_register_budget(native, kernel):
    check_budget(kernel)
