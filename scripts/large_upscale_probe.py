"""Guided upscaling on large scenes on one GPU: rtiow_upscale_large and rtiow_upscale_wide_large against
their twins on the same handle, by the rule of DESIGN.md section 4.27.

For the jittered-lattice scenes of tests/large_scene.py -- 2 000, 6 000 and 20 000 spheres in fp32, 6 000 in fp64 -- the HIP-event
kernel_ms of the four calls from 1920 x 1080 to 3840 x 2160 (F = 2), source denoised, at the defaults' sigmas, with the share off and on
with the layers of a 2 x 2 lattice, guides and layers current: each the median of --runs after one warm-up.  What is upscaled is one
sample a pixel, the first-hit guides and rtiow_denoise of it, all rendered through the device grid (the bits are the twins').  The twins'
device code is the parent commit's, instruction for instruction (profiles/large_upscale/isa_diff_existing_kernels.txt), so their times
are the parent's times.

The rule (fixed before anything was measured): the feature PAYS if upscale_large and upscale_wide_large are both faster than their twins
on the same handle at every one of these points: share off, and on with G = 2; 6 000 and 20 000 spheres in fp32, 6 000 in fp64.
Reported, not judged: the 2 000-sphere point -- against the LDS grid, where the device grid is expected to lose -- and the ratio of
upscale_large (share off) to render_guides_large of the 3840 x 2160 frame, the same ray once per pixel with no taps.  Each point runs in
a child process under its own `timeout`; the script stops at the first one that fails.  Writes one JSON record (--out).

    python scripts/large_upscale_probe.py [--runs 5] [--out profiles/large_upscale/large_upscale_probe.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTS = [(2000, 32), (6000, 32), (20000, 32), (6000, 64)]
JUDGED = [(6000, 32), (20000, 32), (6000, 64)]
FRAME, FACTOR, BOUNCES, GRID = (1920, 1080), 2, 50, 2
PAIRS = (("upscale", "rtiow_upscale", "rtiow_upscale_large"), ("upscale_wide", "rtiow_upscale_wide", "rtiow_upscale_wide_large"))
SHARES = (("plain", 0), ("share", 1))
CHILD_TIMEOUT_S = 300


def child(n, prec, runs):
    sys.path.insert(0, HERE)
    import raytracingincuda_amd as rt
    from raytracingincuda_amd import api
    from tests import large_scene
    sc = large_scene.lattice(n, prec)
    out = {"spheres": n, "precision": prec, "frame": list(FRAME), "factor": FACTOR, "source": "denoised", "coverage_grid": GRID}
    sigmas = {"rtiow_upscale": (api.UPSCALE_SIGMA_NORMAL, api.UPSCALE_SIGMA_ALBEDO, api.UPSCALE_SIGMA_DEPTH),
              "rtiow_upscale_wide": (api.UPSCALE_WIDE_SIGMA_NORMAL, api.UPSCALE_WIDE_SIGMA_ALBEDO, api.UPSCALE_WIDE_SIGMA_DEPTH)}

    def median(call):
        call()                                                       # warm-up: tables, buffers, kernels
        ms = [call() for _ in range(runs)]
        return {"ms": ms, "median_ms": statistics.median(ms)}

    with rt.Renderer(0, prec) as r:
        r.set_camera(rt.camera(prec, FRAME[0], FRAME[1], 1, BOUNCES))
        r.set_scene(sc)
        r.init_rng(1227)
        r.accumulate_large(1); r.render_guides_large(); r.render_coverage_large(GRID)
        r.denoise()

        def upscale(symbol, twin, flag):
            def run():
                ms, covered = ctypes.c_float(0), ctypes.c_uint64(0)
                r._check(getattr(r._lib, symbol)(r._h, FACTOR, api.UPSCALE_DENOISED, *sigmas[twin], flag, ctypes.byref(ms), ctypes.byref(covered)))
                return ms.value
            return run

        for name, twin, large in PAIRS:
            for share, flag in SHARES:
                rec = {"twin": median(upscale(twin, twin, flag)), "large": median(upscale(large, twin, flag))}
                rec["ratio_large_over_twin"] = rec["large"]["median_ms"] / rec["twin"]["median_ms"]
                out["%s_%s" % (name, share)] = rec
        out["scene_source_after"] = r.stats()["scene_source"]
        out["grid"] = r.large_grid()
        # the same ray, once per pixel of the 3840 x 2160 frame, with no taps
        r.set_camera(rt.camera(prec, FACTOR * FRAME[0], FACTOR * FRAME[1], 1, BOUNCES))
        out["guides_large_of_the_output_frame"] = median(r.render_guides_large)
        out["ratio_upscale_large_over_guides_large"] = out["upscale_plain"]["large"]["median_ms"] / out["guides_large_of_the_output_frame"]["median_ms"]
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "large_upscale", "large_upscale_probe.json"))
    ap.add_argument("--child", nargs=2, type=int)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.runs)
    if a.runs < 5:
        ap.error("the rule asks for the median of at least five runs")
    keys = ["%s_%s" % (name, share) for name, _, _ in PAIRS for share, _ in SHARES]
    points = []
    for n, prec in POINTS:
        r = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--runs", str(a.runs), "--child", str(n), str(prec)],
                           capture_output=True, text=True)
        if r.returncode != 0:
            print("point (%d spheres, fp%d) failed with status %d: stopping\n%s" % (n, prec, r.returncode, r.stderr[-2000:]), file=sys.stderr)
            return 1
        p = json.loads(r.stdout.strip().splitlines()[-1])
        points.append(p)
        print("%6d spheres fp%d: " % (n, prec) + "; ".join("%s %.3f -> %.3f ms (x %.4f)" % (
            k, p[k]["twin"]["median_ms"], p[k]["large"]["median_ms"], p[k]["ratio_large_over_twin"]) for k in keys)
            + "; upscale_large / guides_large of the output frame %.3f" % p["ratio_upscale_large_over_guides_large"], flush=True)
    judged = [p for p in points if (p["spheres"], p["precision"]) in JUDGED]
    pays = len(judged) == len(JUDGED) and all(p[k]["large"]["median_ms"] < p[k]["twin"]["median_ms"] for p in judged for k in keys)
    record = {"rule": "pays if upscale_large and upscale_wide_large are both faster than their twins on the same handle, 1920x1080 -> 3840x2160, source "
                      "denoised, share off and on with G = 2, at 6 000 and 20 000 lattice spheres in fp32 and at 6 000 in fp64; the 2 000-sphere point and "
                      "the ratio of upscale_large to render_guides_large of the 3840x2160 frame are reported, not judged",
              "runs": a.runs, "points": points, "pays": pays}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("the feature %s" % ("pays" if pays else "does NOT pay yet"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
