"""A session on a volume scene on one GPU: each _volume call against its _large twin on the same handle, by
the rule of DESIGN.md section 4.29.

For the jittered cubes of tests/volume_scene.py -- 18^3, 27^3 and 46^3 spheres in fp32, 18^3 in fp64 -- at 1920 x 1080 and 50 bounces,
the HIP-event kernel time the call returns of
    a 16-sample chunk                             accumulate_volume(16)                 against accumulate_large(16)
    a 4-sample adaptive chunk, everybody active   accumulate_adaptive_volume(4, ...)    against accumulate_adaptive_large(4, ...)
    the first-hit guides                          render_guides_volume()                against render_guides_large()
    the coverage layers, 2 x 2 sub-samples        render_coverage_volume(2)             against render_coverage_large(2)
    upscale and upscale_wide at F = 2, denoised   rtiow_upscale(_wide)_volume           against rtiow_upscale(_wide)_large
each the median of --runs after one warm-up, every chunk the first after a reset (tile order, from the states of init_rng), with the
launch's stamped shader clock (rtiow_stats.main_clock_mhz) beside each chunk's time (the tile kernels stamp none).  The upscalers find
guides that are current, so their time is the upscale kernel's alone.  The _large twins are the fastest way there was before these calls,
and their device code is the parent commit's, instruction for instruction (profiles/volume_preview/isa_diff_existing_kernels.txt).

The rule (fixed before anything was measured): the feature PAYS if every _volume time is below its _large twin's on every one of the
four cubes.  Reported, not judged: the plain twins by the exact loop (one run after a warm-up, at 18^3 and on the flat lattice only: a
chunk through the exact loop over 97 336 spheres takes minutes), the flat lattice of 6 000 -- where the volume grid is expected to lose
--, the Gaussian cloud, and the ratio of a 16-sample volume chunk to render_volume() at 16 samples.  Each point runs in a child process
under its own `timeout`; the script stops at the first one that fails.  Writes one JSON record (--out).

    python scripts/volume_preview_probe.py [--runs 5] [--out profiles/volume_preview/volume_preview_probe.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTS = [("cube18", 32), ("cube27", 32), ("cube46", 32), ("cube18", 64), ("flat6000", 32), ("gauss", 32)]
JUDGED = [("cube18", 32), ("cube27", 32), ("cube46", 32), ("cube18", 64)]
PLAIN = [("cube18", 32), ("cube18", 64), ("flat6000", 32)]
FRAME = (1920, 1080)
CHUNK, ADAPTIVE_CHUNK, BOUNCES, FACTOR = 16, 4, 50, 2
EVERYBODY = 2 ** 31 - 1
PAIRS = ("chunk16", "adaptive4", "guides", "coverage2", "upscale2", "upscale_wide2")
CHILD_TIMEOUT_S = 280


def scene_of(name, prec):
    from tests import volume_scene
    if name.startswith("cube"):
        return volume_scene.cube(int(name[4:]), prec)
    return volume_scene.flat(prec, 6000) if name == "flat6000" else volume_scene.gauss_cloud(prec)


def child(name, prec, runs):
    sys.path.insert(0, HERE)
    import raytracingincuda_amd as rt
    sc = scene_of(name, prec)
    out = {"scene": name, "spheres": int(len(sc["type"])), "precision": prec, "frame": list(FRAME), "bounces": BOUNCES}
    with rt.Renderer(0, prec) as r:
        r.set_camera(rt.camera(prec, FRAME[0], FRAME[1], CHUNK, BOUNCES))
        r.set_scene(sc)
        r.init_rng(1227)

        def fresh(call):
            def run():
                r.reset_accumulation(); r.init_rng(1227)
                return call()
            return run

        def measure(call, stamped, n=runs):
            call()                                                   # warm-up: tables, buffers, kernels
            ms, clocks = [], []
            for _ in range(n):
                ms.append(call())
                st = r.stats()
                clocks.append(st["main_clock_mhz"] if stamped else None)
            rec = {"ms": ms, "median_ms": statistics.median(ms), "clock_mhz": clocks}
            if stamped:                                              # rtiow_stats describes the last chunk or render, not a tile kernel
                rec.update(scene_source=st["scene_source"], vgprs=st["vgprs"], lds_bytes=st["lds_bytes"])
            return rec

        def upscaler(symbol):
            """The C call itself: the Python method returns the count, not the time.  The share is off and the guides are current."""
            sig = {"rtiow_upscale": (rt.api.UPSCALE_SIGMA_NORMAL, rt.api.UPSCALE_SIGMA_ALBEDO, rt.api.UPSCALE_SIGMA_DEPTH),
                   "rtiow_upscale_wide": (rt.api.UPSCALE_WIDE_SIGMA_NORMAL, rt.api.UPSCALE_WIDE_SIGMA_ALBEDO, rt.api.UPSCALE_WIDE_SIGMA_DEPTH)}[symbol.replace("_volume", "").replace("_large", "")]
            def run():
                ms, n = ctypes.c_float(0), ctypes.c_uint64(0)
                r._check(getattr(r._lib, symbol)(r._h, FACTOR, rt.api.UPSCALE_DENOISED, *sig, 0, ctypes.byref(ms), ctypes.byref(n)))
                return ms.value
            return run

        adaptive = dict(min_samples=EVERYBODY, max_samples=EVERYBODY)
        calls = {   # name -> (volume, large, plain, stamped)
            "chunk16": (fresh(lambda: r.accumulate_volume(CHUNK)), fresh(lambda: r.accumulate_large(CHUNK)), fresh(lambda: r.accumulate(CHUNK)), True),
            "adaptive4": (fresh(lambda: r.accumulate_adaptive_volume(ADAPTIVE_CHUNK, 0.0, **adaptive)[0]),
                          fresh(lambda: r.accumulate_adaptive_large(ADAPTIVE_CHUNK, 0.0, **adaptive)[0]),
                          fresh(lambda: r.accumulate_adaptive(ADAPTIVE_CHUNK, 0.0, **adaptive)[0]), True),
            "guides": (r.render_guides_volume, r.render_guides_large, r.render_guides, False),
            "coverage2": (lambda: r.render_coverage_volume(2), lambda: r.render_coverage_large(2), lambda: r.render_coverage(2), False),
            "upscale2": (upscaler("rtiow_upscale_volume"), upscaler("rtiow_upscale_large"), upscaler("rtiow_upscale"), False),
            "upscale_wide2": (upscaler("rtiow_upscale_wide_volume"), upscaler("rtiow_upscale_wide_large"), upscaler("rtiow_upscale_wide"), False),
        }
        plain_too = (name, prec) in PLAIN
        for pair in PAIRS:
            if pair == "upscale2":                                   # the upscalers' source: a filtered image of one volume chunk, guides current
                r.reset_accumulation(); r.init_rng(1227)
                r.accumulate_volume(1); r.render_guides_volume(); r.denoise()
            volume, large, plain, stamped = calls[pair]
            out[pair] = {"large": measure(large, stamped), "volume": measure(volume, stamped)}
            out[pair]["ratio_volume_over_large"] = out[pair]["volume"]["median_ms"] / out[pair]["large"]["median_ms"]
            if plain_too:
                out[pair]["plain"] = measure(plain, stamped, 1)
        out["render_volume16"] = measure(lambda: (r.init_rng(1227), r.render_volume())[1], True)
        out["ratio_chunk16_over_render_volume16"] = out["chunk16"]["volume"]["median_ms"] / out["render_volume16"]["median_ms"]
        out["volume_grid"], out["large_grid"] = r.volume_grid(), r.large_grid()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "volume_preview", "volume_preview_probe.json"))
    ap.add_argument("--child", nargs=2)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], int(a.child[1]), a.runs)
    if a.runs < 5:
        ap.error("the rule asks for the median of at least five runs")
    points = []
    for name, prec in POINTS:
        r = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--runs", str(a.runs), "--child", name, str(prec)],
                           capture_output=True, text=True)
        if r.returncode != 0:
            print("point (%s, fp%d) failed with status %d: stopping\n%s" % (name, prec, r.returncode, r.stderr[-2000:]), file=sys.stderr)
            return 1
        p = json.loads(r.stdout.strip().splitlines()[-1])
        points.append(p)
        print("%9s fp%d: " % (name, prec) + "; ".join("%s %.2f -> %.2f ms (x %.3f)" % (
            k, p[k]["large"]["median_ms"], p[k]["volume"]["median_ms"], p[k]["ratio_volume_over_large"]) for k in PAIRS)
            + "; chunk16 / render_volume16 %.3f" % p["ratio_chunk16_over_render_volume16"], flush=True)
    judged = [p for p in points if (p["scene"], p["precision"]) in JUDGED]
    verdict = {k: all(p[k]["volume"]["median_ms"] < p[k]["large"]["median_ms"] for p in judged) for k in PAIRS}
    pays = len(judged) == len(JUDGED) and all(verdict.values())
    record = {"rule": "pays if a 16-sample chunk, a 4-sample adaptive chunk with everybody active, the first-hit guides, the coverage layers at 2 x 2 "
                      "and both upscalers at F = 2 from the denoised image are all faster through the volume grid than through their _large twins on "
                      "the same handle, on the cubes of 18^3, 27^3 and 46^3 spheres in fp32 and of 18^3 in fp64; the plain twins, the flat lattice, "
                      "the Gaussian cloud and the ratio of a 16-sample volume chunk to render_volume at 16 samples are reported, not judged",
              "runs": a.runs, "points": points, "pays_by_call": verdict, "pays": pays}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("the feature %s" % ("pays" if pays else "does NOT pay yet: " + ", ".join(k for k in PAIRS if not verdict[k])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
