"""The preview chain on large scenes on one GPU: each _large call against its twin on the same handle, by
the rule of DESIGN.md section 4.26.

For the jittered-lattice scenes of tests/large_scene.py -- 2 000, 6 000 and 20 000 spheres in fp32, 6 000 in fp64 -- at 1920 x 1080 and
50 bounces, the HIP-event kernel time of
    a 16-sample chunk                          accumulate_large(16)                  against accumulate(16)
    a 4-sample adaptive chunk, everybody active   accumulate_adaptive_large(4, ...)     against accumulate_adaptive(4, ...)
    the first-hit guides                       render_guides_large()                 against render_guides()
    the coverage layers, 2 x 2 sub-samples     render_coverage_large(2)              against render_coverage(2)
each the median of --runs after one warm-up, every chunk the first after a reset (tile order, from the states of init_rng), with the
launch's stamped shader clock beside each chunk's time (the tile kernels of the guides and the layers stamp none).  The twins' device
code is the parent commit's, instruction for instruction (profiles/large_preview/isa_diff_existing_kernels.txt), so their times are the
parent's times.

The rule (fixed before anything was measured): the feature PAYS if all four _large calls are faster than their twins at 6 000 and at
20 000 spheres in fp32 and at 6 000 in fp64.  Reported, not judged: the 2 000-sphere point -- against the LDS grid, where the device grid
is expected to lose -- and the ratio of a 16-sample large chunk to render_large() at 16 samples.  Each point runs in a child process
under its own `timeout`; the script stops at the first one that fails.  Writes one JSON record (--out).

    python scripts/large_preview_probe.py [--runs 5] [--out profiles/large_preview/large_preview_probe.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTS = [(2000, 32), (6000, 32), (20000, 32), (6000, 64)]
JUDGED = [(6000, 32), (20000, 32), (6000, 64)]
FRAME = (1920, 1080)
CHUNK, ADAPTIVE_CHUNK, BOUNCES = 16, 4, 50
EVERYBODY = 2 ** 31 - 1
PAIRS = ("chunk16", "adaptive4", "guides", "coverage2")
CHILD_TIMEOUT_S = 300


def child(n, prec, runs):
    sys.path.insert(0, HERE)
    import raytracingincuda_amd as rt
    from tests import large_scene
    sc = large_scene.lattice(n, prec)
    out = {"spheres": n, "precision": prec, "frame": list(FRAME), "bounces": BOUNCES}
    with rt.Renderer(0, prec) as r:
        r.set_camera(rt.camera(prec, FRAME[0], FRAME[1], CHUNK, BOUNCES))
        r.set_scene(sc)
        r.init_rng(1227)

        def fresh(call):
            def run():
                r.reset_accumulation(); r.init_rng(1227)
                return call()
            return run

        def measure(call, stamped):
            call()                                                   # warm-up: tables, buffers, kernels
            ms, clocks = [], []
            for _ in range(runs):
                ms.append(call())
                st = r.stats()
                clocks.append(st["main_clock_mhz"] if stamped else None)
            rec = {"ms": ms, "median_ms": statistics.median(ms), "clock_mhz": clocks}
            if stamped:                                              # rtiow_stats describes the last chunk or render, not a tile kernel
                rec.update(scene_source=st["scene_source"], vgprs=st["vgprs"], lds_bytes=st["lds_bytes"])
            return rec

        adaptive = dict(min_samples=EVERYBODY, max_samples=EVERYBODY)
        calls = {
            "chunk16": (fresh(lambda: r.accumulate(CHUNK)), fresh(lambda: r.accumulate_large(CHUNK)), True),
            "adaptive4": (fresh(lambda: r.accumulate_adaptive(ADAPTIVE_CHUNK, 0.0, **adaptive)[0]),
                          fresh(lambda: r.accumulate_adaptive_large(ADAPTIVE_CHUNK, 0.0, **adaptive)[0]), True),
            "guides": (r.render_guides, r.render_guides_large, False),
            "coverage2": (lambda: r.render_coverage(2), lambda: r.render_coverage_large(2), False),
        }
        for name in PAIRS:
            twin, large, stamped = calls[name]
            out[name] = {"twin": measure(twin, stamped), "large": measure(large, stamped)}
            out[name]["ratio_large_over_twin"] = out[name]["large"]["median_ms"] / out[name]["twin"]["median_ms"]
        out["render_large16"] = measure(lambda: (r.init_rng(1227), r.render_large())[1], True)
        out["ratio_chunk16_over_render_large16"] = out["chunk16"]["large"]["median_ms"] / out["render_large16"]["median_ms"]
        out["grid"] = r.large_grid()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "large_preview", "large_preview_probe.json"))
    ap.add_argument("--child", nargs=2, type=int)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.runs)
    if a.runs < 5:
        ap.error("the rule asks for the median of at least five runs")
    points = []
    for n, prec in POINTS:
        r = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--runs", str(a.runs), "--child", str(n), str(prec)],
                           capture_output=True, text=True)
        if r.returncode != 0:
            print("point (%d spheres, fp%d) failed with status %d: stopping\n%s" % (n, prec, r.returncode, r.stderr[-2000:]), file=sys.stderr)
            return 1
        p = json.loads(r.stdout.strip().splitlines()[-1])
        points.append(p)
        print("%6d spheres fp%d: " % (n, prec) + "; ".join("%s %.2f -> %.2f ms (x %.3f)" % (
            k, p[k]["twin"]["median_ms"], p[k]["large"]["median_ms"], p[k]["ratio_large_over_twin"]) for k in PAIRS)
            + "; chunk16 / render_large16 %.3f" % p["ratio_chunk16_over_render_large16"], flush=True)
    judged = [p for p in points if (p["spheres"], p["precision"]) in JUDGED]
    pays = len(judged) == len(JUDGED) and all(p[k]["large"]["median_ms"] < p[k]["twin"]["median_ms"] for p in judged for k in PAIRS)
    record = {"rule": "pays if a 16-sample chunk, a 4-sample adaptive chunk with everybody active, the first-hit guides and the coverage layers at 2 x 2 "
                      "are all faster through the device grid than through their twins on the same handle, at 6 000 and 20 000 spheres in fp32 and at "
                      "6 000 in fp64; the 2 000-sphere point and the ratio of a 16-sample large chunk to render_large at 16 samples are reported, not judged",
              "runs": a.runs, "points": points, "pays": pays}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("the feature %s" % ("pays" if pays else "does NOT pay yet"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
