"""Progressive rendering against the one-shot render, on one GPU: the 1920 x 1080 scene-3 frame at 100 spp and 50 bounces rendered
whole by rtiow_render (RTIOW_SCHED_SORTED and RTIOW_SCHED_PERSISTENT) and accumulated in chunks by rtiow_accumulate (fp32: 1 x 100,
4 x 25, 10 x 10, 100 x 1; fp64: 1 x 100, 4 x 25).  A chunked figure is the sum of the chunks' HIP-event times; every figure is the
median of --runs after one warm-up.  The accumulated frame is checked bit for bit against the one-shot one.  Prints one JSON record.

    python scripts/accumulate_probe.py [--runs 7] [--out profiles/accumulate/accumulate_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import raytracingincuda_amd as rt  # noqa: E402

W, H, S, B, SCENE = 1920, 1080, 100, 50, 3
PLANS = {32: [[100], [25] * 4, [10] * 10, [1] * 100], 64: [[100], [25] * 4]}


def _median(f, runs):
    f()                                                     # warm-up
    return statistics.median(f() for _ in range(runs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rec = {"probe": "accumulate", "build_id": rt.build_id(), "frame": "scene%d_%dx%d_%dspp_%db" % (SCENE, W, H, S, B), "runs": a.runs,
           "statistic": "median after one warm-up; chunked = sum of the chunks' kernel_ms", "results": {}}
    for prec in (32, 64):
        res = {}
        with rt.Renderer(0, prec) as r:
            r.set_camera(rt.camera(prec, W, H, S, B))
            r.set_scene(rt.build_scene(SCENE, prec))
            r.init_rng(1227)
            for name, sched in (("render_sorted_ms", rt.SCHED_SORTED), ("render_persistent_ms", rt.SCHED_PERSISTENT)):
                r.set_schedule(sched, 0)
                res[name] = round(_median(lambda: r.render(0), a.runs), 3)
            want = r.read_framebuffer()
            r.set_schedule(rt.SCHED_SORTED, 0)
            for plan in PLANS[prec]:
                def chunked():
                    r.reset_accumulation()
                    return sum(r.accumulate(k) for k in plan)
                key = "accumulate_%dx%d_ms" % (len(plan), plan[0])
                res[key] = round(_median(chunked, a.runs), 3)
                res[key.replace("_ms", "_bit_exact")] = bool(np.array_equal(r.read_framebuffer().view(np.uint8), want.view(np.uint8)))
            res["accumulate_1x100_vs_persistent"] = round(res["accumulate_1x100_ms"] / res["render_persistent_ms"] - 1.0, 4)
            res["accumulate_stats"] = {k: v for k, v in r.stats().items() if k in ("vgprs", "grid_blocks", "scene_source", "main_clock_mhz")}
        rec["results"]["f%d" % prec] = res
    line = json.dumps(rec, sort_keys=True)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
