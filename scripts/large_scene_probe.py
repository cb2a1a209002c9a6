"""Large scenes on one GPU: render_large() against render() with the default scene source, by the rule of
DESIGN.md section 4.24.

For the jittered-lattice scenes of tests/large_scene.py -- 2 000, 6 000, 20 000 and 100 000 spheres in fp32, 2 000 and 6 000 in fp64 -- the
HIP-event kernel time of rtiow_render_large and of rtiow_render (default source, default schedule), the median of --runs after one
warm-up each, with the launch's stamped shader clock beside each run.  rtiow_render's device code is the parent commit's, instruction for
instruction (profiles/large_scenes/isa_diff_existing_kernels.txt), so its time is the parent's time.  Frame: 1920 x 1080 at 16 samples,
50 bounces where one warm-up render of the slower call stays under 20 s; otherwise 640 x 360, and the record says which.

The rule (fixed before anything was measured): the feature PAYS if render_large is faster than render at every size from 6 000 spheres
up, in both precisions.  The 2 000-sphere ratio -- against the LDS grid, where the device grid is expected to lose -- is reported, not
judged.  Each point runs in a child process under its own `timeout`; the script stops at the first one that fails.  Writes one JSON
record (--out).

    python scripts/large_scene_probe.py [--runs 5] [--out profiles/large_scenes/large_scene_probe.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTS = [(2000, 32), (6000, 32), (20000, 32), (100000, 32), (2000, 64), (6000, 64)]
JUDGED_FROM = 6000
FULL, SMALL = (1920, 1080), (640, 360)
SAMPLES, BOUNCES = 16, 50
SLOW_LIMIT_MS = 20000.0
CHILD_TIMEOUT_S = 420


def child(n, prec, runs):
    sys.path.insert(0, HERE)
    import raytracingincuda_amd as rt
    from tests import large_scene
    sc = large_scene.lattice(n, prec)
    out = {"spheres": n, "precision": prec, "samples": SAMPLES, "bounces": BOUNCES}
    with rt.Renderer(0, prec) as r:
        r.set_scene(sc)

        def timed(call, frame):
            r.set_camera(rt.camera(prec, frame[0], frame[1], SAMPLES, BOUNCES))
            r.init_rng(1227)
            ms = call()
            st = r.stats()
            return ms, st

        frame = FULL
        warm_ms, st = timed(lambda: r.render(0), frame)              # the slower call at these sizes: it decides the frame
        if warm_ms > SLOW_LIMIT_MS:
            frame = SMALL
            warm_ms, st = timed(lambda: r.render(0), frame)
        out["frame"] = list(frame)
        out["render_source"] = st["scene_source"]
        out["render_warmup_ms"] = warm_ms
        for name, call in (("render", lambda: r.render(0)), ("render_large", r.render_large)):
            timed(call, frame)                                       # warm-up (tables, kernels, the carried order of the sorted schedule)
            ms, clocks = [], []
            for _ in range(runs):
                t, st = timed(call, frame)
                ms.append(t); clocks.append(st["main_clock_mhz"])
            out[name] = {"ms": ms, "median_ms": statistics.median(ms), "clock_mhz": clocks, "scene_source": st["scene_source"],
                         "schedule": st["schedule"], "vgprs": st["vgprs"], "lds_bytes": st["lds_bytes"], "scene_prepare_ms": st["scene_prepare_ms"]}
        out["grid"] = r.large_grid()
    out["ratio_large_over_render"] = out["render_large"]["median_ms"] / out["render"]["median_ms"]
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "large_scenes", "large_scene_probe.json"))
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
        points.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print("%6d spheres fp%d %dx%d: render %.2f ms (source %d), render_large %.2f ms, ratio %.3f" % (
            n, prec, points[-1]["frame"][0], points[-1]["frame"][1], points[-1]["render"]["median_ms"], points[-1]["render"]["scene_source"],
            points[-1]["render_large"]["median_ms"], points[-1]["ratio_large_over_render"]), flush=True)
    judged = [p for p in points if p["spheres"] >= JUDGED_FROM]
    pays = all(p["render_large"]["median_ms"] < p["render"]["median_ms"] for p in judged)
    record = {"rule": "pays if render_large is faster than render at every size from %d spheres up, in both precisions; smaller sizes are reported, not judged" % JUDGED_FROM,
              "runs": a.runs, "points": points, "pays": pays}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("the feature %s" % ("pays" if pays else "does NOT pay yet"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
