"""Host time per frame of the preview chain, for two or more builds of librtiow_hip.so on ONE device: interleaved child processes (one per
library and repeat, RTIOW_HIP_LIBRARY), each running the frame loop of a 1920 x 1080 fp32 preview --

    rtiow_accumulate(1), rtiow_history_update_clipped, rtiow_denoise_history_variance, rtiow_history_commit_filtered, rtiow_synchronize

-- with the defaults, nothing read back and no event times asked for, and taking the wall time of every frame after a warm-up.  Builds
with the same device code differ in the host code of these calls alone.

    preview_host_overhead.py [--repeats 3] [--frames 200] [--warmup 20] [--out FILE] BASE.so OTHER.so [...]

A library's figure is the median of its repeats' medians; the spread of the first library (the base) is the largest minus the smallest
of its repeats' medians.  Exit status 1 if another library's figure exceeds the base's by more than that spread."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(frames, warmup):
    import raytracingincuda_amd as rt
    a = rt.api
    tol = (a.HISTORY_DEPTH_TOL, a.HISTORY_NORMAL_COS, a.HISTORY_MAX)
    guides = (a.DENOISE_SIGMA_NORMAL, a.DENOISE_SIGMA_ALBEDO, a.DENOISE_SIGMA_DEPTH)
    with rt.Renderer(0, 32) as r:
        r.set_camera(rt.camera(32, 1920, 1080, 1, 50))
        r.set_scene(rt.build_scene(3, 32))
        r.init_rng(1227)
        lib, h = r._lib, r._h
        ms = []
        for k in range(warmup + frames):
            t0 = time.perf_counter()
            rc = (lib.rtiow_accumulate(h, 1, 0, None)
                  or lib.rtiow_history_update_clipped(h, *tol, a.HISTORY_CLIP_RADIUS, a.HISTORY_CLIP_GAMMA, None, None, None)
                  or lib.rtiow_denoise_history_variance(h, a.DENOISE_LEVELS, a.HISTORY_SIGMA_VARIANCE, *guides, a.HISTORY_VARIANCE_RADIUS, None)
                  or lib.rtiow_history_commit_filtered(h, a.HISTORY_FEEDBACK_SIGMA_COLOR, *guides, a.HISTORY_FEEDBACK, None)
                  or lib.rtiow_synchronize(h))
            dt = (time.perf_counter() - t0) * 1e3
            if rc:
                raise SystemExit("frame %d failed with %d: %s" % (k, rc, lib.rtiow_last_error_string(h).decode()))
            if k >= warmup:
                ms.append(dt)
        print(json.dumps({"build_id": rt.build_id(), "frames": frames, "ms_median": statistics.median(ms), "ms_min": min(ms),
                          "ms_p90": sorted(ms)[int(0.9 * len(ms))]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.frames, a.warmup)
    if len(a.libs) < 2:
        ap.error("give the base library and at least one other")
    runs = {l: [] for l in a.libs}
    for rd in range(a.repeats):
        for l in a.libs:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--frames", str(a.frames), "--warmup", str(a.warmup)],
                                 env=dict(os.environ, RTIOW_HIP_LIBRARY=os.path.abspath(l)), capture_output=True, text=True, timeout=120)
            if out.returncode != 0:
                print(l, "FAILED", out.stdout[-400:], out.stderr[-400:])
                return 1
            runs[l].append(json.loads(out.stdout.splitlines()[-1]))
    medians = {l: [r["ms_median"] for r in runs[l]] for l in a.libs}
    base = a.libs[0]
    spread = max(medians[base]) - min(medians[base])
    result = {"loop": "1920x1080 fp32 scene 3: accumulate(1), history_update_clipped, denoise_history_variance, history_commit_filtered, synchronize",
              "frames": a.frames, "warmup": a.warmup, "repeats": a.repeats, "base": os.path.basename(base), "base_spread_ms": spread, "libraries": {}}
    worst = 0
    for l in a.libs:
        fig = statistics.median(medians[l])
        result["libraries"][os.path.basename(l)] = {"build_id": runs[l][0]["build_id"], "ms_median": fig, "ms_median_of_each_repeat": medians[l],
                                                    "ms_min_of_each_repeat": [r["ms_min"] for r in runs[l]],
                                                    "over_base_ms": fig - statistics.median(medians[base])}
        worst = max(worst, fig - statistics.median(medians[base]))
    result["within_base_spread"] = worst <= spread
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if result["within_base_spread"] else 1


if __name__ == "__main__":
    sys.exit(main())
