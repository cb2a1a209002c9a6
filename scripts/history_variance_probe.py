"""Variance-guided filtering of the temporal image on one GPU, in the protocol of
scripts/history_clip_probe.py:

  (a) cost at 1920 x 1080, scene 3, fp32 and fp64, on that script's frame (a base committed at the reference's view, the camera turned
      0.5 degrees, 4 samples, a clipped update at its defaults, guides current), once after plain chunks (every pixel takes the spatial
      estimate: the window loop runs everywhere) and once after accumulate_with_variance (every pixel is measured: no window loop).
      HIP-event kernel times of whole calls, medians of --runs (at least 20) after one warm-up each, the calls alternating in one process:
      rtiow_denoise_history_variance at 1 level and variance_radius 1, 2, 3, the same at 5 levels and the default radius,
      rtiow_denoise_history at 5 levels, rtiow_denoise at 1 level (the yardstick of DESIGN.md section 4.10) and, on the measured
      route, rtiow_denoise_variance at 5 levels;
  (b) temporal_noise_kernel alone: the same calls under `rocprofv3 --kernel-trace` in a run of its own (--rocprof-dir says where it
      writes), each dispatch's end - start from the trace, medians per route and radius next to denoise_level_kernel's.  The rule of
      section 4.10 applies: the new kernel's median must not exceed one level of rtiow_denoise (exit status 1 otherwise);
  (c) quality at 320 x 180, 50 bounces, fp32, scenes 1 and 3, over the walk of DESIGN.md section 4.10 (8 cameras, 4 samples each with
      independent noise, seeds 1227 + frame, a clipped update at its defaults and a commit every frame) at 0.5 and at 2 degrees a
      frame, against 1024 samples at the last camera: r_v = MSE(denoise_history_variance) / MSE(denoise_history at its defaults), both
      squared back to linear, over the whole frame and over the specular pixels (scripts/specular_guides_probe.py's mask), for
      sigma_variance x variance_radius swept, with accumulate_with_variance chunks ("measured") and with plain chunks ("spatial": the
      same images, the spatial estimate alone);
  (d) the defaults: the grid point with the smallest worse-of-two-scenes r_v over the whole frame on the measured walk at 0.5 degrees
      a frame, the first such point in grid order; "defaults" holds the ratios at the values raytracingincuda_amd/api.py has now.

Each part runs in a child process under its own `timeout`; the script stops at the first one that fails.  Writes one JSON record
(--out, default profiles/history_variance/history_variance_probe.json).

    python scripts/history_variance_probe.py [--runs 25] [--out FILE] [--rocprof-dir DIR] [--parts cost,trace,quality]
"""
import argparse
import csv
import ctypes
import glob
import itertools
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHILD_TIMEOUT_S = 420
SWEEP_SIGMA = (2.0, 3.0, 3.5, 4.0, 4.5, 5.0, 6.0, 8.0)           # scripts/denoise_variance_probe.py's points
SWEEP_RADIUS = (1, 2, 3)
SPEEDS = (0.5, 2.0)
ROUTES = ("spatial", "measured")


def probe_frame(rt, r, prec, route):
    """scripts/history_clip_probe.py's frame with a clipped update on top."""
    from tests.preview_drive import orbit
    W, H = 1920, 1080
    chunk = r.accumulate if route == "spatial" else r.accumulate_with_variance
    r.set_camera(rt.camera_look(prec, W, H, 1, 50)); r.set_scene(rt.build_scene(3, prec)); r.init_rng(1227)
    chunk(4)
    r.history_update_clipped(); r.history_commit()
    r.set_camera(rt.camera_look(prec, W, H, 1, 50, lookfrom=orbit(0.5))); r.init_rng(1228)
    chunk(4)
    r.render_guides()
    r.history_update_clipped()
    return W * H


def calls(rt, r, route):
    """name -> a function that makes the call and returns its HIP-event kernel time."""
    a = rt.api
    guides = (a.DENOISE_SIGMA_NORMAL, a.DENOISE_SIGMA_ALBEDO, a.DENOISE_SIGMA_DEPTH)

    def timed(fn, *args):
        def go():
            ms = ctypes.c_float(0)
            r._check(fn(r._h, *args, ctypes.byref(ms)))
            return ms.value
        return go

    lib = r._lib
    out = {"denoise_history_variance_1_level_r%d" % radius: timed(lib.rtiow_denoise_history_variance, 1, a.HISTORY_SIGMA_VARIANCE, *guides, radius)
           for radius in SWEEP_RADIUS}
    out["denoise_1_level"] = timed(lib.rtiow_denoise, 1, a.DENOISE_SIGMA_COLOR, *guides)
    out["denoise_history_variance_5_levels"] = timed(lib.rtiow_denoise_history_variance, 5, a.HISTORY_SIGMA_VARIANCE, *guides, a.HISTORY_VARIANCE_RADIUS)
    out["denoise_history_5_levels"] = timed(lib.rtiow_denoise_history, 5, a.DENOISE_SIGMA_COLOR, *guides)
    if route == "measured":
        out["denoise_variance_5_levels"] = timed(lib.rtiow_denoise_variance, 5, a.DENOISE_SIGMA_VARIANCE, *guides)
    return out


def cost(prec, runs):
    import raytracingincuda_amd as rt
    out = {"runs": runs}
    for route in ROUTES:
        with rt.Renderer(0, prec) as r:
            out["pixels"] = probe_frame(rt, r, prec, route)
            fns = calls(rt, r, route)
            for fn in fns.values():                          # warm-up
                fn()
            times = {k: [] for k in fns}
            for _ in range(runs):
                for k, fn in fns.items():
                    times[k].append(fn())
        out[route] = {k + "_ms": round(statistics.median(v), 4) for k, v in times.items()}
    return out


def trace(prec, runs):
    """The calls whose kernels (b) reads from the trace, in a fixed order: per route, runs + 1 rounds of {radius 1, 2, 3, rtiow_denoise}."""
    import raytracingincuda_amd as rt
    for route in ROUTES:
        with rt.Renderer(0, prec) as r:
            probe_frame(rt, r, prec, route)
            fns = calls(rt, r, route)
            for _ in range(runs + 1):
                for radius in SWEEP_RADIUS:
                    fns["denoise_history_variance_1_level_r%d" % radius]()
                fns["denoise_1_level"]()
    return {"runs": runs}


def read_trace(directory, runs):
    """Medians of end - start per route and radius from rocprofv3's kernel trace of trace() (the first round of each route is warm-up)."""
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise RuntimeError("expected one kernel trace under %s, found %s" % (directory, files))
    with open(files[0], newline="") as f:
        rows = list(csv.DictReader(f))
    key = {k.lower(): k for k in rows[0]}
    name, start, end = key["kernel_name"], key["start_timestamp"], key["end_timestamp"]
    rows.sort(key=lambda row: int(row[start]))
    ms = lambda sub: [(int(row[end]) - int(row[start])) * 1e-6 for row in rows if sub in row[name]]
    noise, level = ms("temporal_noise_kernel<"), ms("denoise_level_kernel<")
    per_route = (runs + 1) * len(SWEEP_RADIUS)
    if len(noise) != len(ROUTES) * per_route or len(level) != len(ROUTES) * (runs + 1):
        raise RuntimeError("unexpected dispatch counts in the trace: %d, %d" % (len(noise), len(level)))
    out = {}
    for i, route in enumerate(ROUTES):
        mine = noise[i * per_route:(i + 1) * per_route][len(SWEEP_RADIUS):]
        lv = statistics.median(level[i * (runs + 1):(i + 1) * (runs + 1)][1:])
        out[route] = {"denoise_level_kernel_ms": round(lv, 4)}
        for j, radius in enumerate(SWEEP_RADIUS):
            t = statistics.median(mine[j::len(SWEEP_RADIUS)])
            out[route]["temporal_noise_kernel_r%d_ms" % radius] = round(t, 4)
            out[route]["r%d_over_filter_level" % radius] = round(t / lv, 4)
    return out


def name(sigma, radius):
    return "sigma_variance=%g,variance_radius=%d" % (sigma, radius)


def walk(rt, scene_id, step_deg, route, grid, frames=8, spp=4, W=320, H=180, B=50, prec=32):
    """The walk of (c); returns the linear images of the last frame: denoise_history() at its defaults and denoise_history_variance()
    at every grid point and at the defaults."""
    import numpy as np
    from tests.preview_drive import begin, move, orbit
    a = rt.api
    cams = [rt.camera_look(prec, W, H, 1, B, lookfrom=orbit(step_deg * k)) for k in range(frames)]
    out = {}
    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, scene_id, cams[0])
        for k, cam in enumerate(cams):
            move(r, cam, 1227 + k)
            if route == "spatial":
                r.accumulate(spp)
            else:
                r.accumulate_with_variance(spp)
            r.history_update_clipped()
            if k < frames - 1:
                r.history_commit()
        out["temporal"] = r.history()[0].astype(np.float64)
        out["denoise_history"] = r.denoise_history().astype(np.float64) ** 2
        for p in grid:
            out[name(*p)] = r.denoise_history_variance(sigma_variance=p[0], variance_radius=p[1]).astype(np.float64) ** 2
        out["defaults"] = r.denoise_history_variance().astype(np.float64) ** 2
    return out


def quality(step_deg):
    import numpy as np
    import raytracingincuda_amd as rt
    from tests.preview_drive import begin, orbit
    from tests.preview_model import mse
    a = rt.api
    prec, W, H, B, frames = 32, 320, 180, 50, 8
    grid = list(itertools.product(SWEEP_SIGMA, SWEEP_RADIUS))
    out = {route: {"sweep": {name(*p): {} for p in grid}, "denoise_history_mse": {}, "defaults": {}} for route in ROUTES}
    for scene_id in (1, 3):
        scene = "scene%d" % scene_id
        with rt.Renderer(0, prec) as r:                                    # the reference and the mask at the last camera
            begin(r, rt, prec, scene_id, rt.camera_look(prec, W, H, 1, B, lookfrom=orbit(step_deg * (frames - 1))))
            r.accumulate(1024)
            ref = r.read_linear().astype(np.float64)
            r.set_guide_mode(rt.GUIDES_SPECULAR, 8, float("inf"))
            mask = r.filter_guides()[3] >= 1
        both = lambda img: {"frame": mse(img, ref), "specular_pixels": mse(img, ref, mask)}
        ratios = lambda img, base: {"r_v": round(both(img)["frame"] / base["frame"], 4),
                                    "r_v_specular": round(both(img)["specular_pixels"] / base["specular_pixels"], 4)}
        images = {route: walk(rt, scene_id, step_deg, route, grid) for route in ROUTES}
        if not np.array_equal(images["spatial"]["temporal"], images["measured"]["temporal"]):
            raise RuntimeError("the two routes' temporal images differ")
        for route in ROUTES:
            w = images[route]
            base = both(w["denoise_history"])
            out[route]["denoise_history_mse"][scene] = dict(base, temporal=both(w["temporal"]), specular_pixels_count=int(mask.sum()), pixels=int(mask.size))
            for p in grid:
                out[route]["sweep"][name(*p)][scene] = ratios(w[name(*p)], base)
            out[route]["defaults"][scene] = ratios(w["defaults"], base)
            print(step_deg, scene, route, out[route]["defaults"][scene], file=sys.stderr, flush=True)
    for route in ROUTES:
        out[route]["defaults"]["setting"] = name(a.HISTORY_SIGMA_VARIANCE, a.HISTORY_VARIANCE_RADIUS)
        worst = {name(*p): max(out[route]["sweep"][name(*p)]["scene%d" % s]["r_v"] for s in (1, 3)) for p in grid}
        out[route]["sweep_worst_r_v"] = worst
        out[route]["sweep_best"] = min((name(*p) for p in grid), key=worst.__getitem__)             # the first of equals, in grid order
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "history_variance", "history_variance_probe.json"))
    ap.add_argument("--rocprof-dir", default="")
    ap.add_argument("--parts", default="cost,trace,quality")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs must be at least 20")
    if a.child:
        kind, arg = a.child.split(",")
        res = {"cost": lambda: cost(int(arg), a.runs), "trace": lambda: trace(int(arg), a.runs), "quality": lambda: quality(float(arg))}[kind]()
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    import raytracingincuda_amd as rt
    parts = a.parts.split(",")
    record = {"build_id": rt.build_id(), "call_cost_1920x1080": {}, "kernel_cost_1920x1080": {}, "quality_320x180_b50_f32": {}}
    if os.path.exists(a.out):                            # parts measured in an earlier call stay
        with open(a.out) as f:
            old = json.load(f)
        if old.get("build_id") == record["build_id"]:
            record = old
    jobs = []
    if "cost" in parts:
        jobs += [("cost,%d" % p, "call_cost_1920x1080", "scene3_f%d" % p) for p in (32, 64)]
    if "trace" in parts:
        jobs += [("trace,%d" % p, "kernel_cost_1920x1080", "scene3_f%d" % p) for p in (32, 64)]
    if "quality" in parts:
        jobs += [("quality,%g" % d, "quality_320x180_b50_f32", "%g_degrees_a_frame" % d) for d in SPEEDS]
    for child, group, key in jobs:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", child, "--runs", str(a.runs)]
        with tempfile.TemporaryDirectory(dir=a.rocprof_dir or None) as tmp:
            if child.startswith("trace"):                    # the program itself goes after `--`
                cmd = ["rocprofv3", "--kernel-trace", "-d", tmp, "-o", "kt", "--output-format", "csv", "--"] + cmd
            p = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT_S)] + cmd, stdout=subprocess.PIPE, text=True)
            line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print("child %s failed (exit %d):\n%s" % (child, p.returncode, p.stdout[-2000:]), file=sys.stderr)
                return 1
            res = json.loads(line[0][7:])
            if child.startswith("trace"):
                res.update(read_trace(tmp, a.runs))
        record[group][key] = res
        print(child, json.dumps({k: ({kk: vv for kk, vv in v.items() if kk not in ("sweep", "sweep_worst_r_v")} if isinstance(v, dict) else v)
                                 for k, v in res.items()})[:3000], flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    slow = [(k, route, radius) for k, v in record["kernel_cost_1920x1080"].items() for route in ROUTES for radius in SWEEP_RADIUS
            if v[route]["temporal_noise_kernel_r%d_ms" % radius] > v[route]["denoise_level_kernel_ms"]]
    if slow:
        print("temporal_noise_kernel is slower than one filter level:", slow, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
