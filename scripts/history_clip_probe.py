"""History clipped to the current frame's neighbourhood colours on one GPU, in the protocol of
scripts/history_probe.py:

  (a) cost at 1920 x 1080, scene 3, fp32 and fp64: a base committed at the reference's view, the camera turned 0.5 degrees, 4 samples,
      guides current; rtiow_history_update_clipped at clip_radius 1, 2 and 3, rtiow_history_update and ONE level of rtiow_denoise
      (levels = 1, default sigmas) in the same process, the five calls alternating; HIP-event kernel times, medians of --runs (at least
      20) after one warm-up each.  The rule of DESIGN.md section 4.10 applies to radius 1: its median must not exceed the filter
      level's (exit status 1 otherwise); radii 2 and 3 are reported;
  (b) quality at 320 x 180, 50 bounces, fp32, scenes 1 and 3, over the walk of tests/preview_drive.py (clip_walk: 8 cameras, 4
      samples each with independent noise, seeds 1227 + frame, update and commit every frame) at 0.5 and at 2 degrees a frame, against
      1024 samples at the last camera: clip_radius x clip_gamma x max_history swept, each walk's linear MSE divided by that of the
      plain walk at the same max_history -- for the temporal image (r_t) and for denoise_history() of it (r_dt), over the whole frame
      and over the specular pixels (scripts/specular_guides_probe.py's mask: the centre ray meets a specular surface first);
  (c) the defaults: the grid point with the smallest worse-of-two-scenes r_t over the whole frame at 0.5 degrees a frame and the
      existing HISTORY_MAX, the first such point in grid order; "defaults" holds the ratios at the values raytracingincuda_amd/api.py
      has now (tests/test_history_clip.py asserts on these).

Each part runs in a child process under its own `timeout`; the script stops at the first one that fails.  Writes one JSON record
(--out, default profiles/history_clip/history_clip_probe.json).

    python scripts/history_clip_probe.py [--runs 25] [--out FILE]
"""
import argparse
import ctypes
import itertools
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHILD_TIMEOUT_S = 420
SWEEP_RADIUS = (1, 2, 3)
SWEEP_GAMMA = (0.25, 0.5, 0.75, 1.0, 1.5, 2.0)
SWEEP_MAX_HISTORY = (16.0, 64.0)
SPEEDS = (0.5, 2.0)


def cost(prec, runs):
    import raytracingincuda_amd as rt
    from tests.preview_drive import orbit
    a = rt.api
    W, H = 1920, 1080
    params = (a.HISTORY_DEPTH_TOL, a.HISTORY_NORMAL_COS, a.HISTORY_MAX)
    with rt.Renderer(0, prec) as r:
        r.set_camera(rt.camera_look(prec, W, H, 1, 50)); r.set_scene(rt.build_scene(3, prec)); r.init_rng(1227)
        r.accumulate(4)
        r.history_update(); r.history_commit()
        r.set_camera(rt.camera_look(prec, W, H, 1, 50, lookfrom=orbit(0.5))); r.init_rng(1228)
        r.accumulate(4)
        r.render_guides()

        def clipped(radius):
            ms, n, k = ctypes.c_float(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
            r._check(r._lib.rtiow_history_update_clipped(r._h, *params, radius, a.HISTORY_CLIP_GAMMA, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(k)))
            return ms.value, n.value, k.value

        def update():
            ms, n = ctypes.c_float(0), ctypes.c_uint64(0)
            r._check(r._lib.rtiow_history_update(r._h, *params, ctypes.byref(ms), ctypes.byref(n)))
            return ms.value

        def level():
            ms = ctypes.c_float(0)
            r._check(r._lib.rtiow_denoise(r._h, 1, a.DENOISE_SIGMA_COLOR, a.DENOISE_SIGMA_NORMAL, a.DENOISE_SIGMA_ALBEDO, a.DENOISE_SIGMA_DEPTH, ctypes.byref(ms)))
            return ms.value

        counts = {radius: clipped(radius)[1:] for radius in SWEEP_RADIUS}       # warm-up
        update(); level()
        tc, tu, tl = {radius: [] for radius in SWEEP_RADIUS}, [], []
        for _ in range(runs):
            for radius in SWEEP_RADIUS:
                tc[radius].append(clipped(radius)[0])
            tu.append(update()); tl.append(level())
    u, l = statistics.median(tu), statistics.median(tl)
    out = {"history_update_ms": round(u, 4), "denoise_1_level_ms": round(l, 4), "runs": runs, "pixels": W * H, "clip_gamma": a.HISTORY_CLIP_GAMMA,
           "reprojected_pixels": int(counts[1][0])}
    for radius in SWEEP_RADIUS:
        c = statistics.median(tc[radius])
        out["clip_radius_%d" % radius] = {"history_update_clipped_ms": round(c, 4), "over_plain_update": round(c / u, 4),
                                          "over_filter_level": round(c / l, 4), "clipped_pixels": int(counts[radius][1])}
    return out


def name(radius, gamma, cap):
    return "clip_radius=%d,clip_gamma=%g,max_history=%g" % (radius, gamma, cap)


def quality(step_deg):
    import numpy as np
    import raytracingincuda_amd as rt
    from tests.preview_drive import begin, clip_walk, orbit
    from tests.preview_model import mse
    a = rt.api
    prec, W, H, B, frames = 32, 320, 180, 50, 8
    grid = list(itertools.product(SWEEP_RADIUS, SWEEP_GAMMA, SWEEP_MAX_HISTORY))
    out = {"sweep": {name(*p): {} for p in grid}, "plain_mse": {}, "defaults": {}}
    for scene_id in (1, 3):
        scene = "scene%d" % scene_id
        with rt.Renderer(0, prec) as r:                                    # the reference and the mask at the last camera
            begin(r, rt, prec, scene_id, rt.camera_look(prec, W, H, 1, B, lookfrom=orbit(step_deg * (frames - 1))))
            r.accumulate(1024)
            ref = r.read_linear().astype(np.float64)
            r.set_guide_mode(rt.GUIDES_SPECULAR, 8, float("inf"))
            mask = r.filter_guides()[3] >= 1
        both = lambda w, key: {"frame": mse(w[key], ref), "specular_pixels": mse(w[key], ref, mask)}
        plain = {}
        for cap in SWEEP_MAX_HISTORY:
            w = clip_walk(rt, scene_id, step_deg, None, cap)
            plain[cap] = {"t": both(w, "temporal"), "dt": both(w, "denoise_history")}
            out["plain_mse"].setdefault("max_history=%g" % cap, {})[scene] = dict(plain[cap], specular_pixels=int(mask.sum()), pixels=int(mask.size))
        for p in grid:
            w = clip_walk(rt, scene_id, step_deg, p[:2], p[2])
            t, dt = both(w, "temporal"), both(w, "denoise_history")
            out["sweep"][name(*p)][scene] = {
                "r_t": round(t["frame"] / plain[p[2]]["t"]["frame"], 4), "r_dt": round(dt["frame"] / plain[p[2]]["dt"]["frame"], 4),
                "r_t_specular": round(t["specular_pixels"] / plain[p[2]]["t"]["specular_pixels"], 4),
                "r_dt_specular": round(dt["specular_pixels"] / plain[p[2]]["dt"]["specular_pixels"], 4),
                "clipped_pixels_last_frame": w["clipped"], "reprojected_pixels_last_frame": w["reprojected"]}
            print(step_deg, scene, name(*p), out["sweep"][name(*p)][scene]["r_t"], file=sys.stderr, flush=True)
        w = clip_walk(rt, scene_id, step_deg, (a.HISTORY_CLIP_RADIUS, a.HISTORY_CLIP_GAMMA), a.HISTORY_MAX)
        out["defaults"][scene] = {"r_t": round(mse(w["temporal"], ref) / plain[a.HISTORY_MAX]["t"]["frame"], 4),
                                  "r_dt": round(mse(w["denoise_history"], ref) / plain[a.HISTORY_MAX]["dt"]["frame"], 4)}
    out["defaults"]["setting"] = name(a.HISTORY_CLIP_RADIUS, a.HISTORY_CLIP_GAMMA, a.HISTORY_MAX)
    eligible = [p for p in grid if p[2] == a.HISTORY_MAX]
    worst = {name(*p): max(out["sweep"][name(*p)]["scene%d" % s]["r_t"] for s in (1, 3)) for p in grid}
    out["sweep_worst_r_t"] = worst
    out["sweep_best_at_history_max"] = min((name(*p) for p in eligible), key=worst.__getitem__)     # the first of equals, in grid order
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "history_clip", "history_clip_probe.json"))
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs must be at least 20")
    if a.child:
        kind, arg = a.child.split(",")
        res = cost(int(arg), a.runs) if kind == "cost" else quality(float(arg))
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    import raytracingincuda_amd as rt
    record = {"build_id": rt.build_id(), "frame_cost_1920x1080": {}, "quality_320x180_b50_f32": {}}
    jobs = [("cost,%d" % p, "frame_cost_1920x1080", "scene3_f%d" % p) for p in (32, 64)]
    jobs += [("quality,%g" % d, "quality_320x180_b50_f32", "%g_degrees_a_frame" % d) for d in SPEEDS]
    for child, group, key in jobs:
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--child", child, "--runs", str(a.runs)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print("child %s failed (exit %d):\n%s" % (child, p.returncode, p.stdout[-2000:]), file=sys.stderr)
            return 1
        res = json.loads(line[0][7:])
        record[group][key] = res
        print(child, json.dumps({k: v for k, v in res.items() if k != "sweep"})[:3000], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    slow = [k for k, v in record["frame_cost_1920x1080"].items() if v["clip_radius_1"]["history_update_clipped_ms"] > v["denoise_1_level_ms"]]
    if slow:
        print("history_update_clipped at clip_radius 1 is slower than one filter level:", slow, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
