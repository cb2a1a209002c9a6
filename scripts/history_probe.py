"""Temporal history for progressive previews on one GPU:

  (a) cost at 1920 x 1080, scene 3, fp32 and fp64: a base committed at the reference's view, the camera turned 0.5 degrees, 4 samples,
      guides current; rtiow_history_update next to ONE level of rtiow_denoise (levels = 1, default sigmas) in the same process, the
      two calls alternating; HIP-event kernel times, medians of --runs (at least 20) after one warm-up each.  The update gathers 4
      taps where a filter level gathers 25, so its median must not exceed the level's (exit status 1 otherwise);
  (b) quality at 320 x 180, 50 bounces, fp32, scenes 1 and 3, over the walk of tests/preview_drive.py (orbit_walk: 8 cameras, 0.5
      degrees apart, 4 samples each with independent noise, update and commit every frame), against 1024 samples at the last camera:
      q_t = linear MSE of the temporal image / MSE of the noisy accumulation, q_dt = MSE of denoise_history() / MSE of denoise(),
      at the defaults of raytracingincuda_amd/api.py (tests/test_history.py asserts on these);
  (c) --sweep: q_t and q_dt over a grid of depth_tol, normal_cos and max_history; the defaults are the grid point with the smallest
      worse-of-two-scenes q_t, the first such point in grid order.

Each part runs in a child process under its own `timeout`; the script stops at the first one that fails.  Writes one JSON record
(--out, default profiles/history/history_probe.json).

    python scripts/history_probe.py [--runs 25] [--sweep] [--out FILE]
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

CHILD_TIMEOUT_S = 240
SWEEP_DEPTH_TOL = (0.005, 0.02, 0.05, 0.1)
SWEEP_NORMAL_COS = (0.5, 0.9, 0.98)
SWEEP_MAX_HISTORY = (8.0, 16.0, 64.0, float("inf"))


def cost(prec, runs):
    import raytracingincuda_amd as rt
    from tests.preview_drive import orbit
    a = rt.api
    W, H = 1920, 1080
    with rt.Renderer(0, prec) as r:
        r.set_camera(rt.camera_look(prec, W, H, 1, 50)); r.set_scene(rt.build_scene(3, prec)); r.init_rng(1227)
        r.accumulate(4)
        r.history_update(); r.history_commit()
        r.set_camera(rt.camera_look(prec, W, H, 1, 50, lookfrom=orbit(0.5))); r.init_rng(1228)
        r.accumulate(4)
        r.render_guides()

        def update():
            ms, n = ctypes.c_float(0), ctypes.c_uint64(0)
            r._check(r._lib.rtiow_history_update(r._h, a.HISTORY_DEPTH_TOL, a.HISTORY_NORMAL_COS, a.HISTORY_MAX, ctypes.byref(ms), ctypes.byref(n)))
            return ms.value, n.value

        def level():
            ms = ctypes.c_float(0)
            r._check(r._lib.rtiow_denoise(r._h, 1, a.DENOISE_SIGMA_COLOR, a.DENOISE_SIGMA_NORMAL, a.DENOISE_SIGMA_ALBEDO, a.DENOISE_SIGMA_DEPTH, ctypes.byref(ms)))
            return ms.value

        _, carried = update(); level()                      # warm-up
        tu, tl = [], []
        for _ in range(runs):
            tu.append(update()[0]); tl.append(level())
    u, l = statistics.median(tu), statistics.median(tl)
    return {"history_update_ms": round(u, 4), "denoise_1_level_ms": round(l, 4), "ratio": round(u / l, 4), "runs": runs,
            "reprojected_pixels": int(carried), "pixels": W * H}


def quality(sweep):
    import raytracingincuda_amd as rt
    from tests.preview_drive import orbit_reference, orbit_walk
    from tests.preview_model import quality as q_of
    a = rt.api
    default = (a.HISTORY_DEPTH_TOL, a.HISTORY_NORMAL_COS, a.HISTORY_MAX)
    grid = list(itertools.product(SWEEP_DEPTH_TOL, SWEEP_NORMAL_COS, SWEEP_MAX_HISTORY)) if sweep else []
    name = lambda p: "depth_tol=%g,normal_cos=%g,max_history=%g" % p
    out = {"defaults": name(default), "orbit": {}}
    table = {name(p): {} for p in grid}
    for scene_id in (1, 3):
        ref = orbit_reference(rt, scene_id)
        w = orbit_walk(rt, scene_id, ref=ref)
        q_t, q_dt = q_of(w)
        out["orbit"]["scene%d" % scene_id] = {"q_t": round(q_t, 4), "q_dt": round(q_dt, 4), "reprojected_pixels_last_frame": w["reprojected"]}
        for p in grid:
            q_t, q_dt = q_of(orbit_walk(rt, scene_id, params=p, ref=ref))
            table[name(p)]["scene%d" % scene_id] = {"q_t": round(q_t, 4), "q_dt": round(q_dt, 4)}
    if sweep:
        worst = {name(p): max(table[name(p)]["scene%d" % s]["q_t"] for s in (1, 3)) for p in grid}
        out["sweep"] = table
        out["sweep_worst_q_t"] = worst
        out["sweep_best"] = min((name(p) for p in grid), key=worst.__getitem__)       # the first of equals, in grid order
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "history", "history_probe.json"))
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs must be at least 20")
    if a.child:
        kind, *rest = a.child.split(",")
        res = {"cost": lambda: cost(int(rest[0]), a.runs), "quality": lambda: quality(a.sweep)}[kind]()
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    import raytracingincuda_amd as rt
    record = {"build_id": rt.build_id(), "frame_cost_1920x1080": {}}
    jobs = [("cost,%d" % p, "frame_cost_1920x1080", "scene3_f%d" % p) for p in (32, 64)] + [("quality", None, "quality_320x180_b50_f32")]
    for child, group, name in jobs:
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--child", child, "--runs", str(a.runs)]
        if a.sweep:
            cmd.append("--sweep")
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print("child %s failed (exit %d):\n%s\n%s" % (child, p.returncode, p.stdout[-2000:], p.stderr[-4000:]), file=sys.stderr)
            return 1
        res = json.loads(line[0][7:])
        (record[group] if group else record)[name] = res
        print(child, json.dumps(res)[:1500], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    slow = [k for k, v in record["frame_cost_1920x1080"].items() if v["history_update_ms"] > v["denoise_1_level_ms"]]
    if slow:
        print("history_update is slower than one filter level:", slow, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
