"""Filter guides through mirrors and glass on one GPU, 1920 x 1080, 50 bounces:

  (a) cost, scenes 3 and 1, fp32 and fp64: rtiow_render_guides in FIRST_HIT mode (guide_kernel) and in SPECULAR mode (guide_kernel +
      guide_chain_kernel), and a 5-level rtiow_denoise with current guides in both modes, on an accumulation of 4 samples; HIP-event
      kernel times, medians of --runs after one warm-up;
  (b) quality, fp32, scenes 1 and 3, at 4, 16 and 64 samples: the linear MSE of denoise()^2 (default sigmas) against a 1024-sample
      accumulation, in FIRST_HIT and in SPECULAR mode (the defaults of raytracingincuda_amd/api.py), over the frame and over the
      SPECULAR PIXELS: those whose centre ray meets a specular surface first (bounces >= 1 with max_bounces 8, max_fuzz +inf);
  (c) the same two MSEs at 16 samples for max_bounces in {1, 2, 4, 8} x max_fuzz in {0, 0.1, 0.25, +inf} (how the defaults were chosen;
      the mask stays that of (b), so the settings are compared over the same pixels).

Each part runs in a child process under its own `timeout`; the script stops at the first one that fails.  Writes one JSON record
(--out, default profiles/specular_guides/specular_guides_probe.json).

    python scripts/specular_guides_probe.py [--runs 7] [--out profiles/specular_guides/specular_guides_probe.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [(3, 32), (3, 64), (1, 32), (1, 64)]
CHILD_TIMEOUT_S = 240
INF = float("inf")
W, H, B = 1920, 1080, 50
SAMPLES = (4, 16, 64)
SWEEP_BOUNCES = (1, 2, 4, 8)
SWEEP_FUZZ = (0.0, 0.1, 0.25, INF)


def _median(f, runs):
    f()                                                     # warm-up
    return statistics.median(f() for _ in range(runs))


def cost(scene_id, prec, runs):
    import raytracingincuda_amd as rt
    res = {}
    with rt.Renderer(0, prec) as r:
        r.set_camera(rt.camera(prec, W, H, 1, B))
        r.set_scene(rt.build_scene(scene_id, prec))
        r.init_rng(1227)
        r.accumulate(4)

        def den():
            ms = ctypes.c_float(0)
            r._check(r._lib.rtiow_denoise(r._h, 5, rt.api.DENOISE_SIGMA_COLOR, rt.api.DENOISE_SIGMA_NORMAL, rt.api.DENOISE_SIGMA_ALBEDO,
                                          rt.api.DENOISE_SIGMA_DEPTH, ctypes.byref(ms)))
            return ms.value
        for mode, name in ((rt.GUIDES_FIRST_HIT, "first_hit"), (rt.GUIDES_SPECULAR, "specular")):
            r.set_guide_mode(mode)
            res["render_guides_%s_ms" % name] = round(_median(lambda: r.render_guides(), runs), 4)
            res["denoise_5_levels_%s_ms" % name] = round(_median(den, runs), 4)
    return res


def quality(scene_id):
    import numpy as np
    import raytracingincuda_amd as rt
    prec = 32
    with rt.Renderer(0, prec) as r:
        r.set_camera(rt.camera(prec, W, H, 1, B)); r.set_scene(rt.build_scene(scene_id, prec)); r.init_rng(1227)
        r.accumulate(1024)
        ref = r.read_linear().astype(np.float64)
        r.set_guide_mode(rt.GUIDES_SPECULAR, 8, INF)
        mask = r.filter_guides()[3] >= 1
        r.set_guide_mode(rt.GUIDES_FIRST_HIT)
        out = {"specular_pixels": int(mask.sum()), "pixels": int(mask.size), "by_samples": {}}

        def mses(img):
            d = (img.astype(np.float64) - ref) ** 2
            return {"frame": float(d.mean()), "specular_pixels": float(d[mask].mean())}

        def denoised(mode, *args):
            r.set_guide_mode(mode, *args)
            return mses(r.denoise().astype(np.float64) ** 2)

        r.reset_accumulation()
        for n in SAMPLES:                                   # chunks add up to the same bits as one call
            r.accumulate(n - r.accumulated_samples)
            rec = {"noisy": mses(r.read_linear()), "first_hit": denoised(rt.GUIDES_FIRST_HIT), "specular": denoised(rt.GUIDES_SPECULAR)}
            if n == 16:
                rec["sweep"] = [dict(max_bounces=mb, max_fuzz=mf, **denoised(rt.GUIDES_SPECULAR, mb, mf)) for mb in SWEEP_BOUNCES for mf in SWEEP_FUZZ]
            out["by_samples"][str(n)] = rec
    out["defaults"] = {"max_bounces": rt.api.GUIDE_MAX_BOUNCES, "max_fuzz": rt.api.GUIDE_MAX_FUZZ}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "specular_guides", "specular_guides_probe.json"))
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        kind, *rest = a.child.split(",")
        res = cost(int(rest[0]), int(rest[1]), a.runs) if kind == "cost" else quality(int(rest[0]))
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    import raytracingincuda_amd as rt
    record = {"build_id": rt.build_id(), "frame": "%dx%d, %d bounces" % (W, H, B), "frame_cost": {}, "quality_f32": {}, "runs": a.runs}
    jobs = [("cost,%d,%d" % c, "scene%d_f%d" % c) for c in CONFIGS] + [("quality,%d" % s, "scene%d" % s) for s in (1, 3)]
    for child, name in jobs:
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--child", child, "--runs", str(a.runs)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print("child %s failed (exit %d):\n%s\n%s" % (child, p.returncode, p.stdout[-2000:], p.stderr[-4000:]), file=sys.stderr)
            return 1
        res = json.loads(line[0][7:])
        record["frame_cost" if child.startswith("cost") else "quality_f32"][name] = res
        print(name, json.dumps(res)[:600], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
