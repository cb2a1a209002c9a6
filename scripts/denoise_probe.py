"""Denoised previews on one GPU:

  (a) cost at 1920 x 1080, scenes 3 and 1, fp32 and fp64: rtiow_render_guides, and a 5-level rtiow_denoise with current guides (the
      default sigmas), on an accumulation of 4 samples; HIP-event kernel times, medians of --runs after one warm-up;
  (b) quality at 320 x 180, 50 bounces, fp32, scenes 1 and 3: the linear MSE of denoise()^2 at 16 samples (default sigmas) against a
      1024-sample accumulation, divided by the MSE of the 16-sample linear image (tests/test_denoise.py asks for <= 0.5);
  (c) --sweep: the ratio of (b) for a grid of sigmas (how the defaults in raytracingincuda_amd/api.py were chosen).

Each part runs in a child process under its own `timeout`; the script stops at the first one that fails.  Writes one JSON record
(--out, default profiles/denoise/denoise_probe.json).

    python scripts/denoise_probe.py [--runs 7] [--sweep] [--out profiles/denoise/denoise_probe.json]
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

CONFIGS = [(3, 32), (3, 64), (1, 32), (1, 64)]
CHILD_TIMEOUT_S = 240
INF = float("inf")
SWEEP = {"sigma_color": (0.05, 0.07, 0.1, 0.14, 0.2), "sigma_normal": (0.1, 0.2, 0.4, INF), "sigma_albedo": (0.05, 0.2, INF), "sigma_depth": (0.05, 0.1, 0.5, INF)}


def _median(f, runs):
    f()                                                     # warm-up
    return statistics.median(f() for _ in range(runs))


def cost(scene_id, prec, runs):
    import raytracingincuda_amd as rt
    W, H, B = 1920, 1080, 50
    res = {}
    with rt.Renderer(0, prec) as r:
        r.set_camera(rt.camera(prec, W, H, 1, B))
        r.set_scene(rt.build_scene(scene_id, prec))
        r.init_rng(1227)
        r.accumulate(4)
        res["render_guides_ms"] = round(_median(lambda: r.render_guides(), runs), 4)

        def den():
            ms = ctypes.c_float(0)
            r._check(r._lib.rtiow_denoise(r._h, 5, rt.api.DENOISE_SIGMA_COLOR, rt.api.DENOISE_SIGMA_NORMAL, rt.api.DENOISE_SIGMA_ALBEDO,
                                          rt.api.DENOISE_SIGMA_DEPTH, ctypes.byref(ms)))
            return ms.value
        res["denoise_5_levels_ms"] = round(_median(den, runs), 4)
    return res


def quality(sweep):
    import numpy as np
    import raytracingincuda_amd as rt
    W, H, B, prec = 320, 180, 50, 32
    out = {}
    combos = [dict(zip(SWEEP, v)) for v in itertools.product(*SWEEP.values())] if sweep else []
    default = {"sigma_color": rt.api.DENOISE_SIGMA_COLOR, "sigma_normal": rt.api.DENOISE_SIGMA_NORMAL,
               "sigma_albedo": rt.api.DENOISE_SIGMA_ALBEDO, "sigma_depth": rt.api.DENOISE_SIGMA_DEPTH}
    for scene_id in (1, 3):
        with rt.Renderer(0, prec) as r:
            r.set_camera(rt.camera(prec, W, H, 1, B)); r.set_scene(rt.build_scene(scene_id, prec)); r.init_rng(1227)
            r.accumulate(1024)
            ref = r.read_linear().astype(np.float64)
            r.reset_accumulation()
            r.accumulate(16)
            mse16 = float(np.mean((r.read_linear().astype(np.float64) - ref) ** 2))
            ratio = lambda sig: float(np.mean((r.denoise(5, **sig).astype(np.float64) ** 2 - ref) ** 2)) / mse16
            rec = {"mse_16spp": mse16, "ratio_default": round(ratio(default), 4)}
            if sweep:
                rec["sweep"] = [dict(c, ratio=round(ratio(c), 4)) for c in combos]
            out["scene%d" % scene_id] = rec
    out["default_sigmas"] = default
    if sweep:                                               # the combination with the smaller worse-of-two-scenes ratio
        worst = [max(out["scene1"]["sweep"][k]["ratio"], out["scene3"]["sweep"][k]["ratio"]) for k in range(len(combos))]
        k = min(range(len(combos)), key=worst.__getitem__)
        out["sweep_best"] = dict(combos[k], worst_ratio=worst[k])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise", "denoise_probe.json"))
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        kind, *rest = a.child.split(",")
        res = cost(int(rest[0]), int(rest[1]), a.runs) if kind == "cost" else quality(a.sweep)
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    import raytracingincuda_amd as rt
    record = {"build_id": rt.build_id(), "frame_cost": {}, "runs": a.runs}
    jobs = [("cost,%d,%d" % c, "scene%d_f%d" % c) for c in CONFIGS] + [("quality", "quality")]
    for child, name in jobs:
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--child", child, "--runs", str(a.runs)]
        if a.sweep:
            cmd.append("--sweep")
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print("child %s failed (exit %d):\n%s\n%s" % (child, p.returncode, p.stdout[-2000:], p.stderr[-4000:]), file=sys.stderr)
            return 1
        res = json.loads(line[0][7:])
        if name == "quality":
            record["quality_320x180_b50_f32"] = res
        else:
            record["frame_cost"][name] = res
        print(name, json.dumps(res)[:400], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
