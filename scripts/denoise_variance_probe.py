"""Variance-guided denoising on one GPU:

  (a) cost at 1920 x 1080, scenes 3 and 1, fp32 and fp64, on an accumulation of 4 uniform samples with variance and current guides:
      a 5-level rtiow_denoise_variance next to a 5-level rtiow_denoise (default sigmas) in the same process, the two calls
      alternating; HIP-event kernel times, medians of --runs after one warm-up each;
  (b) --tile LIB: the LDS-tile form of the levels with step 1, 2 and 4 against the L1/L2 form, with the tuning build LIB
      (build.build_variant("tuning", ["-DRTIOW_TUNING"]): RTIOW_TUNE_VARIANCE_TILE, bit k = level k tiled): the 5-level time with
      no level, one level and all three tiled, the settings alternating inside every round; the images must agree bit for bit;
  (c) quality at 320 x 180, 50 bounces, fp32, scenes 1 and 3: q = linear MSE of the denoised image / MSE of the noisy one, against a
      1024-sample accumulation, at 4, 16 and 64 uniform samples, for denoise() at its defaults (q_fixed) and denoise_variance() at
      its defaults (q_var) (tests/test_denoise_variance.py asserts on these), and for scene 1 after accumulate_adaptive(8, thr,
      min_samples=8, max_samples=64) to convergence, thr = the median error after the first call;
  (d) --sweep: q_var for a grid of sigma_variance; the default in raytracingincuda_amd/api.py is the one with the smallest worst
      case, over the three sample counts, of the worse-of-two-scenes q_var / q_fixed.

Each part runs in a child process under its own `timeout`; the script stops at the first one that fails.  Writes one JSON record
(--out, default profiles/denoise_variance/denoise_variance_probe.json).

    python scripts/denoise_variance_probe.py [--runs 7] [--sweep] [--tile raytracingincuda_amd/lib/ab/tuning.so] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [(3, 32), (3, 64), (1, 32), (1, 64)]
CHILD_TIMEOUT_S = 240
SWEEP = (2.0, 3.0, 3.5, 4.0, 4.5, 5.0, 6.0, 8.0)
COUNTS = (4, 16, 64)
TILE_MASKS = (0, 1, 2, 4, 7)


def _prepare(rt, scene_id, prec):
    r = rt.Renderer(0, prec)
    r.set_camera(rt.camera(prec, 1920, 1080, 1, 50))
    r.set_scene(rt.build_scene(scene_id, prec))
    r.init_rng(1227)
    r.accumulate_with_variance(4)
    r.render_guides()
    return r


def _timed(r, fn, *sig):
    ms = ctypes.c_float(0)
    r._check(fn(r._h, 5, *sig, ctypes.byref(ms)))
    return ms.value


def cost(scene_id, prec, runs):
    import raytracingincuda_amd as rt
    a = rt.api
    guide = (a.DENOISE_SIGMA_NORMAL, a.DENOISE_SIGMA_ALBEDO, a.DENOISE_SIGMA_DEPTH)
    with _prepare(rt, scene_id, prec) as r:
        fixed = lambda: _timed(r, r._lib.rtiow_denoise, a.DENOISE_SIGMA_COLOR, *guide)
        var = lambda: _timed(r, r._lib.rtiow_denoise_variance, a.DENOISE_SIGMA_VARIANCE, *guide)
        fixed(); var()                                      # warm-up
        tf, tv = [], []
        for _ in range(runs):
            tf.append(fixed()); tv.append(var())
    f, v = statistics.median(tf), statistics.median(tv)
    return {"denoise_5_levels_ms": round(f, 4), "denoise_variance_5_levels_ms": round(v, 4), "ratio": round(v / f, 4)}


def tile(scene_id, prec, runs):
    import numpy as np
    import raytracingincuda_amd as rt
    a = rt.api
    sig = (a.DENOISE_SIGMA_VARIANCE, a.DENOISE_SIGMA_NORMAL, a.DENOISE_SIGMA_ALBEDO, a.DENOISE_SIGMA_DEPTH)
    times = {m: [] for m in TILE_MASKS}
    with _prepare(rt, scene_id, prec) as r:
        images = {}
        for m in TILE_MASKS:                                # warm-up, and the images
            os.environ["RTIOW_TUNE_VARIANCE_TILE"] = str(m)
            _timed(r, r._lib.rtiow_denoise_variance, *sig)
            images[m] = r.read_denoised()
        same = all(np.array_equal(images[m].view(np.uint8), images[0].view(np.uint8)) for m in TILE_MASKS)
        for _ in range(runs):
            for m in TILE_MASKS:
                os.environ["RTIOW_TUNE_VARIANCE_TILE"] = str(m)
                times[m].append(_timed(r, r._lib.rtiow_denoise_variance, *sig))
    res = {"tiled_levels_mask_%d_ms" % m: round(statistics.median(t), 4) for m, t in times.items()}
    res["same_bits"] = bool(same)
    return res


def quality(sweep):
    import numpy as np
    import raytracingincuda_amd as rt
    W, H, B, prec = 320, 180, 50, 32
    sigmas = sorted(set(SWEEP) | {rt.api.DENOISE_SIGMA_VARIANCE}) if sweep else [rt.api.DENOISE_SIGMA_VARIANCE]
    out = {"default_sigma_variance": rt.api.DENOISE_SIGMA_VARIANCE}
    mse = lambda img, ref: float(np.mean((img.astype(np.float64) - ref) ** 2))
    for scene_id in (1, 3):
        rec = {}
        with rt.Renderer(0, prec) as r:
            r.set_camera(rt.camera(prec, W, H, 1, B)); r.set_scene(rt.build_scene(scene_id, prec)); r.init_rng(1227)
            r.accumulate(1024)
            ref = r.read_linear().astype(np.float64)
            r.reset_accumulation()
            n = 0
            for total in COUNTS:
                r.accumulate_with_variance(total - n)
                n = total
                noisy = mse(r.read_linear(), ref)
                rec["n%d" % n] = {"mse_noisy": noisy, "q_fixed": round(mse(r.denoise().astype(np.float64) ** 2, ref) / noisy, 4),
                                  "q_var": {"%g" % s: round(mse(r.denoise_variance(sigma_variance=s).astype(np.float64) ** 2, ref) / noisy, 4) for s in sigmas}}
            if scene_id == 1:                               # an adaptive accumulation
                r.reset_accumulation()
                r.accumulate_adaptive(8, 0.0, min_samples=8, max_samples=64)
                thr = float(np.median(r.adaptive_state()[1]))
                active, calls = 1, 1
                while active:
                    _, active = r.accumulate_adaptive(8, thr, min_samples=8, max_samples=64)
                    calls += 1
                counts, _ = r.adaptive_state()
                noisy = mse(r.read_linear(), ref)
                rec["adaptive"] = {"threshold": thr, "calls": calls, "mean_samples": float(counts.mean()), "mse_noisy": noisy,
                                   "q_fixed": round(mse(r.denoise().astype(np.float64) ** 2, ref) / noisy, 4),
                                   "q_var": round(mse(r.denoise_variance().astype(np.float64) ** 2, ref) / noisy, 4)}
        out["scene%d" % scene_id] = rec
    if sweep:                                               # smallest worst case of the worse-of-two-scenes q_var / q_fixed
        worst = {s: max(out["scene%d" % sc]["n%d" % n]["q_var"]["%g" % s] / out["scene%d" % sc]["n%d" % n]["q_fixed"] for sc in (1, 3) for n in COUNTS)
                 for s in sigmas}
        best = min(sigmas, key=worst.__getitem__)
        out["sweep_worst_q_var_over_q_fixed"] = {"%g" % s: round(w, 4) for s, w in worst.items()}
        out["sweep_best"] = best
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--tile", default="", help="the tuning build of the library, for part (b)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_variance", "denoise_variance_probe.json"))
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        kind, *rest = a.child.split(",")
        res = {"cost": lambda: cost(int(rest[0]), int(rest[1]), a.runs), "tile": lambda: tile(int(rest[0]), int(rest[1]), a.runs),
               "quality": lambda: quality(a.sweep)}[kind]()
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    import raytracingincuda_amd as rt
    from raytracingincuda_amd.kernel_metadata import device_metadata
    record = {"build_id": rt.build_id(), "runs": a.runs, "frame_cost_1920x1080": {}, "tile_ab_1920x1080": {},
              "registers": {re.search(r"::(\w+<\w+>)", k).group(1): {"vgpr": v["vgpr"], "sgpr": v["sgpr"], "scratch": v["scratch"]}
                            for k, v in device_metadata()[0].items() if "variance_" in k or "denoise_level_kernel<" in k}}
    jobs = [("cost,%d,%d" % c, "frame_cost_1920x1080", "scene%d_f%d" % c, {}) for c in CONFIGS]
    if a.tile:
        jobs += [("tile,%d,%d" % c, "tile_ab_1920x1080", "scene%d_f%d" % c, {"RTIOW_HIP_LIBRARY": os.path.abspath(a.tile)}) for c in CONFIGS]
    jobs.append(("quality", None, "quality_320x180_b50_f32", {}))
    for child, group, name, env in jobs:
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--child", child, "--runs", str(a.runs)]
        if a.sweep:
            cmd.append("--sweep")
        p = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **env))
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print("child %s failed (exit %d):\n%s\n%s" % (child, p.returncode, p.stdout[-2000:], p.stderr[-4000:]), file=sys.stderr)
            return 1
        res = json.loads(line[0][7:])
        (record[group] if group else record)[name] = res
        print(child, json.dumps(res)[:600], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
