"""Edge resolve on one GPU:

  (a) cost at 1920 x 1080, scenes 3 and 1, fp32 and fp64, on an accumulation of 4 samples: rtiow_render_coverage at 2 x 2 and 4 x 4
      sub-samples, next to rtiow_render_guides and one level of rtiow_denoise (kernels this feature leaves as they were:
      profiles/edge_resolve/isa_diff_existing_kernels.txt), and rtiow_resolve_edges at radius 1, 2, 3 with current layers and guides
      after a 5-level rtiow_denoise; HIP-event kernel times, medians of --runs after one warm-up;
  (b) quality at 320 x 180, 50 bounces, fp32, scenes 1 and 3, against a 1024-sample accumulation: the linear MSE of the resolved
      denoise() over that of plain denoise() at 4, 16 and 64 samples, over the whole frame and over the mixed pixels alone, at the
      defaults of raytracingincuda_amd/api.py (tests/test_edge_resolve.py asks for < 1 at 4 and 16 samples);
  (c) --sweep: the whole-frame ratio of (b) over a grid of lattice, radius, sigmas and prior; the best setting is the one with the
      smallest worst case over the three sample counts and both scenes, first of equals in grid order;
  (d) the 8-frame orbit of tests/preview_drive.py at 4 samples a frame, 0.5 and 2 degrees a frame, clipped updates and plain commits:
      the resolved denoise_history() of the last frame over denoise_history() alone, against 1024 samples at the last camera.

The rule (fixed before anything was measured): the feature PAYS if the whole-frame ratio is below 1 on both scenes at 4 and 16 samples
and on both orbit speeds.  Each part runs in a child process under its own `timeout`; the script stops at the first one that fails.
Writes one JSON record (--out, default profiles/edge_resolve/edge_resolve_probe.json).

    python scripts/edge_resolve_probe.py [--runs 7] [--sweep] [--out profiles/edge_resolve/edge_resolve_probe.json]
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
CHILD_TIMEOUT_S = 300
INF = float("inf")
SAMPLES = (4, 16, 64)
SWEEP = {"grid": (4, 2), "radius": (1, 2, 3), "sigma_normal": (0.1, 0.3, 1.0, INF), "sigma_depth": (0.1, 0.5, 2.0, INF), "prior": (2.0, 8.0, 32.0, INF)}
ORBIT_SPEEDS = (0.5, 2.0)


def _median(f, runs):
    f()                                                     # warm-up
    return statistics.median(f() for _ in range(runs))


def _defaults(api):
    return {"grid": api.COVERAGE_GRID, "radius": api.EDGE_RADIUS, "sigma_normal": api.EDGE_SIGMA_NORMAL, "sigma_depth": api.EDGE_SIGMA_DEPTH,
            "prior": api.EDGE_PRIOR}


def cost(scene_id, prec, runs):
    import raytracingincuda_amd as rt
    a = rt.api
    W, H, B = 1920, 1080, 50
    res = {}
    with rt.Renderer(0, prec) as r:
        r.set_camera(rt.camera(prec, W, H, 1, B))
        r.set_scene(rt.build_scene(scene_id, prec))
        r.init_rng(1227)
        r.accumulate(4)
        res["render_guides_ms"] = round(_median(lambda: r.render_guides(), runs), 4)

        def den(levels):
            ms = ctypes.c_float(0)
            r._check(r._lib.rtiow_denoise(r._h, levels, a.DENOISE_SIGMA_COLOR, a.DENOISE_SIGMA_NORMAL, a.DENOISE_SIGMA_ALBEDO, a.DENOISE_SIGMA_DEPTH,
                                          ctypes.byref(ms)))
            return ms.value
        res["denoise_1_level_ms"] = round(_median(lambda: den(1), runs), 4)
        res["denoise_5_levels_ms"] = round(_median(lambda: den(5), runs), 4)
        for grid in (2, 4):
            res["render_coverage_%dx%d_ms" % (grid, grid)] = round(_median(lambda: r.render_coverage(grid), runs), 4)
        ids = r.coverage()[0]
        res["mixed_pixels_4x4"] = int((ids[..., 1] != -2).sum())

        def resolve(radius):                                 # layers and guides are current: the resolve alone
            den(5)
            ms, n = ctypes.c_float(0), ctypes.c_uint64(0)
            r._check(r._lib.rtiow_resolve_edges(r._h, radius, a.EDGE_SIGMA_NORMAL, a.EDGE_SIGMA_DEPTH, a.EDGE_PRIOR, ctypes.byref(ms), ctypes.byref(n)))
            res["resolved_pixels"] = int(n.value)
            return ms.value
        for radius in (1, 2, 3):
            res["resolve_edges_r%d_ms" % radius] = round(_median(lambda: resolve(radius), runs), 4)
    return res


def quality(sweep):
    import numpy as np
    import raytracingincuda_amd as rt
    W, H, B, prec = 320, 180, 50, 32
    default = _defaults(rt.api)
    combos = [dict(zip(SWEEP, v)) for v in itertools.product(*SWEEP.values())] if sweep else []
    out = {"defaults": default}
    for scene_id in (1, 3):
        rec = {}
        with rt.Renderer(0, prec) as r:
            r.set_camera(rt.camera(prec, W, H, 1, B)); r.set_scene(rt.build_scene(scene_id, prec)); r.init_rng(1227)
            r.accumulate(1024)
            ref = r.read_linear().astype(np.float64)
            for samples in SAMPLES:
                r.reset_accumulation()
                r.accumulate(samples)
                noisy = r.read_linear().astype(np.float64)
                plain = r.denoise().astype(np.float64) ** 2
                mse = lambda img, sel=None: float(np.mean(((img - ref) ** 2)[sel] if sel is not None else (img - ref) ** 2))

                def resolved(c):
                    if r.render_coverage(c["grid"]) is None:
                        raise RuntimeError("no layers")
                    r.denoise()
                    n = r.resolve_edges(c["radius"], c["sigma_normal"], c["sigma_depth"], c["prior"])
                    return r.read_denoised().astype(np.float64) ** 2, n
                img, n = resolved(default)
                mixed = r.coverage()[0][..., 1] != -2
                s = {"mse_noisy": mse(noisy), "mse_denoise": mse(plain), "ratio_frame": round(mse(img) / mse(plain), 4),
                     "ratio_mixed": round(mse(img, mixed) / mse(plain, mixed), 4), "mixed_pixels": int(mixed.sum()), "resolved_pixels": n,
                     "mixed_share_of_denoise_error": round(mse(plain, mixed) * mixed.mean() / mse(plain), 4),
                     "mixed_denoised_over_noisy": round(mse(plain, mixed) / mse(noisy, mixed), 4),
                     "mixed_resolved_over_noisy": round(mse(img, mixed) / mse(noisy, mixed), 4)}
                if sweep:
                    s["sweep"] = [round(mse(resolved(c)[0]) / mse(plain), 4) for c in combos]
                rec["%d_samples" % samples] = s
        out["scene%d" % scene_id] = rec
    if sweep:                                               # the smallest worst case over sample counts and scenes, first of equals
        worst = [max(out["scene%d" % sc]["%d_samples" % n]["sweep"][k] for sc in (1, 3) for n in SAMPLES) for k in range(len(combos))]
        k = min(range(len(combos)), key=worst.__getitem__)
        out["sweep_grid"] = {name: list(v) for name, v in SWEEP.items()}
        out["sweep_best"] = dict(combos[k], worst_ratio=worst[k])
        kd = [i for i, c in enumerate(combos) if c == default]
        if kd:
            out["sweep_default_worst_ratio"] = worst[kd[0]]
        for grid in SWEEP["grid"]:                          # the best of each lattice, for the choice between 2 x 2 and 4 x 4
            ks = [i for i, c in enumerate(combos) if c["grid"] == grid]
            kb = min(ks, key=worst.__getitem__)
            out["sweep_best_grid_%d" % grid] = dict(combos[kb], worst_ratio=worst[kb],
                                                    ratios={"scene%d_%d" % (sc, n): out["scene%d" % sc]["%d_samples" % n]["sweep"][kb] for sc in (1, 3) for n in SAMPLES})
    return out


def orbit_quality():
    """clip_walk of tests/preview_drive.py with the last frame's denoise_history() resolved."""
    import numpy as np
    import raytracingincuda_amd as rt
    from tests.preview_drive import begin, history_defaults, move, orbit, orbit_reference
    a = rt.api
    W, H, B, prec, frames, spp = 320, 180, 50, 32, 8, 4
    params = history_defaults(rt)
    out = {}
    for step_deg in ORBIT_SPEEDS:
        for scene_id in (1, 3):
            ref = orbit_reference(rt, scene_id, frames, step_deg, W, H, B, prec)
            cams = [rt.camera_look(prec, W, H, 1, B, lookfrom=orbit(step_deg * k)) for k in range(frames)]
            with rt.Renderer(0, prec) as r:
                begin(r, rt, prec, scene_id, cams[0])
                for k, cam in enumerate(cams):
                    move(r, cam, 1227 + k)
                    r.accumulate(spp)
                    r.history_update_clipped(a.HISTORY_CLIP_RADIUS, a.HISTORY_CLIP_GAMMA, *params)
                    if k < frames - 1:
                        r.history_commit()
                plain = r.denoise_history().astype(np.float64) ** 2
                n = r.resolve_edges()
                img = r.read_denoised().astype(np.float64) ** 2
                mixed = r.coverage()[0][..., 1] != -2
            mse = lambda x, sel=None: float(np.mean(((x - ref) ** 2)[sel] if sel is not None else (x - ref) ** 2))
            out["%.1f_deg_scene%d" % (step_deg, scene_id)] = {"mse_denoise_history": mse(plain), "ratio_frame": round(mse(img) / mse(plain), 4),
                                                              "ratio_mixed": round(mse(img, mixed) / mse(plain, mixed), 4), "resolved_pixels": n}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edge_resolve", "edge_resolve_probe.json"))
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        kind, *rest = a.child.split(",")
        res = cost(int(rest[0]), int(rest[1]), a.runs) if kind == "cost" else quality(a.sweep) if kind == "quality" else orbit_quality()
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    import raytracingincuda_amd as rt
    record = {"build_id": rt.build_id(), "frame_cost_1920x1080": {}, "runs": a.runs}
    jobs = [("cost,%d,%d" % c, "scene%d_f%d" % c) for c in CONFIGS] + [("quality", "quality"), ("orbit", "orbit")]
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
        elif name == "orbit":
            record["orbit_8_frames_4spp_320x180_b50_f32"] = res
        else:
            record["frame_cost_1920x1080"][name] = res
        print(name, json.dumps(res)[:600], flush=True)
    q, o = record["quality_320x180_b50_f32"], record["orbit_8_frames_4spp_320x180_b50_f32"]
    ratios = [q["scene%d" % sc]["%d_samples" % n]["ratio_frame"] for sc in (1, 3) for n in (4, 16)] + [v["ratio_frame"] for v in o.values()]
    record["pays"] = all(x < 1 for x in ratios)
    record["rule"] = "whole-frame MSE ratio below 1 on scenes 1 and 3 at 4 and 16 samples and on both orbit speeds"
    print("pays:", record["pays"], ratios, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
