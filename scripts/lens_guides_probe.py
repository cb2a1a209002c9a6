"""Lens-sampled filter guides on one GPU:

  (a) cost at 1920 x 1080, scenes 3 and 1, fp32 and fp64, on an accumulation of 4 samples: rtiow_render_guides with the lens knob at 0, 2
      and 4 in RTIOW_GUIDES_FIRST_HIT, in RTIOW_GUIDES_SPECULAR at the wrapper's defaults and at 8 bounces with every metal a mirror, next
      to rtiow_render_coverage at 2 x 2 and 4 x 4 in the same process -- a kernel this feature leaves as it was
      (profiles/lens_guides/isa_diff_existing_kernels.txt) that traces the same number of primary rays with the same structure: the
      yardstick; HIP-event kernel times, medians of --runs after one warm-up;
  (b) quality at 320 x 180, 50 bounces, fp32, default sigmas, 5 levels, scenes 1 and 3, against a 1024-sample accumulation of the same
      camera: the linear MSE of the lens-guided denoise() over that of plain denoise() at 4, 16 and 64 samples for G = 2 and G = 4, over
      the whole frame and over the pixels whose circle of confusion exceeds 2 px (|1 - 1/depth| 2|U| / |du| from the first-hit depth; the
      sky counts as infinitely far), and the same ratio with resolve_edges() applied on top in both arms;
  (c) the same at 960 x 540 on scene 3, where the blur is three times wider;
  (d) the 8-frame orbit of tests/preview_drive.py at 4 samples a frame, 0.5 and 2 degrees a frame, clipped updates and plain commits: the
      lens-guided denoise_history() of the last frame over the plain one, of the same temporal image, against 1024 samples at the last camera.

The rule (fixed before anything was measured): the feature PAYS if the whole-frame ratio at G = 2 is below 1 on both scenes at 4 and 16
samples and on both orbit speeds.  Each part runs in a child process under its own `timeout`; the script stops at the first one that
fails.  Writes one JSON record (--out, default profiles/lens_guides/lens_guides_probe.json).

    python scripts/lens_guides_probe.py [--runs 7] [--out profiles/lens_guides/lens_guides_probe.json]
"""
import argparse
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
GRIDS = (2, 4)
ORBIT_SPEEDS = (0.5, 2.0)
REF_SAMPLES = 1024
COC_PX = 2.0


def _median(f, runs):
    f()                                                     # warm-up
    return statistics.median(f() for _ in range(runs))


def cost(scene_id, prec, runs):
    import raytracingincuda_amd as rt
    from tests.preview_drive import begin
    a = rt.api
    W, H, B = 1920, 1080, 50
    res = {}
    modes = (("first_hit", (a.GUIDES_FIRST_HIT,)), ("specular_default", (a.GUIDES_SPECULAR, a.GUIDE_MAX_BOUNCES, a.GUIDE_MAX_FUZZ)),
             ("specular_8_inf", (a.GUIDES_SPECULAR, 8, INF)))
    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, scene_id, rt.camera(prec, W, H, 1, B))
        r.accumulate(4)
        for name, mode in modes:
            r.set_guide_mode(*mode)
            for lens in (0,) + GRIDS:
                r.set_guide_lens(lens)
                res["render_guides_%s_lens%d_ms" % (name, lens)] = round(_median(lambda: r.render_guides(), runs), 4)
        for grid in GRIDS:
            res["render_coverage_%dx%d_ms" % (grid, grid)] = round(_median(lambda: r.render_coverage(grid), runs), 4)
        for grid in GRIDS:                                   # the added time in RTIOW_GUIDES_FIRST_HIT over the coverage render at the same G
            added = res["render_guides_first_hit_lens%d_ms" % grid] - res["render_guides_first_hit_lens0_ms"]
            res["added_over_coverage_%dx%d" % (grid, grid)] = round(added / res["render_coverage_%dx%d_ms" % (grid, grid)], 3)
    return res


def _coc_mask(np, cam, depth):
    """Pixels whose circle of confusion exceeds COC_PX pixels: |1 - 1/depth| 2|U| / |du| from the first-hit depth (in units of the primary
    ray, whose target lies on the focus plane); a miss is infinitely far."""
    U = np.array(cam.defocus_disk_u[:], np.float64); du = np.array(cam.pixel_delta_u[:], np.float64)
    scale = 2.0 * np.sqrt((U * U).sum()) / np.sqrt((du * du).sum())
    d = depth.astype(np.float64)
    with np.errstate(all="ignore"):
        inv = np.where(d > 0, 1.0 / d, 0.0)
    return np.abs(1.0 - inv) * scale > COC_PX


def _arms(np, r, cam, ref, filt):
    """{mse_plain, per G: ratio_frame, ratio_coc, ratio_frame_resolved} of the filter `filt(r)` (gamma-encoded image) with the knob off and on;
    cam: the handle's camera."""
    mse = lambda img, sel=None: float(np.mean(((img - ref) ** 2)[sel] if sel is not None else (img - ref) ** 2))
    lin = lambda g: g.astype(np.float64) ** 2
    r.set_guide_lens(0)
    plain = lin(filt(r))
    r.resolve_edges()
    plain_resolved = lin(r.read_denoised())
    coc = _coc_mask(np, cam, r.guides()[2])
    out = {"mse_plain": mse(plain), "coc_pixels_share": round(float(coc.mean()), 4), "resolved_plain_over_plain": round(mse(plain_resolved) / mse(plain), 4)}
    for G in GRIDS:
        r.set_guide_lens(G)
        img = lin(filt(r))
        r.resolve_edges()
        img_resolved = lin(r.read_denoised())
        out["g%d" % G] = {"ratio_frame": round(mse(img) / mse(plain), 4),
                          "ratio_coc": round(mse(img, coc) / mse(plain, coc), 4) if coc.any() else None,
                          "ratio_frame_resolved": round(mse(img_resolved) / mse(plain_resolved), 4)}
    r.set_guide_lens(0)
    return out


def quality(W, H, scenes):
    import numpy as np
    import raytracingincuda_amd as rt
    from tests.preview_drive import begin
    B, prec = 50, 32
    out = {}
    for scene_id in scenes:
        rec = {}
        cam = rt.camera(prec, W, H, 1, B)
        with rt.Renderer(0, prec) as r:
            begin(r, rt, prec, scene_id, cam)
            r.accumulate(REF_SAMPLES)
            ref = r.read_linear().astype(np.float64)
            for samples in SAMPLES:
                r.reset_accumulation()
                r.accumulate(samples)
                rec["%d_samples" % samples] = _arms(np, r, cam, ref, lambda r: r.denoise())
        out["scene%d" % scene_id] = rec
    return out


def orbit_quality():
    """clip_walk of tests/preview_drive.py; the last frame's temporal image filtered with the knob off and on."""
    import numpy as np
    import raytracingincuda_amd as rt
    from tests.preview_drive import begin, history_defaults, move, orbit, orbit_reference
    a = rt.api
    W, H, B, prec, frames, spp = 320, 180, 50, 32, 8, 4
    params = history_defaults(rt)
    out = {}
    for step_deg in ORBIT_SPEEDS:
        for scene_id in (1, 3):
            ref = orbit_reference(rt, scene_id, frames, step_deg, W, H, B, prec, REF_SAMPLES)
            cams = [rt.camera_look(prec, W, H, 1, B, lookfrom=orbit(step_deg * k)) for k in range(frames)]
            with rt.Renderer(0, prec) as r:
                begin(r, rt, prec, scene_id, cams[0])
                for k, cam in enumerate(cams):
                    move(r, cam, 1227 + k)
                    r.accumulate(spp)
                    r.history_update_clipped(a.HISTORY_CLIP_RADIUS, a.HISTORY_CLIP_GAMMA, *params)
                    if k < frames - 1:
                        r.history_commit()
                out["%.1f_deg_scene%d" % (step_deg, scene_id)] = _arms(np, r, cams[-1], ref, lambda r: r.denoise_history())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lens_guides", "lens_guides_probe.json"))
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        kind, *rest = a.child.split(",")
        if kind == "cost":
            res = cost(int(rest[0]), int(rest[1]), a.runs)
        elif kind == "quality":
            res = quality(320, 180, (1, 3))
        elif kind == "quality_wide":
            res = quality(960, 540, (3,))
        else:
            res = orbit_quality()
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    import raytracingincuda_amd as rt
    record = {"build_id": rt.build_id(), "frame_cost_1920x1080": {}, "runs": a.runs, "reference_samples": REF_SAMPLES, "coc_px": COC_PX}
    names = {"quality": "quality_320x180_b50_f32", "quality_wide": "quality_960x540_b50_f32", "orbit": "orbit_8_frames_4spp_320x180_b50_f32"}
    jobs = [("cost,%d,%d" % c, "scene%d_f%d" % c) for c in CONFIGS] + [(k, k) for k in names]
    for child, name in jobs:
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--child", child, "--runs", str(a.runs)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print("child %s failed (exit %d):\n%s\n%s" % (child, p.returncode, p.stdout[-2000:], p.stderr[-4000:]), file=sys.stderr)
            return 1
        res = json.loads(line[0][7:])
        if name in names:
            record[names[name]] = res
        else:
            record["frame_cost_1920x1080"][name] = res
        print(name, json.dumps(res)[:900], flush=True)
    q, o = record[names["quality"]], record[names["orbit"]]
    ratios = [q["scene%d" % sc]["%d_samples" % n]["g2"]["ratio_frame"] for sc in (1, 3) for n in (4, 16)]
    ratios += [o["%.1f_deg_scene%d" % (deg, sc)]["g2"]["ratio_frame"] for deg in ORBIT_SPEEDS for sc in (1, 3)]
    record["rule_ratios"] = ratios
    record["pays"] = all(x < 1 for x in ratios)
    record["rule"] = "whole-frame MSE ratio at G = 2 below 1 on scenes 1 and 3 at 4 and 16 samples and on both orbit speeds"
    print("pays:", record["pays"], ratios, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
