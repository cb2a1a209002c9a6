"""Edit influence on one GPU:

  (a) payoff at 320 x 180, fp32, 50 bounces, scenes 1 and 3, against 1024 samples of the final frame: the 8-frame walk of
      scripts/scene_motion_probe.py (the large lambertian sphere and eight small spheres translate by STEP a frame), once with a still
      camera and once with the 0.5 degree orbit.  Every frame: rtiow_edit_scene, the plan, budget chunks of SPP samples with at least SPP
      a pixel until nobody is below the target, the clipped update at the defaults, the commit.  For every kappa of SWEEP: the whole-frame
      MSE and the MSE over the influenced pixels -- an unedited first hit and s > 0 in tests/edit_influence_model.py -- of the last frame's
      temporal image, and the primary rays of the whole walk, each as a ratio to the same walk at kappa == 0 in the same build;
  (b) cost at 1920 x 1080, scenes 1 and 3, fp32 and fp64, HIP-event kernel times, medians of --runs after one warm-up: rtiow_render_guides
      on a handle that has not edited (guides), on an edited handle at kappa == 0 (+ surface_motion_kernel) and at kappa == 1 with 2, 18 and
      88 entries in the edit list (+ edit_influence_kernel), so each kernel is a difference of two medians of the same run; and
      rtiow_history_update, rtiow_history_update_clipped and rtiow_history_plan on the edited handle at kappa == 0 and at kappa == 1;
  (c) --existing: the three motion calls at kappa == 0 alone, three repeats of the medians, as one JSON line -- run once in this tree and
      once with --tree pointing at a built checkout of the parent commit.

The rule (fixed before anything was measured): the feature PAYS if one kappa, the same for all four walks, brings the whole-frame ratio
below 1 on both scenes and both camera modes with no more than 1.10 x the rays.  The best kappa by that rule is the one with the smallest
worst-of-four whole-frame ratio among those within the ray bound.  Each part runs in a child process under its own `timeout`; the script
stops at the first one that fails.  Writes one JSON record.

    python scripts/edit_influence_probe.py [--runs 7] [--out profiles/edit_influence/edit_influence_probe.json]
    python scripts/edit_influence_probe.py --existing [--tree /path/to/a/built/checkout]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(3, 32), (3, 64), (1, 32), (1, 64)]
CHILD_TIMEOUT_S = 400
STEP = (0.0, 0.0, 0.05)
FRAMES, SPP, REF_SAMPLES = 8, 4, 1024
SWEEP = (0.0, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0, float("inf"))
RAY_BOUND = 1.10
ENTRY_CASES = (1, 9, 44)         # spheres moved: 2, 18 and 88 entries


def _median(f, runs):
    f()                                                     # warm-up
    return statistics.median(f() for _ in range(runs))


def _timed(r, name, *args, outs=1):
    ms = ctypes.c_float(0)
    extra = [ctypes.c_uint64(0) for _ in range(outs)]
    rc = getattr(r._lib, name)(r._h, *args, ctypes.byref(ms), *[ctypes.byref(e) for e in extra])
    assert rc == 0, (name, rc)
    return ms.value


def _calls(rt, r, runs, guides=True):
    a = rt.api
    d, n, m = a.HISTORY_DEPTH_TOL, a.HISTORY_NORMAL_COS, a.HISTORY_MAX
    out = {"history_update_ms": _median(lambda: _timed(r, "rtiow_history_update", d, n, m), runs),
           "history_update_clipped_ms": _median(lambda: _timed(r, "rtiow_history_update_clipped", d, n, m, a.HISTORY_CLIP_RADIUS, a.HISTORY_CLIP_GAMMA, outs=2), runs),
           "history_plan_ms": _median(lambda: _timed(r, "rtiow_history_plan", d, n, m), runs)}
    if guides:
        out["render_guides_ms"] = _median(lambda: r.render_guides(), runs)
    return {k: round(v, 4) for k, v in out.items()}


def _with_base(rt, prec, scene_id, W, H, B):
    from tests.preview_drive import begin
    r = rt.Renderer(0, prec)
    begin(r, rt, prec, scene_id, rt.camera(prec, W, H, 1, B))
    r.accumulate(4)
    r.history_update()
    r.history_commit()
    return r


def _walk_scene(rt, prec, scene_id, frames=1):
    """The scene with the large lambertian sphere and eight small spheres translated by `frames` steps."""
    import numpy as np
    from tests import scene_motion_model as M
    scene = rt.build_scene(scene_id, prec)
    ty = np.asarray(scene["type"])
    big = [s for s in M.big_spheres(scene) if ty[s] == 0][:1]
    return M.translate(scene, big + M.small_spheres(scene)[:8], tuple(frames * v for v in STEP))


def _edited_handle(rt, prec, scene_id, moved):
    from tests import scene_motion_model as M
    scene = rt.build_scene(scene_id, prec)
    r = _with_base(rt, prec, scene_id, 1920, 1080, 50)
    r.edit_scene(M.translate(scene, M.small_spheres(scene)[:moved], STEP))
    r.init_rng(1228)
    r.accumulate(4)
    return r


def cost(scene_id, prec, runs):
    import raytracingincuda_amd as rt
    res = {}
    plain = _with_base(rt, prec, scene_id, 1920, 1080, 50)
    try:
        plain.init_rng(1228)
        plain.accumulate(4)
        res["guides_ms"] = round(_median(lambda: plain.render_guides(), runs), 4)
    finally:
        plain.close()
    for moved in ENTRY_CASES:
        r = _edited_handle(rt, prec, scene_id, moved)
        try:
            off = _calls(rt, r, runs)
            r.set_edit_influence(1.0)
            on = _calls(rt, r, runs)
            assert r._lib.rtiow_read_edit_influence(r._h, None, 1920 * 1080) == 0       # the plane was made
        finally:
            r.close()
        motion = off["render_guides_ms"] - res["guides_ms"]
        influence = on["render_guides_ms"] - off["render_guides_ms"]
        res["entries_%d" % (2 * moved)] = {"kappa_0": off, "kappa_1": on, "surface_motion_kernel_ms": round(motion, 4), "edit_influence_kernel_ms": round(influence, 4),
                                           "influence_over_motion": round(influence / motion, 3) if motion > 0 else None}
    return res


def existing(runs):
    """The three motion calls at kappa == 0 (an edited handle, nine spheres moved) at 1920 x 1080, three repeats of the medians."""
    import raytracingincuda_amd as rt
    out = {"build_id": rt.build_id()[:12]}
    for scene_id, prec in CONFIGS:
        r = _edited_handle(rt, prec, scene_id, 9)
        try:
            out["scene%d_f%d" % (scene_id, prec)] = [_calls(rt, r, runs, guides=False) for _ in range(3)]
        finally:
            r.close()
    return out


def quality(scene_id, orbit_deg):
    import numpy as np
    import raytracingincuda_amd as rt
    from tests import edit_influence_model as E
    from tests import scene_motion_model as M
    from tests.preview_drive import history_defaults, orbit
    prec, W, H, B = 32, 320, 180, 50
    a = rt.api
    params = history_defaults(rt)
    clip = (a.HISTORY_CLIP_RADIUS, a.HISTORY_CLIP_GAMMA)
    cams = [rt.camera_look(prec, W, H, 1, B, lookfrom=orbit(orbit_deg * k)) for k in range(FRAMES)]
    scenes = [_walk_scene(rt, prec, scene_id, k) for k in range(FRAMES)]
    with rt.Renderer(0, prec) as r:                          # the reference: 1024 samples of the final frame
        r.set_camera(cams[-1]); r.set_scene(scenes[-1]); r.init_rng(99)
        r.accumulate(REF_SAMPLES)
        ref = r.read_linear().astype(np.float64)
    mse = lambda img, sel=None: float(np.mean(((img.astype(np.float64) - ref) ** 2)[sel] if sel is not None else (img.astype(np.float64) - ref) ** 2))
    res = {}
    for kappa in SWEEP:
        rays = 0
        with rt.Renderer(0, prec) as r:
            r.set_edit_influence(kappa)
            r.set_camera(cams[0]); r.set_scene(scenes[0])
            for k in range(FRAMES):
                if k:
                    r.edit_scene(scenes[k])
                r.set_camera(cams[k]); r.init_rng(1227 + k)
                r.history_plan(*params)
                while True:
                    active = r.accumulate_budget(SPP, a.BUDGET_TARGET, SPP)[1]
                    rays += r.stats()["primary_rays"]
                    if not active:
                        break
                if k == FRAMES - 1:
                    ids = r.scene_motion()[2]
                    depth = r.guides()[2]
                r.history_update_clipped(*clip, *params)
                if k < FRAMES - 1:
                    r.history_commit()
            img = r.history()[0]
        cur_t, snap = M.tables(scenes[-1], prec), M.tables(scenes[-2], prec)
        entries, owners = E.edit_list(cur_t, snap)
        fl = M.flags(cur_t, snap)
        carry = np.where((ids >= 0) & ((fl[np.maximum(ids, 0)] & M.CHANGED) != 0), 0, 1).astype(np.int32)    # the same mask in every arm
        _, _, s = E.influence_np(cams[-1], depth, carry, ids, entries, owners, 1.0)
        influenced = (ids >= 0) & (fl[np.maximum(ids, 0)] == 0) & (s > 0)
        res[str(kappa)] = {"mse": mse(img), "mse_influenced": mse(img, influenced), "influenced_pixels": int(influenced.sum()), "rays": int(rays)}
    zero = res["0.0"]
    for v in res.values():
        v["frame_ratio"] = v["mse"] / zero["mse"]
        v["influenced_ratio"] = v["mse_influenced"] / zero["mse_influenced"]
        v["rays_ratio"] = v["rays"] / zero["rays"]
    return res


def verdict(quality_by_walk):
    """The rule of the docstring over {walk: {kappa: ...}}."""
    rows = {}
    for kappa in SWEEP[1:]:
        key = str(kappa)
        frame = [w[key]["frame_ratio"] for w in quality_by_walk.values()]
        rays = [w[key]["rays_ratio"] for w in quality_by_walk.values()]
        rows[key] = {"worst_frame_ratio": max(frame), "worst_rays_ratio": max(rays), "within_rays": max(rays) <= RAY_BOUND,
                     "meets_rule": max(frame) < 1 and max(rays) <= RAY_BOUND}
    allowed = [k for k in rows if rows[k]["within_rays"]]
    best = min(allowed, key=lambda k: rows[k]["worst_frame_ratio"]) if allowed else None
    return {"rule": "one kappa for all four walks: whole-frame ratio below 1 everywhere at no more than %.2f x the rays" % RAY_BOUND, "by_kappa": rows,
            "best_kappa": best, "pays": bool(best is not None and rows[best]["meets_rule"])}


def _child(part, *args):
    cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--part", part] + [str(a) for a in args]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        sys.exit("%s %s failed (%d): %s" % (part, args, p.returncode, p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_influence", "edit_influence_probe.json"))
    ap.add_argument("--existing", action="store_true")
    ap.add_argument("--skip-cost", action="store_true")
    ap.add_argument("--tree", default=ROOT, help="the built checkout whose package and tests are imported (--existing: e.g. the parent commit's)")
    ap.add_argument("--part", default="")
    ap.add_argument("args", nargs="*")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    if a.part == "cost":
        print(json.dumps(cost(int(a.args[0]), int(a.args[1]), int(a.args[2]))))
        return
    if a.part == "quality":
        print(json.dumps(quality(int(a.args[0]), float(a.args[1]))))
        return
    if a.existing:
        print(json.dumps(existing(a.runs)))
        return
    out = {"runs": a.runs, "step": STEP, "frames": FRAMES, "spp": SPP, "ref_samples": REF_SAMPLES, "sweep": [str(k) for k in SWEEP], "cost": {}, "quality": {}}
    for scene_id in (1, 3):
        for name, deg in (("still", 0.0), ("orbit", 0.5)):
            out["quality"]["scene%d_%s" % (scene_id, name)] = _child("quality", scene_id, deg)
            print("quality scene%d_%s done" % (scene_id, name), flush=True)
    out["verdict"] = verdict(out["quality"])
    if not a.skip_cost:
        for scene_id, prec in CONFIGS:
            out["cost"]["scene%d_f%d" % (scene_id, prec)] = _child("cost", scene_id, prec, a.runs)
            print("cost scene%d_f%d done" % (scene_id, prec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out["verdict"]))


if __name__ == "__main__":
    main()
