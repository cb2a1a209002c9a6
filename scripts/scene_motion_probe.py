"""Scene edits that keep the history on one GPU:

  (a) cost at 1920 x 1080, scenes 1 and 3, fp32 and fp64, on an accumulation of 4 samples, HIP-event kernel times, medians of --runs after
      one warm-up: rtiow_render_guides with motion in effect (guides + motion plane) beside the same call on a handle that has not edited
      (guides alone: a kernel this change leaves as it was), so the plane is the difference; rtiow_history_update,
      rtiow_history_update_clipped and rtiow_history_plan on the edited handle (the motion kernels) beside the same calls on the handle
      that has not edited (the existing kernels); and the host time of an edit: rtiow_edit_scene itself plus the table rebuild the next
      render reports (scene_prepare_ms);
  (b) --existing: the un-edited calls alone, three repeats of the medians, as one JSON line -- run once in this tree and once with --tree
      pointing at a built checkout of the parent commit, to state whether the existing paths are within the parent's own spread;
  (c) quality at 320 x 180, fp32, 50 bounces, scenes 1 and 3, against 1024 samples of the final frame: an 8-frame walk at 4 samples a
      frame in which the large lambertian sphere and eight small spheres translate by STEP a frame (about two pixels for the large one),
      once with a still camera and once with the 0.5 degree orbit, clipped updates at the defaults.  Arms: (a) rtiow_edit_scene; (b)
      rtiow_set_scene every frame, where the temporal image is the 4-sample frame; (c) on the host, tests/scene_motion_model.py from the
      planes read back with the base kept but Q = P (no compensation).  Reported: whole-frame MSE (a)/(b), and (a)/(c) over the pixels
      whose first hit is a moved sphere and over the disoccluded pixels.

The rule (fixed before anything was measured): the feature PAYS if (a)/(b) is below 1 on both scenes and both camera modes.  Each part
runs in a child process under its own `timeout`; the script stops at the first one that fails.  Writes one JSON record.

    python scripts/scene_motion_probe.py [--runs 7] [--out profiles/scene_motion/scene_motion_probe.json]
    python scripts/scene_motion_probe.py --existing [--tree /path/to/a/built/checkout]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(3, 32), (3, 64), (1, 32), (1, 64)]
CHILD_TIMEOUT_S = 300
STEP = (0.0, 0.0, 0.05)          # per frame: a pixel of the 320 x 180 frame spans about 0.027 at the large sphere, and z is across the view
FRAMES, SPP, REF_SAMPLES = 8, 4, 1024
CLIP = (1, 0.75)


def _median(f, runs):
    f()                                                     # warm-up
    return statistics.median(f() for _ in range(runs))


def _timed(r, name, *args, outs=1):
    """kernel_ms of the C call `name` on the handle of `r`: its float* kernel_ms, then `outs` uint64* the call also fills."""
    ms = ctypes.c_float(0)
    extra = [ctypes.c_uint64(0) for _ in range(outs)]
    rc = getattr(r._lib, name)(r._h, *args, ctypes.byref(ms), *[ctypes.byref(e) for e in extra])
    assert rc == 0, (name, rc)
    return ms.value


def _calls(rt, r, runs):
    d, n, m = rt.api.HISTORY_DEPTH_TOL, rt.api.HISTORY_NORMAL_COS, rt.api.HISTORY_MAX
    return {"render_guides_ms": _median(lambda: r.render_guides(), runs),
            "history_update_ms": _median(lambda: _timed(r, "rtiow_history_update", d, n, m), runs),
            "history_update_clipped_ms": _median(lambda: _timed(r, "rtiow_history_update_clipped", d, n, m, CLIP[0], CLIP[1], outs=2), runs),
            "history_plan_ms": _median(lambda: _timed(r, "rtiow_history_plan", d, n, m), runs)}


def _with_base(rt, prec, scene_id, W, H, B):
    """A handle with a base committed at the home view and 4 samples of the same view accumulated again."""
    from tests.preview_drive import begin
    r = rt.Renderer(0, prec)
    begin(r, rt, prec, scene_id, rt.camera(prec, W, H, 1, B))
    r.accumulate(4)
    r.history_update()
    r.history_commit()
    return r


def _moved(rt, prec, scene_id, frames=1):
    """The scene with the large lambertian sphere and eight small spheres translated by `frames` steps."""
    from tests import scene_motion_model as M
    import numpy as np
    scene = rt.build_scene(scene_id, prec)
    ty = np.asarray(scene["type"])
    big = [s for s in M.big_spheres(scene) if ty[s] == 0][:1]
    return scene, M.translate(scene, big + M.small_spheres(scene)[:8], tuple(frames * v for v in STEP))


def cost(scene_id, prec, runs):
    import raytracingincuda_amd as rt
    W, H, B = 1920, 1080, 50
    _, edit = _moved(rt, prec, scene_id)
    res = {}
    plain = _with_base(rt, prec, scene_id, W, H, B)
    try:
        plain.init_rng(1228)
        plain.accumulate(4)
        res["plain"] = {k: round(v, 4) for k, v in _calls(rt, plain, runs).items()}
    finally:
        plain.close()
    r = _with_base(rt, prec, scene_id, W, H, B)
    try:
        host = []
        for _ in range(runs):
            t0 = time.perf_counter()
            r.edit_scene(edit)
            host.append((time.perf_counter() - t0) * 1e3)
            r.render_guides()
        res["edit_scene_host_ms"] = round(statistics.median(host), 4)
        r.init_rng(1228)
        r.accumulate(4)
        res["scene_prepare_ms"] = round(r.stats()["scene_prepare_ms"], 4)
        res["motion"] = {k: round(v, 4) for k, v in _calls(rt, r, runs).items()}
        assert r._lib.rtiow_read_scene_motion(r._h, None, None, None, W * H) == 0       # the plane was rendered: motion was in effect
    finally:
        r.close()
    res["motion_plane_ms"] = round(res["motion"]["render_guides_ms"] - res["plain"]["render_guides_ms"], 4)
    res["plane_over_guides"] = round(res["motion_plane_ms"] / res["plain"]["render_guides_ms"], 3)
    for k in ("history_update_ms", "history_update_clipped_ms", "history_plan_ms"):
        res[k.replace("_ms", "_motion_over_plain")] = round(res["motion"][k] / res["plain"][k], 3)
    return res


def existing(runs):
    """The un-edited calls at 1920 x 1080 for every configuration, three repeats of the medians: what the parent commit has too."""
    import raytracingincuda_amd as rt
    out = {"build_id": rt.build_id()[:12]}
    for scene_id, prec in CONFIGS:
        r = _with_base(rt, prec, scene_id, 1920, 1080, 50)
        try:
            r.init_rng(1228)
            r.accumulate(4)
            out["scene%d_f%d" % (scene_id, prec)] = [{k: round(v, 4) for k, v in _calls(rt, r, runs).items()} for _ in range(3)]
        finally:
            r.close()
    return out


def quality(scene_id, orbit_deg):
    import numpy as np
    import raytracingincuda_amd as rt
    from tests import scene_motion_model as M
    from tests.oracle_lib import Oracle
    from tests.preview_drive import as_base, history_defaults, orbit, state
    prec, W, H, B = 32, 320, 180, 50
    params = history_defaults(rt)
    cams = [rt.camera_look(prec, W, H, 1, B, lookfrom=orbit(orbit_deg * k)) for k in range(FRAMES)]
    scenes = [_moved(rt, prec, scene_id, k)[1] for k in range(FRAMES)]
    with rt.Renderer(0, prec) as r:                          # the reference: 1024 samples of the final frame
        r.set_camera(cams[-1]); r.set_scene(scenes[-1]); r.init_rng(99)
        r.accumulate(REF_SAMPLES)
        ref = r.read_linear().astype(np.float64)
    mse = lambda img, sel=None: float(np.mean(((img.astype(np.float64) - ref) ** 2)[sel] if sel is not None else (img.astype(np.float64) - ref) ** 2))
    res = {}
    # arm (a): rtiow_edit_scene; the last frame's base and planes are kept for arm (c)
    with rt.Renderer(0, prec) as r:
        r.set_camera(cams[0]); r.set_scene(scenes[0])
        for k in range(FRAMES):
            if k:
                r.edit_scene(scenes[k])
            r.set_camera(cams[k]); r.init_rng(1227 + k)
            r.accumulate(SPP)
            if k == FRAMES - 1:
                base_rgb, base_len = r.history_base()
                cur = state(r, False)
                _, carry, ids = r.scene_motion()
            reprojected, clipped = r.history_update_clipped(*CLIP, *params)
            if k < FRAMES - 1:
                base_cur = state(r, False)
                r.history_commit()
        a_img = r.history()[0]
        noisy = r.read_linear()
    res["reprojected_pixels"], res["clipped_pixels"] = reprojected, clipped
    res["mse_a"], res["mse_noisy"] = mse(a_img), mse(noisy)
    # arm (b): rtiow_set_scene every frame empties the base: the temporal image of the last frame is its 4 samples
    with rt.Renderer(0, prec) as r:
        r.set_camera(cams[0])
        for k in range(FRAMES):
            r.set_scene(scenes[k]); r.set_camera(cams[k]); r.init_rng(1227 + k)
            r.accumulate(SPP)
            r.history_update_clipped(*CLIP, *params)
            if k < FRAMES - 1:
                r.history_commit()
        b_img = r.history()[0]
    res["mse_b"] = mse(b_img)
    res["a_over_b"] = res["mse_a"] / res["mse_b"]
    # arm (c): the base kept, no compensation (Q = P: the plain gather), on the host from the planes read back
    base = {"cam": cams[-2], "H": base_rgb, "M": base_len, "N": base_cur["N"], "z": base_cur["t"]}
    c_img = M.clipped_np(cams[-1], cur, base, params, *CLIP, None, None)["C"]
    want = M.clipped_np(cams[-1], cur, base, params, *CLIP, *_plane_of(M, Oracle(), prec, scenes, cams))
    res["model_agrees_with_arm_a"] = bool(np.array_equal(want["C"].view(np.uint8), a_img.view(np.uint8)))
    fl = M.flags(M.tables(scenes[-1], prec), M.tables(scenes[-2], prec))
    moved = (ids >= 0) & ((fl[np.maximum(ids, 0)] & M.MOVED) != 0)
    plain_m = M.gather_np(cams[-1], cur, base, *params)[1]
    disoccluded = (ids >= 0) & ~moved & (want["m"] == 0)
    res["moved_pixels"], res["disoccluded_pixels"] = int(moved.sum()), int(disoccluded.sum())
    res["mse_c"] = mse(c_img)
    res["a_over_c_moved"] = mse(a_img, moved) / mse(c_img, moved) if moved.any() else None
    res["a_over_c_disoccluded"] = mse(a_img, disoccluded) / mse(c_img, disoccluded) if disoccluded.any() else None
    res["uncompensated_carries_on_disoccluded"] = int((plain_m[disoccluded] > 0).sum())
    return res


def _plane_of(M, oracle, prec, scenes, cams):
    """(Q, carry) of the last frame against the scene of the frame before it, from the CPU oracle."""
    cur_t, snap = M.tables(scenes[-1], prec), M.tables(scenes[-2], prec)
    O, D, t, k = M.first_hit(oracle, prec, cur_t, cams[-1], range(cams[-1].img_height))
    Q, carry, _ = M.plane_np(O, D, t, k, cur_t, snap)
    return Q, carry


def _child(part, *args):
    cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--part", part] + [str(a) for a in args]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        sys.exit("%s %s failed (%d): %s" % (part, args, p.returncode, p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_motion", "scene_motion_probe.json"))
    ap.add_argument("--existing", action="store_true")
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
    out = {"runs": a.runs, "step": STEP, "frames": FRAMES, "spp": SPP, "ref_samples": REF_SAMPLES, "cost": {}, "quality": {}}
    for scene_id, prec in CONFIGS:
        out["cost"]["scene%d_f%d" % (scene_id, prec)] = _child("cost", scene_id, prec, a.runs)
    for scene_id in (1, 3):
        for name, deg in (("still", 0.0), ("orbit", 0.5)):
            out["quality"]["scene%d_%s" % (scene_id, name)] = _child("quality", scene_id, deg)
    ratios = [q["a_over_b"] for q in out["quality"].values()]
    out["verdict"] = {"rule": "(a)/(b) below 1 on both scenes and both camera modes", "a_over_b": ratios, "pays": all(x < 1 for x in ratios)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out["verdict"]))


if __name__ == "__main__":
    main()
