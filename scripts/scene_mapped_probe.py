"""Scene edits that add and remove spheres on one GPU:

  (a) payoff at 320 x 180, fp32, 50 bounces, scenes 1 and 3, against 1024 samples of the final frame: the 8-frame walk of
      scripts/scene_motion_probe.py (the large lambertian sphere and eight small spheres translate by STEP a frame), once with a still
      camera and once with the 0.5 degree orbit, in which every frame after the first also removes the small sphere the previous frame
      showed most of (not one of the nine) and adds one on the ground elsewhere.  Every frame: the edit, the plan, budget chunks of SPP
      samples with at least SPP a pixel until nobody is below the target, the clipped update at the defaults, the commit.  Arm (a):
      rtiow_edit_scene_mapped; arm (b): rtiow_set_scene every frame, which restarts the history.  Reported: the MSE of the last
      temporal image as (a)/(b) over the whole frame, over the pixels the removals uncover and over the pixels the additions cover (of
      the last frame's edit, and of all seven), and the primary rays of the whole walk as (a)/(b);
  (b) --cost: the host time of one call, median of --runs after a warm-up, on a handle with a base at 320 x 180, scenes 1 and 3, fp32 and
      fp64, through ctypes on the library itself: rtiow_edit_scene and rtiow_edit_scene_mapped under the identity map with the same
      tables (the walk's first step), alternately.  --library names another build of the C-ABI (the parent commit's, which has
      rtiow_edit_scene only); the two are run in one job and compared.

The rule (fixed before anything was measured): the feature PAYS if the whole-frame ratio is below 1 on both scenes and both camera modes
at no more than 1.10 x the restart walk's rays.  Each walk runs in a child process under its own `timeout`; the script stops at the first
one that fails.  Writes one JSON record.

    python scripts/scene_mapped_probe.py [--out profiles/scene_mapped/scene_mapped_probe.json]
    python scripts/scene_mapped_probe.py --cost [--runs 21] [--library /path/to/librtiow_hip.so]
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
sys.path.insert(0, ROOT)
CONFIGS = [(3, 32), (3, 64), (1, 32), (1, 64)]
CHILD_TIMEOUT_S = 400
STEP = (0.0, 0.0, 0.05)
FRAMES, SPP, REF_SAMPLES = 8, 4, 1024
RAY_BOUND = 1.10


def _nine(rt, scene):
    import numpy as np
    from tests import scene_motion_model as M
    ty = np.asarray(scene["type"])
    return [s for s in M.big_spheres(scene) if ty[s] == 0][:1] + M.small_spheres(scene)[:8]


def walk_scenes(rt, oracle, prec, scene_id, cams):
    """[(scene, origin, removed slot, added slot)] per frame.  Slots never move: a removal marks its slot invalid, an addition appends one,
    so origin is the identity over the previous frame's slots and -1 for the new one."""
    import numpy as np
    from tests import scene_mapped_model as S
    from tests import scene_motion_model as M
    scene = S.with_valid(rt.build_scene(scene_id, prec))
    nine = _nine(rt, scene)
    frames = [(scene, None, None, None)]
    for k in range(1, len(cams)):
        prev = frames[-1][0]
        tb = M.tables(prev, prec)
        O, D, t, ids = M.first_hit(oracle, prec, tb, cams[k - 1], range(cams[k - 1].img_height))
        kept = [int(s) for s in M.kept_slots(prev)]
        r = np.asarray(prev["center_radius"], np.float64).reshape(-1, 4)[:, 3]
        shown = np.bincount(ids[ids >= 0], minlength=len(kept))
        candidates = [s for s in M.small_spheres(prev) if s not in nine and s < len(scene["type"])]
        victim = max(candidates, key=lambda s: (int(shown[kept.index(s)]), -s))
        assert shown[kept.index(victim)] > 0
        # the new sphere stands on the ground where a ground pixel of the previous frame looks, the pixels taken in turn across the frame
        ground = np.argwhere((ids >= 0) & (r[np.asarray(kept)][np.maximum(ids, 0)] >= 100))
        y, x = ground[(len(ground) * (2 * k + 1)) // (2 * len(cams))]
        P = np.asarray(O, np.float64) + float(t[y, x]) * np.asarray(D[y, x], np.float64)
        moved = M.translate(prev, nine, STEP)
        step, _ = S.drop(moved, [victim])
        step, origin = S.append(step, [[P[0], 0.2, P[2], 0.2]], [[0.5, 0.25, 0.125, 0.0]], [1.5], [0])
        frames.append((step, origin, victim, len(step["type"]) - 1))
    return frames


def quality(scene_id, orbit_deg):
    import numpy as np
    import raytracingincuda_amd as rt
    from tests import scene_mapped_model as S
    from tests import scene_motion_model as M
    from tests.oracle_lib import Oracle
    from tests.preview_drive import history_defaults, orbit
    prec, W, H, B = 32, 320, 180, 50
    a = rt.api
    params = history_defaults(rt)
    clip = (a.HISTORY_CLIP_RADIUS, a.HISTORY_CLIP_GAMMA)
    oracle = Oracle()
    cams = [rt.camera_look(prec, W, H, 1, B, lookfrom=orbit(orbit_deg * k)) for k in range(FRAMES)]
    frames = walk_scenes(rt, oracle, prec, scene_id, cams)
    with rt.Renderer(0, prec) as r:                          # the reference: 1024 samples of the final frame
        r.set_camera(cams[-1]); r.set_scene(frames[-1][0]); r.init_rng(99)
        r.accumulate(REF_SAMPLES)
        ref = r.read_linear().astype(np.float64)
    mse = lambda img, sel=None: float(np.mean(((img.astype(np.float64) - ref) ** 2)[sel] if sel is not None else (img.astype(np.float64) - ref) ** 2))
    res = {}
    for arm in ("mapped", "restart"):
        rays = 0
        with rt.Renderer(0, prec) as r:
            r.set_camera(cams[0]); r.set_scene(frames[0][0])
            for k in range(FRAMES):
                if k and arm == "mapped":
                    r.edit_scene_mapped(frames[k][0], frames[k][1])
                elif k:
                    r.set_scene(frames[k][0])
                r.set_camera(cams[k]); r.init_rng(1227 + k)
                r.history_plan(*params)
                while True:
                    active = r.accumulate_budget(SPP, a.BUDGET_TARGET, SPP)[1]
                    rays += r.stats()["primary_rays"]
                    if not active:
                        break
                if k == FRAMES - 1 and arm == "mapped":
                    ids = r.scene_motion()[2]
                    plan = r.history_plan_lengths()
                    origin_read = r.scene_origin()
                reprojected, clipped = r.history_update_clipped(*clip, *params)
                if k < FRAMES - 1:
                    r.history_commit()
            res[arm] = {"img": r.history()[0], "rays": int(rays), "reprojected": int(reprojected), "clipped": int(clipped)}
    # the pixel sets, at the last camera: what the last frame's removal uncovers and its addition covers, and the same of all seven edits
    last, before = frames[-1][0], frames[-2][0]
    number = lambda scene, slot: [int(s) for s in M.kept_slots(scene)].index(int(slot))
    _, _, _, k_before = M.first_hit(oracle, prec, M.tables(M.translate(before, _nine(rt, before), STEP), prec), cams[-1], range(H))
    uncovered = k_before == number(before, frames[-1][2])
    covered = ids == number(last, frames[-1][3])
    everything = dict(last, valid=np.where(np.isin(np.arange(len(last["type"])), [f[2] for f in frames[1:]]), 1, last["valid"]).astype(np.int32))
    _, _, _, k_all = M.first_hit(oracle, prec, M.tables(everything, prec), cams[-1], range(H))
    uncovered_any = np.isin(k_all, [number(everything, f[2]) for f in frames[1:]])
    covered_any = np.isin(ids, [number(last, f[3]) for f in frames[1:]])
    assert origin_read[number(last, frames[-1][3])] == -1 and (origin_read >= 0).sum() == len(origin_read) - 1
    out = {"rays_mapped": res["mapped"]["rays"], "rays_restart": res["restart"]["rays"], "rays_ratio": res["mapped"]["rays"] / res["restart"]["rays"],
           "reprojected_pixels": res["mapped"]["reprojected"], "clipped_pixels": res["mapped"]["clipped"]}
    for name, sel in (("frame", None), ("uncovered", uncovered), ("covered", covered), ("uncovered_all_edits", uncovered_any), ("covered_all_edits", covered_any)):
        n = W * H if sel is None else int(sel.sum())
        ma, mb = (mse(res[arm]["img"], sel) if n else None for arm in ("mapped", "restart"))
        out[name] = {"pixels": n, "mse_mapped": ma, "mse_restart": mb, "ratio": ma / mb if n and mb else None}
        if sel is not None and n:
            out[name]["without_history"] = int((plan[sel] == 0).sum())
    return out


# ---- the cost of the call, through ctypes on the library itself (the parent commit's library has no rtiow_edit_scene_mapped)

def cost(library, scene_id, prec, runs):
    import numpy as np
    import raytracingincuda_amd as rt
    from tests import scene_motion_model as M
    lib = ctypes.CDLL(library)
    dt = np.float32 if prec == 32 else np.float64
    i32p, vp = ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p
    scene_args = (vp, ctypes.c_int, vp, vp, vp, i32p, i32p)
    lib.rtiow_create.argtypes = (ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp))
    for name, args in (("rtiow_set_camera", (vp, vp)), ("rtiow_set_scene", scene_args), ("rtiow_edit_scene", scene_args), ("rtiow_init_rng", (vp, ctypes.c_uint64)),
                       ("rtiow_accumulate", (vp, ctypes.c_int, ctypes.c_int, vp)), ("rtiow_history_update", (vp, ctypes.c_double, ctypes.c_double, ctypes.c_double, vp, vp)),
                       ("rtiow_history_commit", (vp,)), ("rtiow_render_guides", (vp, vp)), ("rtiow_destroy", (vp,))):
        getattr(lib, name).argtypes = args
    mapped = hasattr(lib, "rtiow_edit_scene_mapped")
    if mapped:
        lib.rtiow_edit_scene_mapped.argtypes = scene_args + (i32p,)
    scene = rt.build_scene(scene_id, prec)
    edit = M.translate(scene, _nine(rt, scene), STEP)
    cam = rt.camera(prec, 320, 180, 1, 50)

    def tables(sc):
        keep = [np.ascontiguousarray(sc["center_radius"], dt), np.ascontiguousarray(sc["albedo_fuzz"], dt), np.ascontiguousarray(sc["refraction_index"], dt),
                np.ascontiguousarray(sc["type"], np.int32), np.ascontiguousarray(sc["valid"], np.int32)]
        return keep, (len(keep[3]), keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data, keep[3].ctypes.data_as(i32p), keep[4].ctypes.data_as(i32p))
    keep0, args0 = tables(scene)
    keep1, args1 = tables(edit)
    origin = np.arange(len(scene["type"]), dtype=np.int32)
    h = vp()
    ok = lambda rc: rc == 0 or sys.exit("call failed: %d" % rc)
    ok(lib.rtiow_create(0, prec, ctypes.byref(h)))
    try:
        ok(lib.rtiow_set_camera(h, ctypes.addressof(cam))); ok(lib.rtiow_set_scene(h, *args0)); ok(lib.rtiow_init_rng(h, 1227))
        ok(lib.rtiow_accumulate(h, 4, 0, None)); ok(lib.rtiow_history_update(h, rt.api.HISTORY_DEPTH_TOL, rt.api.HISTORY_NORMAL_COS, rt.api.HISTORY_MAX, None, None))
        ok(lib.rtiow_history_commit(h))
        calls = {"rtiow_edit_scene": lambda: lib.rtiow_edit_scene(h, *args1)}
        if mapped:
            calls["rtiow_edit_scene_mapped"] = lambda: lib.rtiow_edit_scene_mapped(h, *args1, origin.ctypes.data_as(i32p))
        times = {name: [] for name in calls}
        for rep in range(runs + 1):                          # the first round is the warm-up; the calls alternate
            for name, call in calls.items():
                t0 = time.perf_counter()
                ok(call())
                t1 = time.perf_counter()
                if rep:
                    times[name].append((t1 - t0) * 1e3)
                ok(lib.rtiow_render_guides(h, None))           # the plane of this edit reads the tables the next edit replaces
        out = {}
        for name, ts in times.items():
            ts.sort()
            out[name + "_host_ms"] = {"median": round(statistics.median(ts), 4), "min": round(ts[0], 4), "quartiles": [round(ts[len(ts) // 4], 4), round(ts[(3 * len(ts)) // 4], 4)]}
        return out
    finally:
        lib.rtiow_destroy(h)


def _child(part, *args):
    cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--part", part] + [str(a) for a in args]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        sys.exit("%s %s failed (%d): %s" % (part, args, p.returncode, p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--out", default="")
    ap.add_argument("--cost", action="store_true")
    ap.add_argument("--library", default="", help="--cost: another build of the C-ABI (default: this tree's librtiow_hip.so)")
    ap.add_argument("--part", default="")
    ap.add_argument("args", nargs="*")
    a = ap.parse_args()
    if a.part == "quality":
        print(json.dumps(quality(int(a.args[0]), float(a.args[1]))))
        return
    if a.part == "cost":
        print(json.dumps(cost(a.args[0], int(a.args[1]), int(a.args[2]), int(a.args[3]))))
        return
    if a.cost:
        import raytracingincuda_amd as rt
        library = os.path.abspath(a.library) if a.library else rt.api.lib_paths()["hip"]
        out = {"library": os.path.relpath(library, ROOT), "runs": a.runs, "frame": "320 x 180, a base of 4 samples, the walk's first step under the identity map"}
        for scene_id, prec in CONFIGS:
            out["scene%d_f%d" % (scene_id, prec)] = _child("cost", library, scene_id, prec, a.runs)
        print(json.dumps(out))
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
        return
    out = {"step": STEP, "frames": FRAMES, "spp": SPP, "ref_samples": REF_SAMPLES, "quality": {}}
    for scene_id in (1, 3):
        for name, deg in (("still", 0.0), ("orbit", 0.5)):
            out["quality"]["scene%d_%s" % (scene_id, name)] = _child("quality", scene_id, deg)
            print("quality scene%d_%s done" % (scene_id, name), flush=True)
    frame = [q["frame"]["ratio"] for q in out["quality"].values()]
    rays = [q["rays_ratio"] for q in out["quality"].values()]
    out["verdict"] = {"rule": "whole-frame ratio below 1 on both scenes and both camera modes at no more than %.2f x the restart walk's rays" % RAY_BOUND,
                      "frame_ratio": frame, "rays_ratio": rays, "pays": bool(max(frame) < 1 and max(rays) <= RAY_BOUND)}
    path = a.out or os.path.join(ROOT, "profiles", "scene_mapped", "scene_mapped_probe.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out["verdict"]))


if __name__ == "__main__":
    main()
