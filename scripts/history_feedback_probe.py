"""Recurrent history on one GPU, in the protocol of scripts/history_clip_probe.py and
scripts/history_variance_probe.py:

  (a) quality at 320 x 180, 50 bounces, fp32, scenes 1 and 3, over the walk of DESIGN.md section 4.10 (8 cameras, 4 samples each with
      independent noise, seeds 1227 + frame, an update and a commit every frame) at 0.5 and at 2 degrees a frame, against 1024 samples
      at the last camera.  Routes: {plain update, clipped update at its defaults} x {history_commit, history_commit_filtered}.
      R_T = MSE(temporal image, filtered commits) / MSE(temporal image, plain commits) on the last frame, R_D the same ratio for
      denoise_history() at its defaults (squared back to linear), each over the whole frame, over the mirror and glass pixels
      (scripts/specular_guides_probe.py's mask) and over the pixels that carried no history into the last frame (length == the
      frame's own samples).  sigma_color x feedback swept, the guide sigmas at the DENOISE_* defaults;
  (b) the defaults: the grid point with the smallest worse-of-two-scenes R_T over the whole frame on the clipped walk at 0.5 degrees a
      frame, the first such point in grid order; "defaults" repeats the sweep's entry at the values raytracingincuda_amd/api.py has now
      (--parts none fills it in again, and the verdict, without a GPU);
  (c) blur: a 32-frame walk at the defaults (clipped update, 0.5 degrees a frame), plain and filtered commits side by side, against
      1024 samples at every camera: R_T per frame, and the first frame at which it exceeds 1;
  (d) cost at 1920 x 1080, scene 3, fp32 and fp64, on scripts/history_clip_probe.py's frame (a base committed at the reference's view,
      the camera turned 0.5 degrees, 4 samples, a clipped update at its defaults, guides current): feedback_filter_kernel and one level
      of denoise_level_kernel (denoise_history(levels=1)) under `rocprofv3 --kernel-trace` in a run of its own (--rocprof-dir says
      where it writes), each dispatch's end - start from the trace, REPS repetitions after one warm-up;
  (e) the yardstick: the same denoise_level_kernel dispatch from the PARENT commit's tree (--parent-tree: a `git archive` of the parent,
      built in place), the same frame, five repetitions.  The new kernel is to be no slower than their median plus their spread
      (max - min); "verdict" says whether it is.

Each part runs in a child process under its own `timeout`; the script stops at the first one that fails.  Writes one JSON record
(--out, default profiles/history_feedback/history_feedback_probe.json); parts measured in an earlier call on the same build stay.

    python scripts/history_feedback_probe.py [--out FILE] [--rocprof-dir DIR] [--parent-tree DIR] [--parts quality,blur,trace,parent | none]
"""
import argparse
import csv
import glob
import itertools
import json
import os
import statistics
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("RTIOW_PROBE_TREE") or HERE           # the children of part (e) import the parent commit's package and tests
sys.path.insert(0, ROOT)

CHILD_TIMEOUT_S = 420
SWEEP_SIGMA = (0.05, 0.1, 0.2, 0.4, float("inf"))
SWEEP_FEEDBACK = (0.25, 0.5, 1.0)
SPEEDS = (0.5, 2.0)
UPDATES = ("plain_update", "clipped_update")
REPS = 5
REGIONS = ("frame", "specular_pixels", "no_history_pixels")


def name(sigma, feedback):
    return "sigma_color=%g,feedback=%g" % (sigma, feedback)


def clip_of(rt, update):
    return None if update == "plain_update" else (rt.api.HISTORY_CLIP_RADIUS, rt.api.HISTORY_CLIP_GAMMA)


def reference_and_mask(rt, scene_id, step_deg, frame, W=320, H=180, B=50, prec=32, samples=1024):
    """The linear image of `samples` samples at camera `frame` of the walk, and the pixels whose centre ray meets a mirror or glass."""
    import numpy as np
    from tests.preview_drive import begin, orbit
    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, scene_id, rt.camera_look(prec, W, H, 1, B, lookfrom=orbit(step_deg * frame)))
        r.accumulate(samples)
        ref = r.read_linear().astype(np.float64)
        r.set_guide_mode(rt.GUIDES_SPECULAR, 8, float("inf"))
        mask = r.filter_guides()[3] >= 1
    return ref, mask


def quality(step_deg):
    import numpy as np
    import raytracingincuda_amd as rt
    from tests.preview_drive import feedback_walk
    from tests.preview_model import mse
    frames, spp = 8, 4
    grid = list(itertools.product(SWEEP_SIGMA, SWEEP_FEEDBACK))
    out = {u: {"sweep": {name(*p): {} for p in grid}, "plain_commit_mse": {}} for u in UPDATES}
    for scene_id in (1, 3):
        scene = "scene%d" % scene_id
        ref, spec = reference_and_mask(rt, scene_id, step_deg, frames - 1)
        for u in UPDATES:
            clip = clip_of(rt, u)
            plain = feedback_walk(rt, scene_id, step_deg, clip, None)
            fresh = plain["length"] <= spp                       # nothing carried into the last frame
            sel = {"frame": None, "specular_pixels": spec, "no_history_pixels": fresh}
            both = lambda w: {k: {reg: mse(w[k], ref, sel[reg]) for reg in REGIONS} for k in ("temporal", "denoise_history")}
            base = both(plain)
            out[u]["plain_commit_mse"][scene] = dict(base, specular_pixels_count=int(spec.sum()), no_history_pixels_count=int(fresh.sum()),
                                                     pixels=int(spec.size))

            def ratios(commit):
                w = feedback_walk(rt, scene_id, step_deg, clip, commit)
                if not np.array_equal(w["length"], plain["length"]):
                    raise RuntimeError("the filtered commit changed the history lengths")
                got = both(w)
                res = {}
                for reg, tag in zip(REGIONS, ("", "_specular", "_no_history")):
                    res["R_T" + tag] = round(got["temporal"][reg] / base["temporal"][reg], 4)
                    res["R_D" + tag] = round(got["denoise_history"][reg] / base["denoise_history"][reg], 4)
                return res

            for p in grid:
                out[u]["sweep"][name(*p)][scene] = ratios({"sigma_color": p[0], "feedback": p[1]})
            print(step_deg, scene, u, "done", file=sys.stderr, flush=True)
    for u in UPDATES:
        worst = {name(*p): max(out[u]["sweep"][name(*p)]["scene%d" % s]["R_T"] for s in (1, 3)) for p in grid}
        out[u]["sweep_worst_R_T"] = worst
        out[u]["sweep_best"] = min((name(*p) for p in grid), key=worst.__getitem__)                 # the first of equals, in grid order
    return out


def blur(frames):
    """Part (c): two handles walk side by side, one committing plainly, one through the filter at the defaults."""
    import numpy as np
    import raytracingincuda_amd as rt
    from tests.preview_drive import begin, move, orbit
    from tests.preview_model import mse
    a = rt.api
    step_deg, spp, W, H, B, prec = 0.5, 4, 320, 180, 50, 32
    clip = clip_of(rt, "clipped_update")
    out = {"frames": frames, "degrees_a_frame": step_deg, "setting": name(a.HISTORY_FEEDBACK_SIGMA_COLOR, a.HISTORY_FEEDBACK)}
    for scene_id in (1, 3):
        cams = [rt.camera_look(prec, W, H, 1, B, lookfrom=orbit(step_deg * k)) for k in range(frames)]
        curve = []
        with rt.Renderer(0, prec) as plain, rt.Renderer(0, prec) as filt, rt.Renderer(0, prec) as truth:
            for r in (plain, filt, truth):
                begin(r, rt, prec, scene_id, cams[0])
            for k, cam in enumerate(cams):
                move(truth, cam, 99)
                truth.accumulate(1024)
                ref = truth.read_linear().astype(np.float64)
                err = []
                for r in (plain, filt):
                    move(r, cam, 1227 + k)
                    r.accumulate(spp)
                    r.history_update_clipped(*clip)
                    err.append(mse(r.history()[0].astype(np.float64), ref))
                plain.history_commit()
                filt.history_commit_filtered()
                curve.append(round(err[1] / err[0], 4))
        above = [k for k, v in enumerate(curve) if v > 1]
        out["scene%d" % scene_id] = {"R_T_per_frame": curve, "first_frame_above_1": above[0] if above else None,
                                     "R_T_last_frame": curve[-1], "R_T_smallest": min(curve), "R_T_largest_after_frame_0": max(curve[1:])}
        print("blur", scene_id, curve, file=sys.stderr, flush=True)
    return out


def probe_frame(rt, r, prec):
    """scripts/history_clip_probe.py's frame with a clipped update on top."""
    from tests.preview_drive import orbit
    W, H = 1920, 1080
    r.set_camera(rt.camera_look(prec, W, H, 1, 50)); r.set_scene(rt.build_scene(3, prec)); r.init_rng(1227)
    r.accumulate(4)
    r.history_update_clipped(); r.history_commit()
    r.set_camera(rt.camera_look(prec, W, H, 1, 50, lookfrom=orbit(0.5))); r.init_rng(1228)
    r.accumulate(4)
    r.render_guides()
    r.history_update_clipped()
    return W * H


def trace(prec, with_feedback):
    """The dispatches parts (d) and (e) read from the trace: REPS + 1 times one filter level of the temporal image, then -- this tree
    only -- REPS + 1 times a filtered commit and a clipped update to have a temporal image again."""
    import raytracingincuda_amd as rt
    with rt.Renderer(0, prec) as r:
        pixels = probe_frame(rt, r, prec)
        for _ in range(REPS + 1):                            # the same temporal image in both trees
            r.denoise_history(1)
        for _ in range(REPS + 1 if with_feedback else 0):
            r.history_commit_filtered()
            r.history_update_clipped()                       # a temporal image again, now over the frame's own base: the same work
    return {"pixels": pixels, "repetitions": REPS}


def read_trace(directory, with_feedback):
    """Per-dispatch end - start in ms from rocprofv3's kernel trace of trace() (the first round is warm-up)."""
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise RuntimeError("expected one kernel trace under %s, found %s" % (directory, files))
    with open(files[0], newline="") as f:
        rows = list(csv.DictReader(f))
    key = {k.lower(): k for k in rows[0]}
    kname, start, end = key["kernel_name"], key["start_timestamp"], key["end_timestamp"]
    rows.sort(key=lambda row: int(row[start]))
    ms = lambda sub: [round((int(row[end]) - int(row[start])) * 1e-6, 4) for row in rows if sub in row[kname]]
    out = {}
    for sub, label in (("denoise_level_kernel<", "denoise_level_kernel"),) + ((("feedback_filter_kernel<", "feedback_filter_kernel"),) if with_feedback else ()):
        t = ms(sub)
        if len(t) != REPS + 1:
            raise RuntimeError("unexpected dispatch count of %s in the trace: %d" % (sub, len(t)))
        t = t[1:]
        out[label + "_ms"] = round(statistics.median(t), 4)
        out[label + "_repetitions_ms"] = t
        out[label + "_spread_ms"] = round(max(t) - min(t), 4)
    return out


def verdict(record, api):
    """Fills in "defaults" -- the sweep's entry at the values raytracingincuda_amd/api.py has now, which the rule of (b) takes from the
    grid -- and returns the verdict over whatever parts the record holds."""
    v = {}
    q = record["quality_320x180_b50_f32"]
    setting = name(api.HISTORY_FEEDBACK_SIGMA_COLOR, api.HISTORY_FEEDBACK)
    for by in q.values():
        for u in UPDATES:
            by[u]["defaults"] = dict(by[u]["sweep"][setting], setting=setting)
    if len(q) == len(SPEEDS):
        ratios = {"%s,%s,%s" % (speed, u, scene): (d["R_T"], d["R_D"]) for speed, by in q.items() for u in UPDATES
                  for scene, d in by[u]["defaults"].items() if scene != "setting"}
        v["defaults"] = setting
        v["sweep_best_clipped_0.5_degrees"] = q["0.5_degrees_a_frame"]["clipped_update"]["sweep_best"]
        v["worst_R_T_at_defaults"] = max(r[0] for r in ratios.values())
        v["worst_R_D_at_defaults"] = max(r[1] for r in ratios.values())
        v["pays"] = all(r[0] < 1 and r[1] < 1 for r in ratios.values())
    cost, parent = record["kernel_cost_1920x1080"], record["parent_filter_level_1920x1080"]
    for key in cost:
        if key in parent:
            bound = parent[key]["denoise_level_kernel_ms"] + parent[key]["denoise_level_kernel_spread_ms"]
            v["cost_" + key] = {"feedback_filter_kernel_ms": cost[key]["feedback_filter_kernel_ms"], "bound_ms": round(bound, 4),
                                "within_bound": cost[key]["feedback_filter_kernel_ms"] <= bound}
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "history_feedback", "history_feedback_probe.json"))
    ap.add_argument("--rocprof-dir", default="")
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--blur-frames", type=int, default=32)
    ap.add_argument("--parts", default="quality,blur,trace,parent")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        kind, arg = a.child.split(",")
        res = {"quality": lambda: quality(float(arg)), "blur": lambda: blur(int(arg)), "trace": lambda: trace(int(arg), True),
               "parent": lambda: trace(int(arg), False)}[kind]()
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    import raytracingincuda_amd as rt
    parts = a.parts.split(",")
    if "parent" in parts and not os.path.isdir(a.parent_tree):
        ap.error("part `parent` needs --parent-tree: the parent commit exported with git archive and built in place")
    record = {"build_id": rt.build_id(), "quality_320x180_b50_f32": {}, "blur_320x180_b50_f32": {}, "kernel_cost_1920x1080": {},
              "parent_filter_level_1920x1080": {}}
    if os.path.exists(a.out):                            # parts measured in an earlier call stay
        with open(a.out) as f:
            old = json.load(f)
        if old.get("build_id") == record["build_id"]:
            record = old
    jobs = []
    if "quality" in parts:
        jobs += [("quality,%g" % d, "quality_320x180_b50_f32", "%g_degrees_a_frame" % d) for d in SPEEDS]
    if "blur" in parts:
        jobs += [("blur,%d" % a.blur_frames, "blur_320x180_b50_f32", "clipped_update")]
    if "trace" in parts:
        jobs += [("trace,%d" % p, "kernel_cost_1920x1080", "scene3_f%d" % p) for p in (32, 64)]
    if "parent" in parts:
        jobs += [("parent,%d" % p, "parent_filter_level_1920x1080", "scene3_f%d" % p) for p in (32, 64)]
    for child, group, key in jobs:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", child]
        env = dict(os.environ)
        traced = child.startswith(("trace", "parent"))
        if child.startswith("parent"):
            env["RTIOW_PROBE_TREE"] = os.path.abspath(a.parent_tree)
        with tempfile.TemporaryDirectory(dir=a.rocprof_dir or None) as tmp:
            if traced:                                       # the program itself goes after `--`
                cmd = ["rocprofv3", "--kernel-trace", "-d", tmp, "-o", "kt", "--output-format", "csv", "--"] + cmd
            p = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT_S)] + cmd, stdout=subprocess.PIPE, text=True, env=env)
            line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print("child %s failed (exit %d):\n%s" % (child, p.returncode, p.stdout[-2000:]), file=sys.stderr)
                return 1
            res = json.loads(line[0][7:])
            if traced:
                res.update(read_trace(tmp, child.startswith("trace")))
        record[group][key] = res
        record["verdict"] = verdict(record, rt.api)
        print(child, json.dumps({k: ({kk: vv for kk, vv in v.items() if kk not in ("sweep", "sweep_worst_R_T")} if isinstance(v, dict) else v)
                                 for k, v in res.items()})[:3000], flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    if not jobs:                                         # --parts none: "defaults" and the verdict again, e.g. after new defaults in api.py
        record["verdict"] = verdict(record, rt.api)
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    print("verdict", json.dumps(record.get("verdict", {})), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
