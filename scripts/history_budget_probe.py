"""History-guided sample budgets on one GPU:

  (a) cost at 1920 x 1080, scene 3, fp32 and fp64: a base committed at the reference's view, the camera turned 0.5 degrees, 4 samples in
      the adaptive mode, guides current.  rtiow_history_plan next to rtiow_history_update, and a chunk of rtiow_accumulate_budget next to
      one of rtiow_accumulate_adaptive at equal active count -- none, so that the chunk is its select and its finish and only the select
      differs -- the calls alternating in one process; HIP-event kernel times, medians of --runs (at least 20) after one warm-up each.
      The plan gathers the update's taps and moves less, so its median must not exceed the update's (exit status 1 otherwise);
  (b) quality at 320 x 180, 50 bounces, fp32, scenes 1 and 3, over the walk of tests/preview_drive.py (8 cameras, 0.5 degrees apart,
      independent noise, update and commit every frame), against 1024 samples at the last camera: the walk with 4 uniform samples a
      frame next to the walk with plan and budget chunks to convergence every frame, at the defaults of raytracingincuda_amd/api.py
      (tests/preview_drive.py's walk, uniform_sampler, budget_sampler, compare; test_it_pays asserts on these): primary rays of the
      whole walk, linear MSE of the temporal image at the last frame over the whole frame and over the pixels with m = 0 in the last
      frame's plan;
  (c) --sweep: the same over target x min_samples x chunk x max_history.  A setting is eligible if its walk traces no more primary rays
      than the uniform walk in both scenes; the defaults are the eligible setting with the smallest worse-of-two-scenes ratio of
      whole-frame MSE to the uniform walk's, the first such setting in grid order.

Each part runs in a child process under its own `timeout`; the script stops at the first one that fails.  Writes one JSON record
(--out, default profiles/history_budget/history_budget_probe.json).

    python scripts/history_budget_probe.py [--runs 25] [--sweep] [--out FILE]
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

CHILD_TIMEOUT_S = {"cost": 240, "quality": 600}
SWEEP_TARGET = (8.0, 16.0, 32.0)
SWEEP_MIN_SAMPLES = (0, 1, 2)
SWEEP_CHUNK = (1, 2, 4)
SWEEP_MAX_HISTORY = (16.0, 64.0)
BIG = 2 ** 31 - 1


def cost(prec, runs):
    import raytracingincuda_amd as rt
    from tests.preview_drive import orbit
    a = rt.api
    W, H = 1920, 1080
    params = (a.HISTORY_DEPTH_TOL, a.HISTORY_NORMAL_COS, a.HISTORY_MAX)
    with rt.Renderer(0, prec) as r:
        r.set_camera(rt.camera_look(prec, W, H, 1, 50)); r.set_scene(rt.build_scene(3, prec)); r.init_rng(1227)
        r.accumulate_adaptive(4, 0.0, min_samples=4)
        r.history_update(); r.history_commit()
        r.set_camera(rt.camera_look(prec, W, H, 1, 50, lookfrom=orbit(0.5))); r.init_rng(1228)
        r.accumulate_adaptive(4, 0.0, min_samples=4)
        r.render_guides()

        def timed(fn, *args):
            ms, n = ctypes.c_float(0), ctypes.c_uint64(0)
            r._check(fn(r._h, *args, ctypes.byref(ms), ctypes.byref(n)))
            return ms.value, n.value

        def chunk(fn, rule):
            ms, active = ctypes.c_float(0), ctypes.c_int(-1)
            r._check(fn(r._h, 1, 0, rule, BIG, ctypes.byref(ms), ctypes.byref(active)))
            assert active.value == 0, active.value
            return ms.value

        plan = lambda: timed(r._lib.rtiow_history_plan, *params)
        update = lambda: timed(r._lib.rtiow_history_update, *params)
        budget = lambda: chunk(r._lib.rtiow_accumulate_budget, 1e-30)                  # nobody is below the target
        adaptive = lambda: chunk(r._lib.rtiow_accumulate_adaptive, float("inf"))       # nobody is above the error
        _, planned = plan(); _, carried = update(); budget(); adaptive()               # warm-up
        assert planned == carried, (planned, carried)
        tp, tu, tb, ta = [], [], [], []
        for _ in range(runs):
            tp.append(plan()[0]); tu.append(update()[0]); tb.append(budget()); ta.append(adaptive())
    p, u, b, d = (statistics.median(t) for t in (tp, tu, tb, ta))
    return {"history_plan_ms": round(p, 4), "history_update_ms": round(u, 4), "plan_over_update": round(p / u, 4),
            "budget_chunk_no_active_ms": round(b, 4), "adaptive_chunk_no_active_ms": round(d, 4), "budget_over_adaptive": round(b / d, 4),
            "runs": runs, "reprojected_pixels": int(planned), "pixels": W * H}


def quality(sweep):
    import raytracingincuda_amd as rt
    from tests.preview_drive import budget_sampler, compare, orbit_reference, uniform_sampler, walk
    a = rt.api
    default = (a.BUDGET_TARGET, a.BUDGET_MIN_SAMPLES, a.BUDGET_CHUNK, a.HISTORY_MAX)
    grid = list(itertools.product(SWEEP_TARGET, SWEEP_MIN_SAMPLES, SWEEP_CHUNK, SWEEP_MAX_HISTORY)) if sweep else []
    name = lambda p: "target=%g,min_samples=%d,chunk=%d,max_history=%g" % p
    rounded = lambda q: {k: (round(v, 4) if k in ("rays", "frame", "disoccluded") else v) for k, v in q.items()}
    out = {"defaults": name(default), "orbit": {}}
    table = {name(p): {} for p in grid}

    def run(scene_id, uniform, ref, p):
        target, min_samples, chunk, max_history = p
        params = (a.HISTORY_DEPTH_TOL, a.HISTORY_NORMAL_COS, max_history)
        return compare(uniform, walk(rt, scene_id, budget_sampler(chunk, target, min_samples), params=params), ref)

    for scene_id in (1, 3):
        ref = orbit_reference(rt, scene_id)
        uniform = walk(rt, scene_id, uniform_sampler())
        out["orbit"]["scene%d" % scene_id] = rounded(run(scene_id, uniform, ref, default))
        for k, p in enumerate(grid):
            if k % 6 == 0:
                print("scene %d: setting %d of %d" % (scene_id, k, len(grid)), file=sys.stderr, flush=True)
            q = run(scene_id, uniform, ref, p)
            table[name(p)]["scene%d" % scene_id] = {k: round(q[k], 4) for k in ("rays", "frame", "disoccluded")}
    if sweep:
        worst = lambda p, k: max(table[name(p)]["scene%d" % s][k] for s in (1, 3))
        eligible = [p for p in grid if worst(p, "rays") <= 1]
        out["sweep"] = table
        out["sweep_eligible"] = [name(p) for p in eligible]
        out["sweep_worst_frame"] = {name(p): worst(p, "frame") for p in eligible}
        out["sweep_best"] = name(min(eligible, key=lambda p: worst(p, "frame"))) if eligible else None     # the first of equals, in grid order
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "history_budget", "history_budget_probe.json"))
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
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S[child.split(",")[0]]), sys.executable, os.path.abspath(__file__), "--child", child,
               "--runs", str(a.runs)]
        if a.sweep:
            cmd.append("--sweep")
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)          # the child's progress lines (stderr) pass through
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print("child %s failed (exit %d):\n%s" % (child, p.returncode, p.stdout[-4000:]), file=sys.stderr)
            return 1
        res = json.loads(line[0][7:])
        (record[group] if group else record)[name] = res
        print(child, json.dumps(res)[:1500], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    slow = [k for k, v in record["frame_cost_1920x1080"].items() if v["history_plan_ms"] > v["history_update_ms"]]
    if slow:
        print("history_plan is slower than history_update:", slow, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
