"""Adaptive progressive rendering (rtiow_accumulate_adaptive) on one GPU, 1920 x 1080 at 50 bounces, scenes 3 and 1, fp32 and fp64:

  (a) one all-active adaptive chunk of 100 samples (min_samples = max_samples = INT32_MAX) against one rtiow_accumulate chunk of 100;
  (b) the select and finish kernels alone: a chunk in which no pixel is active (after one chunk of 8 samples, rel_error = 1e30);
  (c) primary rays and kernel time to reach a frame-median error: the target is the median err of the uniform image at 64 samples
      (chunks of 8 for every pixel); the adaptive run uses chunks of 8, min_samples = 8, rel_error = the target, and stops when the
      median err reaches the target (or no pixel is active).

(a) and (b) are medians of --runs after one warm-up.  Each configuration runs in a child process under its own `timeout`; the script
stops at the first one that fails.  Writes one JSON record (--out, default profiles/adaptive/adaptive_probe.json).

    python scripts/adaptive_probe.py [--runs 5] [--out profiles/adaptive/adaptive_probe.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, B = 1920, 1080, 50
BIG = 2 ** 31 - 1
CONFIGS = [(3, 32), (3, 64), (1, 32), (1, 64)]
CHILD_TIMEOUT_S = 240


def _median(f, runs):
    f()                                                     # warm-up
    return statistics.median(f() for _ in range(runs))


def child(scene_id, prec, runs):
    import numpy as np
    import raytracingincuda_amd as rt
    res = {}
    with rt.Renderer(0, prec) as r:
        r.set_camera(rt.camera(prec, W, H, 1, B))
        r.set_scene(rt.build_scene(scene_id, prec))
        r.init_rng(1227)

        def plain():
            r.reset_accumulation()
            return r.accumulate(100)
        res["accumulate_100_ms"] = round(_median(plain, runs), 3)
        want = r.read_framebuffer()

        def all_active():
            r.reset_accumulation()
            ms, active = r.accumulate_adaptive(100, 0.0, min_samples=BIG, max_samples=BIG)
            assert active == W * H
            return ms
        res["adaptive_all_active_100_ms"] = round(_median(all_active, runs), 3)
        res["adaptive_all_active_bit_exact"] = bool(np.array_equal(r.read_framebuffer().view(np.uint8), want.view(np.uint8)))
        res["adaptive_all_active_vs_accumulate"] = round(res["adaptive_all_active_100_ms"] / res["accumulate_100_ms"] - 1.0, 4)
        res["adaptive_stats"] = {k: v for k, v in r.stats().items() if k in ("vgprs", "grid_blocks", "scene_source", "main_clock_mhz")}

        r.reset_accumulation()
        r.accumulate_adaptive(8, 0.0, min_samples=BIG, max_samples=BIG)

        def select_finish():
            ms, active = r.accumulate_adaptive(8, 1e30)
            assert active == 0
            return ms
        res["select_finish_ms"] = round(_median(select_finish, runs), 4)

        # (c) uniform to 64 samples, then adaptive to the same frame-median error
        r.reset_accumulation()
        uni_ms = 0.0
        for _ in range(8):
            ms, _ = r.accumulate_adaptive(8, 0.0, min_samples=BIG, max_samples=BIG)
            uni_ms += ms
        _, err = r.adaptive_state()
        target = float(np.median(err))
        res["uniform"] = {"samples": 64, "median_err": target, "primary_rays": 64 * W * H, "kernel_ms": round(uni_ms, 3),
                          "p90_err": float(np.quantile(err, 0.9))}
        r.reset_accumulation()
        ad_ms, rays, calls = 0.0, 0, 0
        while True:
            ms, active = r.accumulate_adaptive(8, target, min_samples=8, max_samples=1024)
            ad_ms += ms
            rays += active * 8
            calls += 1
            counts, err = r.adaptive_state()
            if float(np.median(err)) <= target or active == 0:
                break
        res["adaptive"] = {"median_err": float(np.median(err)), "primary_rays": rays, "kernel_ms": round(ad_ms, 3), "calls": calls,
                           "mean_samples": round(float(counts.mean()), 2), "max_samples": int(counts.max()),
                           "p90_err": float(np.quantile(err, 0.9))}
        res["rays_saved"] = round(1.0 - rays / (64 * W * H), 4)
        res["time_saved"] = round(1.0 - ad_ms / uni_ms, 4)
    print(json.dumps(res, sort_keys=True), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive", "adaptive_probe.json"))
    ap.add_argument("--child", nargs=2, type=int, default=None)
    a = ap.parse_args()
    if a.child:
        child(a.child[0], a.child[1], a.runs)
        return 0
    import raytracingincuda_amd as rt
    rec = {"probe": "adaptive", "build_id": rt.build_id(), "frame": "%dx%d_%db" % (W, H, B), "runs": a.runs,
           "statistic": "(a), (b): median after one warm-up; (c): one run, sums of kernel_ms", "results": {}}
    for scene_id, prec in CONFIGS:
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--child", str(scene_id), str(prec),
               "--runs", str(a.runs)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            print("adaptive_probe: scene %d f%d failed with status %d; stopping" % (scene_id, prec, p.returncode), file=sys.stderr)
            return 1
        rec["results"]["scene%d_f%d" % (scene_id, prec)] = json.loads(p.stdout.strip().splitlines()[-1])
    line = json.dumps(rec, sort_keys=True)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
