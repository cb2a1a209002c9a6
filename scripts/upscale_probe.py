"""Guided upscaling on one GPU:

  (a) cost: kernel_ms of rtiow_upscale from 1920 x 1080 to 3840 x 2160 (F = 2) with guides and layers current, scenes 1 and 3, fp32 and
      fp64, each source, the share on and off; HIP-event kernel times, medians of --runs after one warm-up.  Next to it
      rtiow_render_guides at a 3840 x 2160 camera, which traces the same number of first-hit rays: of this build and, with --parent-lib,
      of the parent commit's build (a kernel this feature leaves as it was: profiles/upscale/isa_diff_existing_kernels.txt), the two
      builds alternating --rounds times in fresh processes; the ratio upscale / guides is reported;
  (b) payoff at 640 x 360 output pixels, 50 bounces, fp32, scenes 1 and 3, against a 1024-sample accumulation at a 640 x 360 camera
      (its pixel grid is the upscaled grid up to rounding), from traced frames of 320 x 180 (F = 2) and 160 x 90 (F = 4), n = 1 and 4
      primary rays per OUTPUT pixel:
        a  the 640 x 360 frame at n samples, denoise()
        b  the traced frame at F F n samples, denoise(), upscale(): the same number of rays as a
        c  the traced frame at n samples, denoise(), upscale(): 1 / (F F) of the rays; reported, not part of the rule
        d  b's denoised image interpolated bilinearly in numpy
      linear MSE of each, and the summed kernel_ms of each arm;
  (c) --sweep: b / a at F = 2 over a grid of sigmas and the share; the defaults of raytracingincuda_amd/api.py are the setting with
      the smallest worst case over both scenes and both n, first of equals in grid order.

The rule (fixed before anything was measured): the feature PAYS if b / a < 1 at F = 2 on both scenes at both n, and b < d at every point
of F = 2 and F = 4.  Each part runs in a child process under its own `timeout`; the script stops at the first one that fails.  Writes one
JSON record (--out, default profiles/upscale/upscale_probe.json).

    python scripts/upscale_probe.py [--runs 7] [--rounds 3] [--sweep] [--parent-lib PATH] [--out profiles/upscale/upscale_probe.json]
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
SAMPLES = (1, 4)
FACTORS = (2, 4)
SWEEP = {"sigma_normal": (0.1, 0.3), "sigma_albedo": (0.1, INF), "sigma_depth": (0.1, 0.5, INF), "use_coverage": (0, 1)}
SOURCES = ("denoised", "linear", "history")


def _median(f, runs):
    f()                                                     # warm-up
    return statistics.median(f() for _ in range(runs))


def _defaults(api):
    return {"sigma_normal": api.UPSCALE_SIGMA_NORMAL, "sigma_albedo": api.UPSCALE_SIGMA_ALBEDO, "sigma_depth": api.UPSCALE_SIGMA_DEPTH,
            "use_coverage": api.UPSCALE_COVERAGE}


def cost(scene_id, prec, runs):
    import raytracingincuda_amd as rt
    from tests.preview_drive import begin
    a = rt.api
    W, H, B, F = 1920, 1080, 50, 2
    res = {}
    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, scene_id, rt.camera(prec, W, H, 1, B))
        r.accumulate(4)
        r.history_update()
        r.denoise()
        r.render_coverage(a.COVERAGE_GRID)
        res["render_guides_1920x1080_ms"] = round(_median(lambda: r.render_guides(), runs), 4)
        res["render_coverage_%dx%d_ms" % (a.COVERAGE_GRID, a.COVERAGE_GRID)] = round(_median(lambda: r.render_coverage(a.COVERAGE_GRID), runs), 4)

        def up(source, flag):                                # guides and layers are current: the upscale alone
            ms, n = ctypes.c_float(0), ctypes.c_uint64(0)
            r._check(r._lib.rtiow_upscale(r._h, F, source, a.UPSCALE_SIGMA_NORMAL, a.UPSCALE_SIGMA_ALBEDO, a.UPSCALE_SIGMA_DEPTH, flag, ctypes.byref(ms),
                                          ctypes.byref(n)))
            res["covered_pixels"] = max(int(n.value), res.get("covered_pixels", 0))
            return ms.value
        for source, name in enumerate(SOURCES):
            for flag in (0, 1):
                res["upscale_%s_%s_ms" % (name, "share" if flag else "plain")] = round(_median(lambda: up(source, flag), runs), 4)
    return res


def guides_4k(scene_id, prec, runs, library):
    """rtiow_render_guides at 3840 x 2160 through the C-ABI of `library` (this build's, or the parent commit's, which lacks the new calls)."""
    import raytracingincuda_amd as rt
    a = rt.api
    lib = ctypes.CDLL(library)
    for name in ("rtiow_create", "rtiow_destroy", "rtiow_set_camera", "rtiow_set_scene", "rtiow_render_guides", "rtiow_build_id"):
        getattr(lib, name).argtypes = a.HIP_ABI[name]
    lib.rtiow_build_id.restype = ctypes.c_char_p
    h = ctypes.c_void_p()
    dtype = "float32" if prec == 32 else "float64"
    cam = rt.camera(prec, 3840, 2160, 1, 50)
    ms = ctypes.c_float(0)

    def call(rc):
        if rc != 0:
            raise RuntimeError("rc %d from %s" % (rc, library))
    call(lib.rtiow_create(0, prec, ctypes.byref(h)))
    try:
        call(lib.rtiow_set_camera(h, ctypes.byref(cam)))
        call(a._set_scene(lib.rtiow_set_scene, h, rt.build_scene(scene_id, prec), dtype))

        def guides():
            call(lib.rtiow_render_guides(h, ctypes.byref(ms)))
            return ms.value
        return {"render_guides_3840x2160_ms": round(_median(guides, runs), 4), "build_id": lib.rtiow_build_id().decode()}
    finally:
        lib.rtiow_destroy(h)


def _bilinear(img, F):
    """img [H, W, 3] at the pixel centres of a grid F times as fine, taps clamped to the frame: plain numpy, in double."""
    import numpy as np
    H, W = img.shape[:2]

    def axis(n):
        f = (np.arange(F * n) + 0.5) / F - 0.5
        i0 = np.floor(f).astype(int)
        return np.clip(i0, 0, n - 1), np.clip(i0 + 1, 0, n - 1), f - i0
    x0, x1, gx = axis(W)
    y0, y1, gy = axis(H)
    gx, gy = gx[None, :, None], gy[:, None, None]
    top = img[y0][:, x0] * (1 - gx) + img[y0][:, x1] * gx
    bottom = img[y1][:, x0] * (1 - gx) + img[y1][:, x1] * gx
    return top * (1 - gy) + bottom * gy


def payoff(sweep):
    import numpy as np
    import raytracingincuda_amd as rt
    from tests.preview_drive import begin
    a = rt.api
    OW, OH, B, prec = 640, 360, 50, 32
    default = _defaults(a)
    combos = [dict(zip(SWEEP, v)) for v in itertools.product(*SWEEP.values())] if sweep else []
    out = {"defaults": {name: (str(x) if x == INF else x) for name, x in default.items()}}

    def denoise(r):
        ms = ctypes.c_float(0)
        r._check(r._lib.rtiow_denoise(r._h, a.DENOISE_LEVELS, a.DENOISE_SIGMA_COLOR, a.DENOISE_SIGMA_NORMAL, a.DENOISE_SIGMA_ALBEDO, a.DENOISE_SIGMA_DEPTH,
                                      ctypes.byref(ms)))
        return ms.value

    def upscale(r, F, c):
        ms = ctypes.c_float(0)
        r._check(r._lib.rtiow_upscale(r._h, F, a.UPSCALE_DENOISED, c["sigma_normal"], c["sigma_albedo"], c["sigma_depth"], c["use_coverage"],
                                      ctypes.byref(ms), None))
        return r.read_upscaled().astype(np.float64) ** 2, ms.value

    for scene_id in (1, 3):
        rec = {}
        with rt.Renderer(0, prec) as r:
            begin(r, rt, prec, scene_id, rt.camera(prec, OW, OH, 1, B))
            r.accumulate(1024)
            ref = r.read_linear().astype(np.float64)
            mse = lambda img: float(np.mean((img - ref) ** 2))
            full = {}
            for n in SAMPLES:
                r.reset_accumulation()
                ms = r.accumulate(n)
                ms += denoise(r)
                full[n] = (mse(r.read_denoised().astype(np.float64) ** 2), ms)
        for F in FACTORS:
            with rt.Renderer(0, prec) as r:
                begin(r, rt, prec, scene_id, rt.camera(prec, OW // F, OH // F, 1, B))
                r.render_coverage(a.COVERAGE_GRID)
                for n in SAMPLES:
                    s = {"mse_a": full[n][0], "ms_a": round(full[n][1], 4)}
                    for arm, samples in (("b", F * F * n), ("c", n)):
                        r.reset_accumulation()
                        ms = r.accumulate(samples)
                        ms += denoise(r)
                        small = r.read_denoised().astype(np.float64) ** 2
                        img, ms_up = upscale(r, F, default)
                        s["mse_" + arm] = mse(img)
                        s["ms_" + arm] = round(ms + ms_up, 4)
                        s["ms_upscale_" + arm] = round(ms_up, 4)
                        if arm == "b":
                            s["mse_d"] = mse(_bilinear(small, F))
                            if sweep and F == 2:
                                s["sweep"] = [round(mse(upscale(r, F, c)[0]) / full[n][0], 4) for c in combos]
                    s["b_over_a"] = round(s["mse_b"] / s["mse_a"], 4)
                    s["b_over_d"] = round(s["mse_b"] / s["mse_d"], 4)
                    s["c_over_a"] = round(s["mse_c"] / s["mse_a"], 4)
                    s["ray_share_c"] = 1.0 / (F * F)
                    rec["F%d_n%d" % (F, n)] = s
        out["scene%d" % scene_id] = rec
    if sweep:                                               # the smallest worst case over scenes and n at F = 2, first of equals
        worst = [max(out["scene%d" % sc]["F2_n%d" % n]["sweep"][k] for sc in (1, 3) for n in SAMPLES) for k in range(len(combos))]
        k = min(range(len(combos)), key=worst.__getitem__)
        out["sweep_grid"] = {name: [str(x) if x == INF else x for x in v] for name, v in SWEEP.items()}
        out["sweep_worst_b_over_a"] = worst
        out["sweep_best"] = dict({name: (str(x) if x == INF else x) for name, x in combos[k].items()}, worst_b_over_a=worst[k])
        kd = [i for i, c in enumerate(combos) if c == default]
        if kd:
            out["sweep_default_worst_b_over_a"] = worst[kd[0]]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upscale", "upscale_probe.json"))
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        kind, *rest = a.child.split(",")
        if kind == "cost":
            res = cost(int(rest[0]), int(rest[1]), a.runs)
        elif kind == "guides":
            res = guides_4k(int(rest[0]), int(rest[1]), a.runs, rest[2])
        else:
            res = payoff(a.sweep)
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    import raytracingincuda_amd as rt
    record = {"build_id": rt.build_id(), "runs": a.runs, "rounds": a.rounds, "upscale_1920x1080_to_3840x2160": {}, "render_guides_3840x2160": {}}

    def child(spec):
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--child", spec, "--runs", str(a.runs)]
        if a.sweep:
            cmd.append("--sweep")
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print("child %s failed (exit %d):\n%s\n%s" % (spec, p.returncode, p.stdout[-2000:], p.stderr[-4000:]), file=sys.stderr)
            return None
        return json.loads(line[0][7:])

    builds = [("this", rt.lib_paths()["hip"])] + ([("parent", os.path.abspath(a.parent_lib))] if a.parent_lib else [])
    for scene_id, prec in CONFIGS:
        name = "scene%d_f%d" % (scene_id, prec)
        res = child("cost,%d,%d" % (scene_id, prec))
        if res is None:
            return 1
        times = {which: [] for which, _ in builds}
        for _ in range(a.rounds):                           # the two builds alternate, each in a fresh process
            for which, path in builds:
                g = child("guides,%d,%d,%s" % (scene_id, prec, path))
                if g is None:
                    return 1
                times[which].append(g["render_guides_3840x2160_ms"])
                record.setdefault("build_ids", {})[which] = g["build_id"]
        guides = {which: round(statistics.median(v), 4) for which, v in times.items()}
        record["render_guides_3840x2160"][name] = dict(guides, rounds={which: v for which, v in times.items()})
        against = guides.get("parent", guides["this"])
        res["ratio_to_render_guides_3840x2160"] = {k[8:-3]: round(v / against, 3) for k, v in res.items() if k.startswith("upscale_")}
        record["upscale_1920x1080_to_3840x2160"][name] = res
        print(name, json.dumps(res), json.dumps(guides), flush=True)
    res = child("payoff")
    if res is None:
        return 1
    record["payoff_640x360_b50_f32"] = res
    points = [res["scene%d" % sc]["F%d_n%d" % (F, n)] for sc in (1, 3) for F in FACTORS for n in SAMPLES]
    half = [res["scene%d" % sc]["F2_n%d" % n] for sc in (1, 3) for n in SAMPLES]
    record["pays"] = all(p["b_over_a"] < 1 for p in half) and all(p["mse_b"] < p["mse_d"] for p in points)
    record["rule"] = "b / a < 1 at F = 2 on scenes 1 and 3 at n = 1 and 4, and b < d at every point of F = 2 and F = 4"
    print("payoff", json.dumps({k: v for k, v in res.items() if k.startswith("sweep_best") or k == "defaults"}), flush=True)
    for sc in (1, 3):
        for key, p in res["scene%d" % sc].items():
            print("scene%d %s" % (sc, key), json.dumps({k: v for k, v in p.items() if k != "sweep"}), flush=True)
    print("pays:", record["pays"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
