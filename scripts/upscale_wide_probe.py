"""Wide-support guided upscaling on one GPU, by the rule of DESIGN.md section 4.23:

  (a) cost: kernel_ms of rtiow_upscale_wide from 1920 x 1080 to 3840 x 2160 (F = 2) with guides and layers current, scenes 1 and 3, fp32
      and fp64, each source, the share on and off; HIP-event kernel times, medians of --runs after one warm-up.  Beside it rtiow_upscale
      at the same points on a build of the parent commit (--parent-root: a built checkout of it, whose own package drives its library),
      the two alternating --rounds times in fresh processes; the ratio wide / narrow is reported;
  (b) payoff at 640 x 360 output pixels, 50 bounces, fp32, scenes 1 and 3, against a 1024-sample accumulation at a 640 x 360 camera, from
      traced frames of 320 x 180 (F = 2) and 160 x 90 (F = 4), n = 1 and 4 primary rays per OUTPUT pixel -- scripts/upscale_probe.py's
      frames and arms:
        a  the 640 x 360 frame at n samples, denoise()
        b  the traced frame at F F n samples, denoise(), upscale() at its defaults
        d  b's denoised image interpolated bilinearly in numpy
        w  b's denoised image through upscale_wide()
        s  b's denoised image through upscale_wide() with every sigma = +inf and no share: the unguided B-spline
      linear MSE of each, and the kernel_ms of the two upscales;
  (c) the sweep: w / a over scripts/upscale_probe.py's 24 settings at every point.  The defaults of upscale_wide() are the setting with
      the smallest worst case of w / a at F = 2 over both scenes and both n, first of equals in grid order; w is reported at that setting.

The rule (fixed before anything was measured): the feature PAYS if, at those defaults, w < d and w < b at all eight points of F = 2 and
F = 4.  w / s is reported at every point -- what the guiding adds -- and is not part of the rule.  Each part runs in a child process under
its own `timeout`; the script stops at the first one that fails.  Writes one JSON record (--out).

    python scripts/upscale_wide_probe.py [--runs 7] [--rounds 3] [--parent-root PATH] [--out profiles/upscale_wide/upscale_wide_probe.json]
"""
import argparse
import ctypes
import itertools
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(3, 32), (3, 64), (1, 32), (1, 64)]
CHILD_TIMEOUT_S = 300
INF = float("inf")
SAMPLES = (1, 4)
FACTORS = (2, 4)
SWEEP = {"sigma_normal": (0.1, 0.3), "sigma_albedo": (0.1, INF), "sigma_depth": (0.1, 0.5, INF), "use_coverage": (0, 1)}      # upscale_probe.py's
SOURCES = ("denoised", "linear", "history")
UNGUIDED = {"sigma_normal": INF, "sigma_albedo": INF, "sigma_depth": INF, "use_coverage": 0}


def _median(f, runs):
    f()                                                     # warm-up
    return statistics.median(f() for _ in range(runs))


def _defaults(api, wide):
    p = "UPSCALE_WIDE_" if wide else "UPSCALE_"
    return {"sigma_normal": getattr(api, p + "SIGMA_NORMAL"), "sigma_albedo": getattr(api, p + "SIGMA_ALBEDO"), "sigma_depth": getattr(api, p + "SIGMA_DEPTH"),
            "use_coverage": getattr(api, p + "COVERAGE")}


def _text(setting):
    return {name: (str(x) if x == INF else x) for name, x in setting.items()}


def cost(scene_id, prec, runs, call):
    """kernel_ms of `call` (rtiow_upscale or rtiow_upscale_wide) of the package on sys.path, at its sigmas' defaults."""
    import raytracingincuda_amd as rt
    from tests.preview_drive import begin
    a = rt.api
    W, H, B, F = 1920, 1080, 50, 2
    d = _defaults(a, call.endswith("_wide"))
    res = {"build_id": rt.build_id(), "call": call}
    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, scene_id, rt.camera(prec, W, H, 1, B))
        r.accumulate(4)
        r.history_update()
        r.denoise()
        r.render_coverage(a.COVERAGE_GRID)
        fn = getattr(r._lib, call)

        def up(source, flag):                                # guides and layers are current: the upscale alone
            ms, n = ctypes.c_float(0), ctypes.c_uint64(0)
            r._check(fn(r._h, F, source, d["sigma_normal"], d["sigma_albedo"], d["sigma_depth"], flag, ctypes.byref(ms), ctypes.byref(n)))
            return ms.value
        for source, name in enumerate(SOURCES):
            for flag in (0, 1):
                res["%s_%s_ms" % (name, "share" if flag else "plain")] = round(_median(lambda: up(source, flag), runs), 4)
    return res


def payoff():
    import numpy as np
    import raytracingincuda_amd as rt
    from scripts.upscale_probe import _bilinear
    from tests.preview_drive import begin
    a = rt.api
    OW, OH, B, prec = 640, 360, 50, 32
    narrow, wide = _defaults(a, False), _defaults(a, True)
    combos = [dict(zip(SWEEP, v)) for v in itertools.product(*SWEEP.values())]
    out = {"defaults_upscale": _text(narrow), "defaults_upscale_wide": _text(wide)}

    def denoise(r):
        r._check(r._lib.rtiow_denoise(r._h, a.DENOISE_LEVELS, a.DENOISE_SIGMA_COLOR, a.DENOISE_SIGMA_NORMAL, a.DENOISE_SIGMA_ALBEDO, a.DENOISE_SIGMA_DEPTH, None))

    def upscale(r, fn, F, c):
        ms = ctypes.c_float(0)
        r._check(fn(r._h, F, a.UPSCALE_DENOISED, c["sigma_normal"], c["sigma_albedo"], c["sigma_depth"], c["use_coverage"], ctypes.byref(ms), None))
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
                r.accumulate(n)
                denoise(r)
                full[n] = mse(r.read_denoised().astype(np.float64) ** 2)
        for F in FACTORS:
            with rt.Renderer(0, prec) as r:
                begin(r, rt, prec, scene_id, rt.camera(prec, OW // F, OH // F, 1, B))
                r.render_coverage(a.COVERAGE_GRID)
                for n in SAMPLES:
                    s = {"mse_a": full[n]}
                    r.reset_accumulation()
                    r.accumulate(F * F * n)
                    denoise(r)
                    small = r.read_denoised().astype(np.float64) ** 2
                    img, s["ms_upscale"] = upscale(r, r._lib.rtiow_upscale, F, narrow)
                    s["mse_b"] = mse(img)
                    s["mse_d"] = mse(_bilinear(small, F))
                    img, s["ms_upscale_wide_unguided"] = upscale(r, r._lib.rtiow_upscale_wide, F, UNGUIDED)
                    s["mse_s"] = mse(img)
                    s["ms_upscale_wide"] = upscale(r, r._lib.rtiow_upscale_wide, F, wide)[1]
                    s["sweep_mse_w"] = [mse(upscale(r, r._lib.rtiow_upscale_wide, F, c)[0]) for c in combos]
                    rec["F%d_n%d" % (F, n)] = s
        out["scene%d" % scene_id] = rec
    points = [(sc, F, n) for sc in (1, 3) for F in FACTORS for n in SAMPLES]
    at = lambda sc, F, n: out["scene%d" % sc]["F%d_n%d" % (F, n)]
    # the smallest worst case of w / a over scenes and n at F = 2, first of equals in grid order
    worst = [max(at(sc, 2, n)["sweep_mse_w"][k] / at(sc, 2, n)["mse_a"] for sc in (1, 3) for n in SAMPLES) for k in range(len(combos))]
    k = min(range(len(combos)), key=worst.__getitem__)
    out["sweep_grid"] = {name: [str(x) if x == INF else x for x in v] for name, v in SWEEP.items()}
    out["sweep_worst_w_over_a_F2"] = [round(x, 4) for x in worst]
    out["sweep_best"] = dict(_text(combos[k]), worst_w_over_a=round(worst[k], 4))
    out["defaults_are_the_sweeps_best"] = combos[k] == wide
    for sc, F, n in points:
        s = at(sc, F, n)
        s["mse_w"] = s["sweep_mse_w"][k]
        for name, over in (("w_over_a", "mse_a"), ("w_over_b", "mse_b"), ("w_over_d", "mse_d"), ("w_over_s", "mse_s")):
            s[name] = round(s["mse_w"] / s[over], 4)
        s["b_over_d"] = round(s["mse_b"] / s["mse_d"], 4)
        s["s_over_d"] = round(s["mse_s"] / s["mse_d"], 4)
        s["sweep_w_over_a"] = [round(x / s["mse_a"], 4) for x in s.pop("sweep_mse_w")]
    out["pays"] = all(at(*p)["mse_w"] < at(*p)["mse_d"] and at(*p)["mse_w"] < at(*p)["mse_b"] for p in points)
    out["rule"] = "at the sweep's best setting, w < d and w < b at all eight points: scenes 1 and 3, F = 2 and 4, n = 1 and 4"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--skip-payoff", action="store_true")
    ap.add_argument("--skip-cost", action="store_true")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "upscale_wide", "upscale_wide_probe.json"))
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))              # the package and tests/ of the build that is measured
    if a.child:
        kind, *rest = a.child.split(",")
        res = cost(int(rest[0]), int(rest[1]), a.runs, rest[2]) if kind == "cost" else payoff()
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    import raytracingincuda_amd as rt
    record = {"build_id": rt.build_id(), "runs": a.runs, "rounds": a.rounds}

    def child(spec, root=HERE):
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--child", spec, "--runs", str(a.runs), "--root", root]
        p = subprocess.run(cmd, capture_output=True, text=True, cwd=root)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print("child %s failed (exit %d):\n%s\n%s" % (spec, p.returncode, p.stdout[-2000:], p.stderr[-4000:]), file=sys.stderr)
            return None
        return json.loads(line[0][7:])

    if not a.skip_cost:
        arms = [("upscale_wide", HERE, "rtiow_upscale_wide")] + ([("upscale_parent", os.path.abspath(a.parent_root), "rtiow_upscale")] if a.parent_root else [])
        table = record["kernel_ms_1920x1080_to_3840x2160"] = {}
        for scene_id, prec in CONFIGS:
            name = "scene%d_f%d" % (scene_id, prec)
            rounds = {which: [] for which, _, _ in arms}
            for _ in range(a.rounds):                       # the builds alternate, each in a fresh process
                for which, root, call in arms:
                    res = child("cost,%d,%d,%s" % (scene_id, prec, call), root)
                    if res is None:
                        return 1
                    record.setdefault("build_ids", {})[which] = res.pop("build_id")
                    res.pop("call")
                    rounds[which].append(res)
            med = {which: {k: round(statistics.median(r[k] for r in rs), 4) for k in rs[0]} for which, rs in rounds.items()}
            table[name] = dict(med, rounds=rounds)
            if "upscale_parent" in med:
                table[name]["wide_over_parent"] = {k[:-3]: round(med["upscale_wide"][k] / med["upscale_parent"][k], 3) for k in med["upscale_wide"]}
            print(name, json.dumps({k: v for k, v in table[name].items() if k != "rounds"}), flush=True)
    if not a.skip_payoff:
        res = child("payoff")
        if res is None:
            return 1
        record["payoff_640x360_b50_f32"] = res
        record["pays"] = res["pays"]
        print("payoff", json.dumps({k: v for k, v in res.items() if not k.startswith("scene")}), flush=True)
        for sc in (1, 3):
            for key, p in res["scene%d" % sc].items():
                print("scene%d %s" % (sc, key), json.dumps({k: v for k, v in p.items() if k != "sweep_w_over_a"}), flush=True)
        print("pays:", record["pays"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
