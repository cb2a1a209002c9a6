"""Volume scenes on one GPU: render_volume() against render_large() on the same handle, by the rule of
DESIGN.md section 4.28.

For the scenes of tests/volume_scene.py the HIP-event kernel time of rtiow_render_volume and of rtiow_render_large, the median of --runs
after one warm-up each, with the launch's stamped shader clock beside each run.  rtiow_render_large's device code is the parent
commit's, instruction for instruction (profiles/volume_scenes/isa_diff_existing_kernels.txt), so its time on the same handle is the
parent's time.  Frame: 1920 x 1080 at 16 samples, 50 bounces; the camera is outside the cloud and looks at its centre.

The rule (fixed before anything was measured): the feature PAYS if render_volume is faster than render_large on cube(18), cube(27) and
cube(46) in fp32 and on cube(18) in fp64.  Reported, not judged: the flat lattice at 6 000 and 20 000 spheres (where the three-axis grid
is expected to lose a little: ny = 2 and up to twice the index entries), slab_of_layers, gauss_cloud, and cube(27) in fp32 with the
plan's cell-size constant K at 1.0, 1.5 and 2.0 -- builds of the library with -DRTIOW_VOLUME_GRID_K (build.build_variant, names
volume_k15 and volume_k20; a variant that is not built is left out).  Each point runs in a child process under its own `timeout`; the
script stops at the first one that fails.  Writes one JSON record (--out).

    python scripts/volume_scene_probe.py [--runs 5] [--out profiles/volume_scenes/volume_scene_probe.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (scene, precision, judged)
POINTS = [("cube18", 32, True), ("cube27", 32, True), ("cube46", 32, True), ("cube18", 64, True),
          ("flat6000", 32, False), ("flat20000", 32, False), ("slab_of_layers", 32, False), ("gauss_cloud", 32, False)]
K_VARIANTS = [("1.0", None), ("1.5", "volume_k15"), ("2.0", "volume_k20")]
K_SCENE = ("cube27", 32)
FRAME = (1920, 1080)
SAMPLES, BOUNCES = 16, 50
CHILD_TIMEOUT_S = 300


def scene_and_view(name, prec):
    """(scene, lookfrom, lookat): the camera outside the cloud, looking at its centre."""
    from tests import volume_scene
    if name.startswith("cube"):
        side = int(name[4:])
        return volume_scene.cube(side, prec), (2.0 * side, 0.9 * side, 1.2 * side), (0.0, 0.5 * side, 0.0)
    if name.startswith("flat"):
        return volume_scene.flat(prec, int(name[4:])), (13.0, 2.0, 3.0), (0.0, 0.0, 0.0)
    if name == "slab_of_layers":
        return volume_scene.slab_of_layers(prec), (45.0, 12.0, 30.0), (0.0, 1.5, 0.0)
    if name == "gauss_cloud":
        return volume_scene.gauss_cloud(prec), (50.0, 30.0, 30.0), (0.0, 20.0, 0.0)
    raise ValueError(name)


def child(name, prec, runs):
    sys.path.insert(0, HERE)
    import raytracingincuda_amd as rt
    sc, lookfrom, lookat = scene_and_view(name, prec)
    out = {"scene": name, "spheres": int(len(sc["type"])), "precision": prec, "frame": list(FRAME), "samples": SAMPLES, "bounces": BOUNCES,
           "library": os.path.relpath(os.environ["RTIOW_HIP_LIBRARY"], HERE) if os.environ.get("RTIOW_HIP_LIBRARY") else ""}
    with rt.Renderer(0, prec) as r:
        r.set_scene(sc)
        r.set_camera(rt.camera_look(prec, FRAME[0], FRAME[1], SAMPLES, BOUNCES, lookfrom=lookfrom, lookat=lookat, vfov=40.0, defocus_angle=0.0,
                                    focus_dist=10.0))

        def timed(call):
            r.init_rng(1227)
            ms = call()
            return ms, r.stats()

        for which, call in (("render_large", r.render_large), ("render_volume", r.render_volume)):
            timed(call)                                              # warm-up: tables, kernels
            ms, clocks = [], []
            for _ in range(runs):
                t, st = timed(call)
                ms.append(t); clocks.append(st["main_clock_mhz"])
            out[which] = {"ms": ms, "median_ms": statistics.median(ms), "clock_mhz": clocks, "scene_source": st["scene_source"], "vgprs": st["vgprs"],
                          "lds_bytes": st["lds_bytes"], "grid_blocks": st["grid_blocks"]}
        out["large_grid"] = r.large_grid()
        out["volume_grid"] = r.volume_grid()
    out["ratio_volume_over_large"] = out["render_volume"]["median_ms"] / out["render_large"]["median_ms"]
    print(json.dumps(out))


def run_child(name, prec, runs, library=None):
    env = dict(os.environ)
    if library:
        env["RTIOW_HIP_LIBRARY"] = library
    r = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--runs", str(runs), "--child", name, str(prec)],
                       capture_output=True, text=True, env=env)
    if r.returncode != 0:
        print("point (%s, fp%d) failed with status %d: stopping\n%s" % (name, prec, r.returncode, r.stderr[-2000:]), file=sys.stderr)
        return None
    p = json.loads(r.stdout.strip().splitlines()[-1])
    g, v = p["large_grid"], p["volume_grid"]
    print("%-15s fp%d %6d spheres: render_large %9.2f ms (%d x %d, longest %d), render_volume %9.2f ms (%d x %d x %d, longest %d), ratio %.3f" % (
        name, prec, p["spheres"], p["render_large"]["median_ms"], g["nx"], g["nz"], g["longest_list"], p["render_volume"]["median_ms"],
        v["nx"], v["ny"], v["nz"], v["longest_list"], p["ratio_volume_over_large"]), flush=True)
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "volume_scenes", "volume_scene_probe.json"))
    ap.add_argument("--child", nargs=2)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], int(a.child[1]), a.runs)
    if a.runs < 5:
        ap.error("the rule asks for the median of at least five runs")
    points, k_points = [], []
    for name, prec, judged in POINTS:
        p = run_child(name, prec, a.runs)
        if p is None:
            return 1
        p["judged"] = judged
        points.append(p)
    for k, variant in K_VARIANTS:
        lib = os.path.join(HERE, "raytracingincuda_amd", "lib", "ab", variant + ".so") if variant else None
        if lib and not os.path.exists(lib):
            print("K = %s: %s is not built, left out" % (k, lib))
            continue
        p = run_child(K_SCENE[0], K_SCENE[1], a.runs, lib)
        if p is None:
            return 1
        p["K"] = float(k)
        k_points.append(p)
    pays = all(p["render_volume"]["median_ms"] < p["render_large"]["median_ms"] for p in points if p["judged"])
    record = {"rule": "pays if render_volume is faster than render_large on cube(18), cube(27) and cube(46) in fp32 and on cube(18) in fp64; "
                      "the flat lattices, slab_of_layers, gauss_cloud and the K values on cube(27) are reported, not judged",
              "runs": a.runs, "points": points, "K_on_cube27_fp32": k_points, "pays": pays}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("the feature %s" % ("pays" if pays else "does NOT pay yet"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
