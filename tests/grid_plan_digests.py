"""One SHA-256 per scene over everything the two plan hooks return (rtiow_debug_grid_plan, rtiow_debug_large_grid_plan: host arithmetic
of the test build, no GPU): dims and params as raw bytes, cells, indices where the plan has them, the direct list, the half-widths and
the usable flag.  tests/golden/make_grid_plan_digests.py records them for a build, tests/test_grid_plan_digests.py holds the working
tree to the record: a restatement of the plans' arithmetic has to return the same bits.

The scenes are those of tests/test_grid_plan.py (restated here: that file builds them inline) and of tests/large_scene.py."""
import ctypes
import hashlib

import numpy as np

from tests import large_scene
from tests.conftest import compact

_f64p = ctypes.POINTER(ctypes.c_double)


def lds_scenes(oracle):
    """{name: (spheres [n, 4], centre [3])} for rtiow_debug_grid_plan: reference scenes 1-3 in both precisions, the twelve seeds of
    test_grid_plan.test_random_scenes and the three scenes of test_declines_unsuitable_scenes, centred as that file centres them."""
    out = {}

    def add(name, cr, centre=None):
        cr = np.ascontiguousarray(cr, np.float64)
        out[name] = (cr, cr[cr[:, 3] < 100.0, :3].mean(axis=0) if centre is None else np.asarray(centre, np.float64))

    for scene_id in (1, 2, 3):
        for prec in (32, 64):
            add("reference_scene%d_f%d" % (scene_id, prec), compact(oracle.build_scene(scene_id, prec))["center_radius"])
    for seed in range(12):
        rng = np.random.default_rng(seed)
        n = int(rng.integers(30, 900))
        half = float(rng.uniform(2, 40))
        off = rng.uniform(-50, 50, 3) if seed % 3 == 0 else np.zeros(3)
        r = [np.full(n, 0.2), rng.uniform(0.02, 0.6, n), np.exp(rng.uniform(np.log(0.005), np.log(2.0), n)), rng.choice([0.1, 0.45, 1.0], n)][seed % 4]
        cr = np.column_stack([rng.uniform(-half, half, n) + off[0], r + rng.uniform(0, 3, n) * (seed % 2) + off[1], rng.uniform(-half, half, n) + off[2], r])
        add("random_seed%d" % seed, np.vstack([[off[0], off[1] - 1000.0, off[2], 1000.0], cr]))
    rng = np.random.default_rng(0)
    add("declined_few", np.column_stack([rng.uniform(-5, 5, 20), np.full(20, 0.2), rng.uniform(-5, 5, 20), np.full(20, 0.2)]))
    add("declined_dense", np.column_stack([rng.uniform(-1, 1, 400), np.full(400, 0.2), rng.uniform(-1, 1, 400), np.full(400, 0.2)]))
    bad = np.column_stack([rng.uniform(-5, 5, 60), np.full(60, 0.2), rng.uniform(-5, 5, 60), np.full(60, 0.2)])
    bad[5, 0] = np.nan; bad[6, 3] = -0.2; bad[7, 3] = np.inf
    add("declined_bad", bad, centre=np.zeros(3))
    return out


def large_scenes():
    """{name: scene} for rtiow_debug_large_grid_plan: the scenes tests/test_render_large.py and tests/test_render_large_edges.py render."""
    out = {"lattice6000_f32": large_scene.lattice(6000, 32), "lattice6000_f64": large_scene.lattice(6000, 64), "lattice20000_f32": large_scene.lattice(20000, 32),
           "line2000_f32": large_scene.line(2000, 32), "line2000_f64": large_scene.line(2000, 64), "ten_spheres": large_scene.ten_spheres()}
    for prec in (32, 64):
        for name in large_scene.EDGE_SCENES:
            out["edge_%s_f%d" % (name, prec)] = large_scene.edge_scene(name, prec)
        for case in large_scene.RANDOM_CASES:
            out["random_%s_f%d" % (case, prec)] = large_scene.random_case(case)[prec]
    return out


def _digest(usable, *arrays):
    h = hashlib.sha256(b"usable" if usable else b"unusable")
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(("|%s%d|" % (a.dtype.str, a.size)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def lds_digest(native, cr, centre):
    lib = native.load_hip_library(debug=True)
    n = len(cr)
    centre = np.ascontiguousarray(centre, np.float64)
    dims, params = np.zeros(4, np.int32), np.zeros(8, np.float64)
    cells, direct, hw = np.zeros(4096 * 4, np.uint16), np.zeros(n, np.int32), np.zeros(n, np.float64)
    rc = lib.rtiow_debug_grid_plan(n, cr.ctypes.data_as(_f64p), centre.ctypes.data_as(_f64p), dims.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                   params.ctypes.data_as(_f64p), cells.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)), cells.size,
                                   direct.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), direct.size, hw.ctypes.data_as(_f64p))
    assert rc in (0, 1), rc
    nx, nz, _, nd = (int(v) for v in dims)
    return _digest(rc == 1, dims, params, cells[:nx * nz * 4], direct[:nd], hw)


def large_digest(native, scene):
    cr = np.asarray(scene["center_radius"], np.float64)
    pl = native.debug_large_grid_plan(cr, large_scene.centre(scene), tables=True)
    dims = np.array([pl[k] for k in ("nx", "nz", "registered", "direct", "index_entries", "longest_list")], np.int32)
    params = np.array([pl[k] for k in ("x0", "z0", "cell", "ylo", "yhi", "rfar", "eps", "cmax")], np.float64)
    none = np.zeros(0, np.uint32)
    return _digest(pl["usable"], dims, params, pl.get("cells", none), pl.get("indices", none), pl.get("direct_list", none.astype(np.int32)), pl.get("halfwidth", np.zeros(0)))


def all_digests(native, oracle):
    """{"grid_plan": {name: sha256}, "large_grid_plan": {name: sha256}} of the loaded test build."""
    return {"grid_plan": {name: lds_digest(native, cr, centre) for name, (cr, centre) in lds_scenes(oracle).items()},
            "large_grid_plan": {name: large_digest(native, sc) for name, sc in large_scenes().items()}}
