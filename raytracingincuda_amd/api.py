"""ctypes mirror of the C-ABI (include/rtiow.h, include/rtiow_host.h).

The call sequence a user writes mirrors the phases of the reference's main()
(/root/reference/src/GlobalFloatCUDAInOneWeekend/main.cu:37-400):

    cam   = camera(32, width, height, samples, bounces)      # main.cu:100-124
    scene = build_scene(scene_id, 32)                        # main.cu:148-296
    r = Renderer(device=0, precision=32)                     # main.cu:81-92
    r.set_camera(cam); r.set_scene(scene)                    # main.cu:301-321
    r.init_rng(1227)                                         # main.cu:326-330
    ms  = r.render(threads=8)                                # main.cu:334-341
    rgb = r.read_framebuffer()                               # main.cu:373
    write_ppm(ppm_filename(32, scene_id, ...), rgb)          # main.cu:349-379

There is no CPU fallback: if librtiow_hip.so is missing or no GPU is visible the calls
raise.  (The CPU oracle lives in oracle/ and is test infrastructure only.)
"""
import ctypes
import math
import os
import sys

import numpy as np

LAMBERTIAN, METAL, DIELECTRIC = 0, 1, 2
SCENE_LDS, SCENE_SCALAR, SCENE_LDS_EXACT, SCENE_GRID = 0, 1, 2, 3
SCENE_DEVICE_GRID = 4                                       # what stats()["scene_source"] reads after render_large(); set_scene_source refuses it
SCENE_VOLUME_GRID = 5                                       # what stats()["scene_source"] reads after render_volume(); set_scene_source refuses it
SCHED_STATIC, SCHED_PERSISTENT, SCHED_SORTED = 0, 1, 2
GATHER_AUTO, GATHER_RCCL, GATHER_PEER, GATHER_HOST = 0, 1, 2, 3
GUIDES_FIRST_HIT, GUIDES_SPECULAR = 0, 1  # rtiow_set_guide_mode
UPSCALE_DENOISED, UPSCALE_LINEAR, UPSCALE_HISTORY = 0, 1, 2  # rtiow_upscale's source
GROUP_MAX_STATS = 16
ABI_VERSION = 6          # include/rtiow.h RTIOW_ABI_VERSION

_PKG = os.path.dirname(os.path.abspath(__file__))
_LIBDIR = os.path.join(_PKG, "lib")


class RtiowError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("rtiow error %d: %s" % (code, message))
        self.code = code


class CameraF32(ctypes.Structure):
    _fields_ = [("img_width", ctypes.c_int32), ("img_height", ctypes.c_int32),
                ("samples_per_pixel", ctypes.c_int32), ("max_depth", ctypes.c_int32),
                ("pixel_samples_scale", ctypes.c_float),
                ("center", ctypes.c_float * 3), ("pixel00_loc", ctypes.c_float * 3),
                ("pixel_delta_u", ctypes.c_float * 3), ("pixel_delta_v", ctypes.c_float * 3),
                ("defocus_angle", ctypes.c_float),
                ("defocus_disk_u", ctypes.c_float * 3), ("defocus_disk_v", ctypes.c_float * 3)]


class CameraF64(ctypes.Structure):
    _fields_ = [("img_width", ctypes.c_int32), ("img_height", ctypes.c_int32),
                ("samples_per_pixel", ctypes.c_int32), ("max_depth", ctypes.c_int32),
                ("pixel_samples_scale", ctypes.c_double),
                ("center", ctypes.c_double * 3), ("pixel00_loc", ctypes.c_double * 3),
                ("pixel_delta_u", ctypes.c_double * 3), ("pixel_delta_v", ctypes.c_double * 3),
                ("defocus_angle", ctypes.c_double),
                ("defocus_disk_u", ctypes.c_double * 3), ("defocus_disk_v", ctypes.c_double * 3)]


class Stats(ctypes.Structure):
    _fields_ = [("rng_init_ms", ctypes.c_double), ("render_ms", ctypes.c_double),
                ("primary_rays", ctypes.c_uint64), ("local_rows", ctypes.c_int32),
                ("num_spheres", ctypes.c_int32), ("block_x", ctypes.c_int32), ("block_y", ctypes.c_int32),
                ("vgprs", ctypes.c_int32), ("sgprs", ctypes.c_int32), ("lds_bytes", ctypes.c_int32),
                ("scene_source", ctypes.c_int32),
                ("schedule", ctypes.c_int32), ("grid_blocks", ctypes.c_int32), ("phases", ctypes.c_int32),
                ("prepass_samples", ctypes.c_int32), ("prepass_ms", ctypes.c_double), ("main_ms", ctypes.c_double),
                ("segments_prepass", ctypes.c_uint64), ("segments_main", ctypes.c_uint64),
                ("max_chain_prepass", ctypes.c_uint64), ("max_chain_main", ctypes.c_uint64),
                ("grid_nx", ctypes.c_int32), ("grid_nz", ctypes.c_int32), ("grid_registered", ctypes.c_int32),
                ("grid_direct", ctypes.c_int32), ("grid_cell", ctypes.c_double),
                ("solo_waves", ctypes.c_int32), ("solo_lanes", ctypes.c_int32), ("scene_prepare_ms", ctypes.c_double),
                ("staged_stores", ctypes.c_int32), ("num_cus", ctypes.c_int32), ("place_ms", ctypes.c_double),
                ("clock_mhz", ctypes.c_int32), ("order_reused", ctypes.c_int32),
                ("main_clock_mhz", ctypes.c_double), ("prepass_clock_mhz", ctypes.c_double), ("main_wave0_ms", ctypes.c_double)]


class LargeGridInfo(ctypes.Structure):
    """rtiow_large_grid_info (include/rtiow.h)."""
    _fields_ = [("usable", ctypes.c_int32), ("nx", ctypes.c_int32), ("nz", ctypes.c_int32), ("cell", ctypes.c_double), ("rfar", ctypes.c_double),
                ("registered", ctypes.c_int32), ("direct", ctypes.c_int32), ("index_entries", ctypes.c_uint64), ("longest_list", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("blob_bytes", ctypes.c_uint64)]


class VolumeGridInfo(ctypes.Structure):
    """rtiow_volume_grid_info (include/rtiow.h)."""
    _fields_ = [("usable", ctypes.c_int32), ("nx", ctypes.c_int32), ("ny", ctypes.c_int32), ("nz", ctypes.c_int32), ("cell", ctypes.c_double),
                ("rfar", ctypes.c_double), ("registered", ctypes.c_int32), ("direct", ctypes.c_int32), ("index_entries", ctypes.c_uint64),
                ("occupied_cells", ctypes.c_uint64), ("longest_list", ctypes.c_int32), ("reserved", ctypes.c_int32), ("blob_bytes", ctypes.c_uint64)]


class GroupStats(ctypes.Structure):
    _fields_ = [("ngpus", ctypes.c_int32), ("strip_rows", ctypes.c_int32), ("gather_mode", ctypes.c_int32),
                ("rccl_version", ctypes.c_int32), ("kernel_ms", ctypes.c_double * GROUP_MAX_STATS),
                ("kernel_ms_max", ctypes.c_double), ("gather_ms", ctypes.c_double), ("gather_bytes", ctypes.c_uint64),
                ("create_ms", ctypes.c_double), ("peer_links", ctypes.c_int32), ("reserved", ctypes.c_int32)]


# The C types the headers use, by the names the tables below spell them with.
_int, _dbl, _size, _u64, _str, _vp = ctypes.c_int, ctypes.c_double, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_void_p
_H = _G = ctypes.c_void_p                                   # rtiow_handle, rtiow_group
_intp, _i32p, _i64p = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
_u8p, _u16p, _u32p, _u64p = (ctypes.POINTER(t) for t in (ctypes.c_ubyte, ctypes.c_uint16, ctypes.c_uint32, ctypes.c_uint64))
_f32p, _f64p, _sizep, _vpp = (ctypes.POINTER(t) for t in (ctypes.c_float, ctypes.c_double, ctypes.c_size_t, ctypes.c_void_p))

# One row per function, in the order of its header: symbol -> argtypes.  The loaders below declare every row on the library they open;
# tests, probe scripts and the wrappers below all call through these declarations.  Every function returns int but those of RESTYPES.
HIP_ABI = {                                                 # include/rtiow.h: librtiow_hip.so and the test build
    "rtiow_abi_version": (),
    "rtiow_build_id": (),
    "rtiow_create": (_int, _int, ctypes.POINTER(_H)),
    "rtiow_destroy": (_H,),
    "rtiow_last_error_string": (_H,),
    "rtiow_set_stream": (_H, _vp),
    "rtiow_set_scene": (_H, _int, _vp, _vp, _vp, _i32p, _i32p),
    "rtiow_set_camera": (_H, _vp),
    "rtiow_set_shard": (_H, _int, _int, _int),
    "rtiow_local_rows": (_H, _intp),
    "rtiow_local_row_map": (_H, _i32p),
    "rtiow_init_rng": (_H, _u64),
    "rtiow_render": (_H, _int, _f32p),
    "rtiow_render_async": (_H, _int),
    "rtiow_render_wait": (_H, _f32p),
    "rtiow_count_segments": (_H, _int, _u64p),
    "rtiow_accumulate_reset": (_H,),
    "rtiow_accumulate": (_H, _int, _int, _f32p),
    "rtiow_accumulated_samples": (_H, _intp),
    "rtiow_accumulate_adaptive": (_H, _int, _int, _dbl, _int, _f32p, _intp),
    "rtiow_read_adaptive_state": (_H, _i32p, _f32p, _size),
    "rtiow_read_linear": (_H, _vp, _size),
    "rtiow_render_guides": (_H, _f32p),
    "rtiow_read_guides": (_H, _vp, _vp, _vp, _size),
    "rtiow_denoise": (_H, _int, _dbl, _dbl, _dbl, _dbl, _f32p),
    "rtiow_read_denoised": (_H, _vp, _size),
    "rtiow_denoised_device_ptr": (_H, _vpp, _sizep),
    "rtiow_read_variance": (_H, _vp, _size),
    "rtiow_denoise_variance": (_H, _int, _dbl, _dbl, _dbl, _dbl, _f32p),
    "rtiow_history_reset": (_H,),
    "rtiow_history_update": (_H, _dbl, _dbl, _dbl, _f32p, _u64p),
    "rtiow_history_commit": (_H,),
    "rtiow_read_history": (_H, _vp, _vp, _size),
    "rtiow_history_device_ptr": (_H, _vpp, _sizep),
    "rtiow_denoise_history": (_H, _int, _dbl, _dbl, _dbl, _dbl, _f32p),
    "rtiow_set_guide_mode": (_H, _int, _int, _dbl),
    "rtiow_read_filter_guides": (_H, _vp, _vp, _vp, _i32p, _size),
    "rtiow_history_plan": (_H, _dbl, _dbl, _dbl, _f32p, _u64p),
    "rtiow_read_history_plan": (_H, _vp, _size),
    "rtiow_accumulate_budget": (_H, _int, _int, _dbl, _int, _f32p, _intp),
    "rtiow_history_update_clipped": (_H, _dbl, _dbl, _dbl, _int, _dbl, _f32p, _u64p, _u64p),
    "rtiow_denoise_history_variance": (_H, _int, _dbl, _dbl, _dbl, _dbl, _int, _f32p),
    "rtiow_read_history_variance": (_H, _vp, _size),
    "rtiow_history_commit_filtered": (_H, _dbl, _dbl, _dbl, _dbl, _dbl, _f32p),
    "rtiow_read_history_base": (_H, _vp, _vp, _size),
    "rtiow_render_coverage": (_H, _int, _f32p),
    "rtiow_read_coverage": (_H, _i32p, _i32p, _vp, _vp, _size),
    "rtiow_resolve_edges": (_H, _int, _dbl, _dbl, _dbl, _f32p, _u64p),
    "rtiow_set_guide_lens": (_H, _int),
    "rtiow_edit_scene": (_H, _int, _vp, _vp, _vp, _i32p, _i32p),
    "rtiow_read_scene_motion": (_H, _vp, _i32p, _i32p, _size),
    "rtiow_set_edit_influence": (_H, _dbl),
    "rtiow_read_edit_influence": (_H, _vp, _size),
    "rtiow_edit_scene_mapped": (_H, _int, _vp, _vp, _vp, _i32p, _i32p, _i32p),
    "rtiow_read_scene_origin": (_H, _i32p, _size),
    "rtiow_upscale": (_H, _int, _int, _dbl, _dbl, _dbl, _int, _f32p, _u64p),
    "rtiow_read_upscaled": (_H, _vp, _size),
    "rtiow_upscaled_device_ptr": (_H, _vpp, _sizep),
    "rtiow_upscale_wide": (_H, _int, _int, _dbl, _dbl, _dbl, _int, _f32p, _u64p),
    "rtiow_render_large": (_H, _f32p),
    "rtiow_read_large_grid": (_H, ctypes.POINTER(LargeGridInfo)),
    "rtiow_accumulate_large": (_H, _int, _f32p),
    "rtiow_accumulate_adaptive_large": (_H, _int, _int, _dbl, _int, _f32p, _intp),
    "rtiow_accumulate_budget_large": (_H, _int, _int, _dbl, _int, _f32p, _intp),
    "rtiow_render_guides_large": (_H, _f32p),
    "rtiow_render_coverage_large": (_H, _int, _f32p),
    "rtiow_upscale_large": (_H, _int, _int, _dbl, _dbl, _dbl, _int, _f32p, _u64p),
    "rtiow_upscale_wide_large": (_H, _int, _int, _dbl, _dbl, _dbl, _int, _f32p, _u64p),
    "rtiow_render_volume": (_H, _f32p),
    "rtiow_read_volume_grid": (_H, ctypes.POINTER(VolumeGridInfo)),
    "rtiow_accumulate_volume": (_H, _int, _f32p),
    "rtiow_accumulate_adaptive_volume": (_H, _int, _int, _dbl, _int, _f32p, _intp),
    "rtiow_accumulate_budget_volume": (_H, _int, _int, _dbl, _int, _f32p, _intp),
    "rtiow_render_guides_volume": (_H, _f32p),
    "rtiow_render_coverage_volume": (_H, _int, _f32p),
    "rtiow_upscale_volume": (_H, _int, _int, _dbl, _dbl, _dbl, _int, _f32p, _u64p),
    "rtiow_upscale_wide_volume": (_H, _int, _int, _dbl, _dbl, _dbl, _int, _f32p, _u64p),
    "rtiow_bind_framebuffer": (_H, _vp, _size),
    "rtiow_framebuffer_device_ptr": (_H, _vpp, _sizep),
    "rtiow_read_framebuffer": (_H, _vp, _size),
    "rtiow_read_levels": (_H, _u8p, _size, _u64p),
    "rtiow_set_scene_source": (_H, _int),
    "rtiow_set_schedule": (_H, _int, _int),
    "rtiow_get_stats": (_H, ctypes.POINTER(Stats)),
    "rtiow_synchronize": (_H,),
    "rtiow_stream": (_H, _vpp),
    "rtiow_device": (_H, _intp),
    "rtiow_group_create": (_int, _intp, _int, _int, _int, ctypes.POINTER(_G)),
    "rtiow_group_create_error": (),
    "rtiow_group_destroy": (_G,),
    "rtiow_group_last_error_string": (_G,),
    "rtiow_group_size": (_G,),
    "rtiow_group_member": (_G, _int, ctypes.POINTER(_H)),
    "rtiow_group_set_scene": (_G, _int, _vp, _vp, _vp, _i32p, _i32p),
    "rtiow_group_set_camera": (_G, _vp),
    "rtiow_group_set_scene_source": (_G, _int),
    "rtiow_group_set_schedule": (_G, _int, _int),
    "rtiow_group_init_rng": (_G, _u64),
    "rtiow_group_render": (_G, _int, _f32p),
    "rtiow_group_gather": (_G,),
    "rtiow_group_framebuffer_device_ptr": (_G, _vpp, _sizep),
    "rtiow_group_read_framebuffer": (_G, _vp, _size),
    "rtiow_group_get_stats": (_G, ctypes.POINTER(GroupStats)),
    "rtiow_group_transport_note": (_G,),
}
# include/rtiow_debug.h: exported by lib/librtiow_hip_debug.so (the test build) only.  Its two hooks of instrumented builds
# (rtiow_debug_region_cycles, rtiow_debug_path_stats) are in no library built here and stay out.
DEBUG_ABI = {
    "rtiow_debug_read_rng": (_H, _u32p, _size),
    "rtiow_debug_read_costs": (_H, _u32p, _u32p, _size),
    "rtiow_debug_read_order": (_H, _i32p, _i32p, _size, _i32p, _u32p, _size),
    "rtiow_debug_read_chunk_costs": (_H, _u32p, _size),
    "rtiow_debug_poison_staged": (_H,),
    "rtiow_debug_timeline": (_H, _int, _u64p, _size, _intp),
    "rtiow_debug_pixel_times": (_H, _int, _u32p, _size),
    "rtiow_debug_ops": (_H, _int, _size, _vp, _vp, _vp, _vp),
    "rtiow_debug_hit_world": (_H, _int, _vp, _vp, _i32p),
    "rtiow_debug_scatter": (_H, _int, _int, _vp, _i32p, _u32p, _vp, _i32p, _u32p, _intp),
    "rtiow_debug_jump_matrices": (_u32p, _size, _int),
    "rtiow_debug_grid_plan": (_int, _f64p, _f64p, _i32p, _f64p, _u16p, _size, _i32p, _size, _f64p),
    "rtiow_debug_large_grid_plan": (_int, _f64p, _f64p, _i32p, _f64p, _u32p, _size, _u32p, _size, _i32p, _size, _f64p),
    "rtiow_debug_hit_world_large": (_H, _int, _vp, _vp, _i32p, _i32p),
    "rtiow_debug_volume_grid_plan": (_int, _f64p, _f64p, ctypes.c_int64, _i32p, _f64p, _u32p, _size, _u32p, _size, _i32p, _size, _f64p),
    "rtiow_debug_hit_world_volume": (_H, _int, _vp, _vp, _i32p, _i32p),
    "rtiow_debug_gather_schedule": (_int, _intp, _intp, _int, _int, _int, _int, _i64p, _size, _intp),
}
HOST_ABI = {                                                # include/rtiow_host.h: librtiow_host.so
    "rtiow_host_scene_slots": (_int,),
    "rtiow_host_build_scene": (_int, _int, _vp, _vp, _vp, _i32p, _i32p),
    "rtiow_host_camera": (_int, _int, _int, _int, _int, _vp),
    "rtiow_host_camera_look": (_int, _int, _int, _int, _int, _f64p, _f64p, _f64p, _dbl, _dbl, _dbl, _vp),
    "rtiow_host_ppm_filename": (_int, _int, _int, _int, _int, _int, _int, _str, _size),
    "rtiow_host_write_ppm": (_str, _int, _int, _int, _vp),
    "rtiow_host_format_ppm": (_int, _int, _int, _vp, _str, _size, _sizep),
    "rtiow_host_write_ppm_binary": (_str, _int, _int, _int, _vp),
    "rtiow_host_write_ppm_levels": (_str, _int, _int, _u8p, _int),
    "rtiow_host_levels": (_int, _int, _int, _vp, _u8p),
    "rtiow_host_shard_rows": (_int, _int, _int, _int, _i32p),
    "rtiow_host_place_rows": (_int, _int, _int, _int, _int, _int, _vp, _vp),
}
RESTYPES = {"rtiow_build_id": _str, "rtiow_last_error_string": _str, "rtiow_group_create_error": _str, "rtiow_group_last_error_string": _str,
            "rtiow_group_transport_note": _str, "rtiow_host_levels": ctypes.c_longlong}
HIP_SYMBOLS, DEBUG_SYMBOLS, HOST_SYMBOLS = list(HIP_ABI), list(DEBUG_ABI), list(HOST_ABI)
ORDER_NONE, ORDER_RENDER, ORDER_ACCUMULATE, ORDER_ADAPTIVE = 0, 1, 2, 3     # rtiow_debug_read_order: info["kind"]
ORDER_INFO_FIELDS = ("kind", "total_slots", "solo_slots", "total_pools", "pools_per_block", "deal_group", "lane_cap", "blocks", "n_active", "W", "local_rows")

_loaded = {}


def lib_paths():
    # RTIOW_HIP_LIBRARY: another build of the same C-ABI (A/B timing of kernel variants, the stats build)
    # "hip_debug": the test build (the same kernels + the hooks of include/rtiow_debug.h); RTIOW_HIP_DEBUG_LIBRARY: another build of it
    return {"hip": os.environ.get("RTIOW_HIP_LIBRARY") or os.path.join(_LIBDIR, "librtiow_hip.so"),
            "hip_debug": os.environ.get("RTIOW_HIP_DEBUG_LIBRARY") or os.path.join(_LIBDIR, "librtiow_hip_debug.so"),
            "host": os.path.join(_LIBDIR, "librtiow_host.so")}


def _load(which, *tables):
    """dlopen lib_paths()[which] once and declare every row of the tables on it.  Raises loudly when it is missing: no fallback."""
    if which not in _loaded:
        path = lib_paths()[which]
        if not os.path.exists(path):
            raise RtiowError(-100, "%s not built; run `python -m raytracingincuda_amd.build`" % path)
        lib = ctypes.CDLL(path)
        for table in tables:
            for symbol, argtypes in table.items():
                fn = getattr(lib, symbol)
                fn.argtypes = argtypes
                if symbol in RESTYPES:
                    fn.restype = RESTYPES[symbol]
        _loaded[which] = lib
    return _loaded[which]


def load_host_library():
    return _load("host", HOST_ABI)


def load_hip_library(debug=False):
    """Load librtiow_hip.so -- or, debug=True, the test build librtiow_hip_debug.so, which also exports the hooks of
    include/rtiow_debug.h.  Raises loudly when it is missing: there is no fallback path."""
    return _load("hip_debug", HIP_ABI, DEBUG_ABI) if debug else _load("hip", HIP_ABI)


def build_id():
    """rtiow_build_id() of the loaded HIP library: SHA-256 of the sources + flags it was built from."""
    return load_hip_library().rtiow_build_id().decode()


def _dtype(precision):
    if precision == 32:
        return np.float32
    if precision == 64:
        return np.float64
    raise ValueError("precision must be 32 or 64")


def scene_slots(scene_id):
    return load_host_library().rtiow_host_scene_slots(int(scene_id))


def build_scene(scene_id, precision=32):
    """World creation, main.cu:148-296.  Returns a dict of numpy arrays in slot order
    (center_radius [n,4], albedo_fuzz [n,4], refraction_index [n], type [n], valid [n])."""
    lib = load_host_library()
    dt = _dtype(precision)
    n = lib.rtiow_host_scene_slots(int(scene_id))
    cr = np.zeros((n, 4), dt); af = np.zeros((n, 4), dt); ri = np.zeros(n, dt)
    ty = np.zeros(n, np.int32); va = np.zeros(n, np.int32)
    got = lib.rtiow_host_build_scene(int(scene_id), precision, cr.ctypes.data, af.ctypes.data, ri.ctypes.data,
                                     ty.ctypes.data_as(_i32p),
                                     va.ctypes.data_as(_i32p))
    if got != n:
        raise RtiowError(got, "rtiow_host_build_scene failed")
    return {"scene_id": int(scene_id), "precision": precision, "center_radius": cr, "albedo_fuzz": af,
            "refraction_index": ri, "type": ty, "valid": va}


def compact_scene(scene):
    """Drop the slots the reference leaves default-constructed (main.cu:168)."""
    keep = scene["valid"] != 0
    out = dict(scene)
    for k in ("center_radius", "albedo_fuzz", "refraction_index", "type", "valid"):
        out[k] = np.ascontiguousarray(scene[k][keep])
    return out


def camera(precision, width, height, samples, bounces):
    """camera configuration + camera::initialize (main.cu:100-124, camera.h:33-68)."""
    lib = load_host_library()
    cam = CameraF64() if precision == 64 else CameraF32()
    _dtype(precision)
    rc = lib.rtiow_host_camera(precision, int(width), int(height), int(samples), int(bounces), ctypes.addressof(cam))
    if rc:
        raise RtiowError(rc, "rtiow_host_camera: bad arguments")
    return cam


def camera_look(precision, width, height, samples, bounces, lookfrom=(13.0, 2.0, 3.0), lookat=(0.0, 0.0, 0.0), vup=(0.0, 1.0, 0.0),
                vfov=20.0, defocus_angle=0.6, focus_dist=10.0):
    """camera::initialize (camera.h:33-68) for a placement of the caller's; the defaults are the reference's (main.cu:114-121), with
    which this is camera() byte for byte.  Every argument is rounded to the precision on entry."""
    lib = load_host_library()
    cam = CameraF64() if precision == 64 else CameraF32()
    _dtype(precision)
    v3 = lambda v: (ctypes.c_double * 3)(*[float(x) for x in v])
    rc = lib.rtiow_host_camera_look(precision, int(width), int(height), int(samples), int(bounces), v3(lookfrom), v3(lookat), v3(vup),
                                    float(vfov), float(defocus_angle), float(focus_dist), ctypes.addressof(cam))
    if rc:
        raise RtiowError(rc, "rtiow_host_camera_look: bad arguments")
    return cam


def ppm_filename(precision, scene_id, width, height, samples, bounces, threads):
    buf = ctypes.create_string_buffer(256)
    rc = load_host_library().rtiow_host_ppm_filename(precision, scene_id, width, height, samples, bounces, threads, buf, 256)
    if rc:
        raise RtiowError(rc, "rtiow_host_ppm_filename failed")
    return buf.value.decode()


def _rgb_precision(rgb):
    if rgb.dtype == np.float32:
        return 32
    if rgb.dtype == np.float64:
        return 64
    raise ValueError("rgb must be float32 or float64")


def format_ppm(rgb):
    """P3 text of an [H, W, 3] image, main.cu:368-379."""
    rgb = np.ascontiguousarray(rgb)
    h, w = rgb.shape[0], rgb.shape[1]
    lib = load_host_library()
    n = ctypes.c_size_t(0)
    p = _rgb_precision(rgb)
    rc = lib.rtiow_host_format_ppm(p, w, h, rgb.ctypes.data, None, 0, ctypes.byref(n))
    if rc:
        raise RtiowError(rc, "rtiow_host_format_ppm failed")
    buf = ctypes.create_string_buffer(n.value)
    rc = lib.rtiow_host_format_ppm(p, w, h, rgb.ctypes.data, buf, n.value, ctypes.byref(n))
    if rc:
        raise RtiowError(rc, "rtiow_host_format_ppm failed")
    return buf.raw[:n.value]


def write_ppm(path, rgb, binary=False):
    """P3 text file exactly as main.cu:368-379 writes it; binary=True writes the P6 twin (same levels)."""
    rgb = np.ascontiguousarray(rgb)
    lib = load_host_library()
    fn = lib.rtiow_host_write_ppm_binary if binary else lib.rtiow_host_write_ppm
    rc = fn(os.fsencode(path), _rgb_precision(rgb), rgb.shape[1], rgb.shape[0], rgb.ctypes.data)
    if rc:
        raise RtiowError(rc, "Could not open file for writing: %s" % path)


def levels(rgb):
    """(levels, nan_channels): main.cu:367, 374-376 per channel on the host, uint8 [H, W, 3] (what rtiow_read_levels computes on the device)."""
    rgb = np.ascontiguousarray(rgb)
    out = np.empty(rgb.shape, np.uint8)
    n = load_host_library().rtiow_host_levels(_rgb_precision(rgb), rgb.shape[1], rgb.shape[0], rgb.ctypes.data, out.ctypes.data_as(_u8p))
    if n < 0:
        raise RtiowError(int(n), "rtiow_host_levels: bad arguments")
    return out, int(n)


def write_ppm_levels(path, lev, binary=False):
    """The P3 / P6 file from levels (uint8 [H, W, 3]): threaded formatter, every thread writes its own range of the file."""
    lev = np.ascontiguousarray(lev, np.uint8)
    rc = load_host_library().rtiow_host_write_ppm_levels(os.fsencode(path), lev.shape[1], lev.shape[0], lev.ctypes.data_as(_u8p), 1 if binary else 0)
    if rc:
        raise RtiowError(rc, "Could not open file for writing: %s" % path)


def shard_rows(height, rank, nranks, strip_rows=8):
    """Global row indices rendered by `rank` (same rule as rtiow_set_shard)."""
    lib = load_host_library()
    n = lib.rtiow_host_shard_rows(height, rank, nranks, strip_rows, None)
    if n < 0:
        raise RtiowError(n, "rtiow_host_shard_rows: bad arguments")
    rows = np.zeros(n, np.int32)
    if n:
        lib.rtiow_host_shard_rows(height, rank, nranks, strip_rows, rows.ctypes.data_as(_i32p))
    return rows


def place_rows(full_rgb, local_rgb, rank, nranks, strip_rows):
    """Scatter one shard's rows (rtiow_set_shard order) into the full [H, W, 3] image."""
    assert full_rgb.flags.c_contiguous and local_rgb.flags.c_contiguous and full_rgb.dtype == local_rgb.dtype
    rc = load_host_library().rtiow_host_place_rows(_rgb_precision(full_rgb), full_rgb.shape[1], full_rgb.shape[0],
                                                   rank, nranks, strip_rows, local_rgb.ctypes.data, full_rgb.ctypes.data)
    if rc:
        raise RtiowError(rc, "rtiow_host_place_rows: bad arguments")
    return full_rgb


# Renderer.denoise defaults: the best of scripts/denoise_probe.py --sweep, i.e. the smallest worse-of-two MSE ratio on scenes 1 and 3
# at 320 x 180 and 16 samples against 1024 (profiles/denoise/denoise_probe.json).
DENOISE_LEVELS = 5
DENOISE_SIGMA_COLOR = 0.1
DENOISE_SIGMA_NORMAL = 0.1
DENOISE_SIGMA_ALBEDO = 0.2
DENOISE_SIGMA_DEPTH = 0.05
# Renderer.denoise_variance default: the best of scripts/denoise_variance_probe.py --sweep, i.e. the smallest worst case over 4, 16 and
# 64 uniform samples of the worse-of-two-scenes ratio q_var / q_fixed, q = MSE ratio as above, q_fixed from denoise() at its defaults
# (profiles/denoise_variance/denoise_variance_probe.json).  Dimensionless: a tolerance in standard deviations.
DENOISE_SIGMA_VARIANCE = 4.5


# Renderer.history_update defaults: the best of scripts/history_probe.py --sweep, i.e. the smallest worse-of-two-scenes MSE ratio of
# the temporal image against the noisy one at the end of an 8-frame orbit, 320 x 180, 4 samples a frame, against 1024 samples
# (profiles/history/history_probe.json).
HISTORY_DEPTH_TOL = 0.1
HISTORY_NORMAL_COS = 0.9
HISTORY_MAX = 16.0
# Renderer.accumulate_budget defaults (with history_plan at the history defaults above): the eligible setting of
# scripts/history_budget_probe.py's sweep with the smallest worse-of-two-scenes ratio of whole-frame MSE to the uniform walk's, on the
# walk above; eligible: no more primary rays than that walk.  At these the disoccluded pixels' MSE is a quarter of the uniform walk's
# and the whole frame's is 1.14 to 1.21 times it: no eligible setting lowers the whole frame's
# (profiles/history_budget/history_budget_probe.json).
BUDGET_TARGET = 16.0
BUDGET_MIN_SAMPLES = 1
BUDGET_CHUNK = 2
# Renderer.history_update_clipped defaults: the best of scripts/history_clip_probe.py's sweep by the rule above at 0.5 degrees a frame
# and HISTORY_MAX, i.e. the smallest worse-of-two-scenes MSE ratio of the clipped walk's temporal image against the unclipped walk's
# (profiles/history_clip/history_clip_probe.json).
HISTORY_CLIP_RADIUS = 1
HISTORY_CLIP_GAMMA = 0.5
# Renderer.denoise_history_variance defaults: the best of scripts/history_variance_probe.py's sweep by the same rule at 0.5 degrees a
# frame, i.e. the smallest worse-of-two-scenes ratio of its MSE to denoise_history()'s at the defaults above, first of equals in grid
# order (profiles/history_variance/history_variance_probe.json).  At these the ratio is 0.86 on scene 1 and
# 1.00 on scene 3: it does not pay on both yet, and denoise_history() stays the filter the documents recommend for the temporal image.
HISTORY_VARIANCE_RADIUS = 1
HISTORY_SIGMA_VARIANCE = 2.0
# Renderer.history_commit_filtered defaults: the best of scripts/history_feedback_probe.py's sweep by the same rule on the clipped walk at
# 0.5 degrees a frame, i.e. the smallest worse-of-two-scenes ratio R_T of the temporal image's MSE with filtered commits to its MSE with
# plain commits, first of equals in grid order (profiles/history_feedback/history_feedback_probe.json).  At these
# R_T is 0.97 on scene 1 and 0.93 on scene 3, but denoise_history() of that image is worse than after plain commits (1.09 / 1.09): it
# does not pay yet, and history_commit() stays the commit the documents recommend.
HISTORY_FEEDBACK_SIGMA_COLOR = 0.05
HISTORY_FEEDBACK = 1.0
# Renderer.render_coverage / resolve_edges defaults: the best of scripts/edge_resolve_probe.py --sweep, i.e. the smallest worst case over
# 4, 16 and 64 samples and scenes 1 and 3 of the whole-frame MSE of the resolved denoise() over plain denoise()'s, at 320 x 180 against
# 1024 samples, first of equals in grid order (profiles/edge_resolve/edge_resolve_probe.json).  At these the
# ratio is 0.85 to 0.87 at 4 samples, 0.88 to 0.90 at 16 and 0.92 to 0.94 at 64.  The 4 x 4 lattice is better at 4 samples alone (0.82 to
# 0.84 with the same radius, sigmas and prior) for about three times the render_coverage time.
COVERAGE_GRID = 2
EDGE_RADIUS = 1
EDGE_SIGMA_NORMAL = 0.1
EDGE_SIGMA_DEPTH = 0.1
EDGE_PRIOR = 32.0
# The filter guides' chain (Renderer.set_guide_mode, GUIDES_SPECULAR): the cap on specular bounces and the largest fuzz a metal may have
# to count as a mirror.  From the sweep of scripts/specular_guides_probe.py (profiles/specular_guides/specular_guides_probe.json; DESIGN.md
# section 4.11): the setting with the smallest worse-of-two-scenes MSE over the specular pixels at 16 samples.  No setting beat the
# first-hit guides on both scenes, which is why GUIDES_FIRST_HIT stays the mode a handle starts in.
GUIDE_MAX_BOUNCES = 1
GUIDE_MAX_FUZZ = 0.0
# Renderer.set_guide_lens: the lens points per side the wrapper turns on.  2 x 2 is the lattice the rule of
# DESIGN.md section 4.18 is stated for; 4 x 4 traces four times the rays.  A handle starts with the lattice off.
GUIDE_LENS_GRID = 2
# Renderer.set_edit_influence: the kappa the wrapper turns on.  From the sweep of scripts/edit_influence_probe.py
# (profiles/edit_influence/edit_influence_probe.json): the kappa with the smallest worst-of-four-walks whole-frame
# MSE ratio among those within 1.10 x the rays of kappa == 0.  No kappa of the sweep brought that ratio below 1 (0.25: 1.006), which is
# why a handle starts with kappa == 0, off.
EDIT_INFLUENCE_KAPPA = 0.25
# Renderer.upscale defaults: the factor, and the best of scripts/upscale_probe.py --sweep by the rule of DESIGN.md
# section 4.22, i.e. the smallest worse-of-two-scenes ratio of the MSE of the upscaled half-resolution frame to that of the full-resolution
# frame at the same number of rays, at 1 and 4 rays an output pixel, first of equals in grid order (profiles/upscale/upscale_probe.json).
# At these the ratio is 0.10 / 0.08 at 1 ray and 0.38 / 0.35 at 4 (scenes 1 / 3), but plain bilinear interpolation of the same denoised
# image is 8 to 21 % better still at factor 2 (at factor 4 the guided gather wins): it does not pay yet, and the call stays opt-in.
UPSCALE_FACTOR = 2
UPSCALE_SIGMA_NORMAL = 0.3
UPSCALE_SIGMA_ALBEDO = float("inf")
UPSCALE_SIGMA_DEPTH = float("inf")
UPSCALE_COVERAGE = 0
# Renderer.upscale_wide defaults: the best of scripts/upscale_wide_probe.py's sweep by the same rule over the same
# 24 settings (profiles/upscale_wide/upscale_wide_probe.json): the setting upscale() has.  At it the ratio to the
# full-resolution frame is 0.08 / 0.07 at 1 ray and 0.40 / 0.37 at 4 (scenes 1 / 3); against bilinear interpolation of the same denoised
# image it wins at 1 ray at factor 2 (0.91 / 0.94) and loses at 4 rays (1.14 / 1.29): it does not pay yet, and the call stays opt-in.
UPSCALE_WIDE_SIGMA_NORMAL = 0.3
UPSCALE_WIDE_SIGMA_ALBEDO = float("inf")
UPSCALE_WIDE_SIGMA_DEPTH = float("inf")
UPSCALE_WIDE_COVERAGE = 0


def _out(ctype, wanted=True):
    """(holder, argument) of an optional output parameter: a zeroed ctype and its address, or NULL when the caller does not want it --
    kernel_ms and the counts a call only knows after waiting (sync=False)."""
    holder = ctype(0)
    return holder, (ctypes.byref(holder) if wanted else None)


def _set_scene(fn, handle, scene, dt, *more):
    """rtiow_set_scene / rtiow_group_set_scene: build_scene()'s five tables in the handle's precision ('valid' may be absent); `more`:
    what the call takes behind them."""
    cr = np.ascontiguousarray(scene["center_radius"], dt)
    af = np.ascontiguousarray(scene["albedo_fuzz"], dt)
    ri = np.ascontiguousarray(scene["refraction_index"], dt)
    ty = np.ascontiguousarray(scene["type"], np.int32)
    va = np.ascontiguousarray(scene["valid"], np.int32) if scene.get("valid") is not None else None
    return fn(handle, len(ty), cr.ctypes.data, af.ctypes.data, ri.ctypes.data, ty.ctypes.data_as(_i32p), va.ctypes.data_as(_i32p) if va is not None else None,
              *more)


class Renderer:
    """One GPU's render state behind the C-ABI handle (include/rtiow.h)."""

    def __init__(self, device=0, precision=32, debug=False):
        """debug=True: the handle lives in the test build of the library (librtiow_hip_debug.so: the same kernels), whose hooks
        (include/rtiow_debug.h) the debug_* methods call; the product library exports none of them."""
        self._lib = load_hip_library(debug)
        self._debug = bool(debug)
        self.precision = precision
        self.dtype = _dtype(precision)
        self._borrowed = False
        self._h = ctypes.c_void_p()
        rc = self._lib.rtiow_create(int(device), int(precision), ctypes.byref(self._h))
        if rc:
            self._h = None
            raise RtiowError(rc, "rtiow_create(device=%d) failed -- is a GPU visible?" % device)
        self.width = self.height = 0

    @classmethod
    def _borrow(cls, lib, handle, precision, width, height):
        """A view of a handle somebody else owns (a member of a RendererGroup): close() leaves it alone."""
        r = cls.__new__(cls)
        r._lib, r.precision, r.dtype, r._borrowed = lib, precision, _dtype(precision), True
        r._debug = lib is _loaded.get("hip_debug")
        r._h = handle
        r.width, r.height = width, height
        return r

    def _check(self, rc):
        if rc:
            raise RtiowError(rc, self._lib.rtiow_last_error_string(self._h).decode(errors="replace"))

    def close(self):
        if getattr(self, "_h", None):
            if not self._borrowed:
                self._lib.rtiow_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_stream(self, hip_stream):
        self._check(self._lib.rtiow_set_stream(self._h, ctypes.c_void_p(int(hip_stream))))

    def _plane(self, *channels, dtype=None):
        """An uninitialised host array [local_rows, W, *channels] (the handle's precision unless dtype says otherwise) for a read to fill."""
        return np.empty((self.local_rows, self.width) + channels, dtype or self.dtype)

    def _device_ptr(self, fn):
        """(device address, bytes) from one of the *_device_ptr calls."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t(0)
        self._check(fn(self._h, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def set_scene(self, scene):
        self._check(_set_scene(self._lib.rtiow_set_scene, self._h, scene, self.dtype))

    def edit_scene(self, scene):
        """set_scene() that keeps the history base: the same tables with the same number of slots and the
        same 'valid' pattern, spheres moved, resized or given another material.  With a base, the updates and the plan that follow carry
        the history of a moved sphere along with it until the next commit.  The loop of an edited frame: edit_scene, set_camera if it
        moved, init_rng, history_plan, accumulate_budget ..., history_update_clipped, history_commit."""
        self._check(_set_scene(self._lib.rtiow_edit_scene, self._h, scene, self.dtype))

    def edit_scene_mapped(self, scene, origin):
        """edit_scene() for a scene of another shape: spheres added and removed, slots reordered, any 'valid'.
        origin[i] is the slot of the scene the renderer holds now that slot i of `scene` continues, or -1 for a new sphere (one entry per
        slot of `scene`; those of dropped slots are not read); a sphere of the current scene that no slot continues is removed.  A
        continued sphere carries its history as under edit_scene(), an added one carries none, and the pixels a removed one uncovers fail
        the gather's depth test, so accumulate_budget() samples them."""
        origin = np.ascontiguousarray(origin, np.int32).reshape(-1)
        if origin.size != len(scene["type"]):
            raise ValueError("origin needs one entry per slot of the scene")
        self._check(_set_scene(self._lib.rtiow_edit_scene_mapped, self._h, scene, self.dtype, origin.ctypes.data_as(_i32p)))

    def scene_origin(self):
        """from_snapshot [kept spheres] int32 while an edit is in effect: per kept sphere of the current scene, the number of the sphere it
        continues among the kept spheres of the scene the base was committed under, or -1 for one added since."""
        st = Stats()
        self._check(self._lib.rtiow_get_stats(self._h, ctypes.byref(st)))
        out = np.empty(st.num_spheres, np.int32)
        self._check(self._lib.rtiow_read_scene_origin(self._h, out.ctypes.data_as(_i32p), out.size))
        return out

    def set_camera(self, cam):
        want = CameraF64 if self.precision == 64 else CameraF32
        if not isinstance(cam, want):
            raise TypeError("camera precision does not match the renderer")
        self._check(self._lib.rtiow_set_camera(self._h, ctypes.addressof(cam)))
        self.width, self.height = cam.img_width, cam.img_height

    def set_shard(self, rank, nranks, strip_rows=8):
        self._check(self._lib.rtiow_set_shard(self._h, rank, nranks, strip_rows))

    def set_scene_source(self, source):
        self._check(self._lib.rtiow_set_scene_source(self._h, source))

    def debug_hit_world(self, rays):
        """hit_world alone on rays [n, 6] = {origin, direction}: (t [n], sphere index [n])."""
        self._need_debug()
        dt = _dtype(self.precision)
        rays = np.ascontiguousarray(rays, dt)
        n = rays.shape[0]
        t = np.zeros(n, dt); idx = np.zeros(n, np.int32)
        self._check(self._lib.rtiow_debug_hit_world(self._h, n, rays.ctypes.data, t.ctypes.data, idx.ctypes.data_as(_i32p)))
        return t, idx

    def debug_hit_world_large(self, rays):
        """debug_hit_world() through the device grid of render_large(): (t [n], sphere index [n], cells [n]) -- cells: how many cells the
        ray's walk read, or -1 when its wave took the exact loop."""
        self._need_debug()
        dt = _dtype(self.precision)
        rays = np.ascontiguousarray(rays, dt)
        n = rays.shape[0]
        t = np.zeros(n, dt); idx = np.zeros(n, np.int32); cells = np.zeros(n, np.int32)
        self._check(self._lib.rtiow_debug_hit_world_large(self._h, n, rays.ctypes.data, t.ctypes.data, idx.ctypes.data_as(_i32p), cells.ctypes.data_as(_i32p)))
        return t, idx, cells

    def debug_hit_world_volume(self, rays):
        """debug_hit_world() through the volume grid of render_volume(): (t [n], sphere index [n], cells [n]) -- cells: how many cells the
        ray's walk read, or -1 when its wave took the exact loop."""
        self._need_debug()
        dt = _dtype(self.precision)
        rays = np.ascontiguousarray(rays, dt)
        n = rays.shape[0]
        t = np.zeros(n, dt); idx = np.zeros(n, np.int32); cells = np.zeros(n, np.int32)
        self._check(self._lib.rtiow_debug_hit_world_volume(self._h, n, rays.ctypes.data, t.ctypes.data, idx.ctypes.data_as(_i32p), cells.ctypes.data_as(_i32p)))
        return t, idx, cells

    def debug_scatter(self, form, O, D, closest, hit, atten, sky_uy, depth, states):
        """The scatter step alone, one call per lane (calls 64 w ... 64 w + 63 share wave w), from caller-supplied (closest, hit).
        form 0: shade_step; 1: the bounded shade_step until it stops retrying; 2 (fp64): shade_front, merged_rounds, shade_back.
        A dict of status [n] (1: the path ended), col / O / D / atten [n, 3], depth, trips, flags [n], states [n, 6] and
        rounds_per_trip (the build's bound of the rejection loop)."""
        self._need_debug()
        dt = _dtype(self.precision)
        n = len(hit)
        real = np.zeros((n, 11), dt)
        real[:, 0:3] = O; real[:, 3:6] = D; real[:, 6] = closest; real[:, 7:10] = atten; real[:, 10] = sky_uy
        ints = np.ascontiguousarray(np.column_stack([hit, depth]), np.int32)
        st = np.ascontiguousarray(states, np.uint32)
        assert st.shape == (n, 6)
        out = np.zeros((n, 12), dt); oi = np.zeros((n, 4), np.int32); os_ = np.zeros((n, 6), np.uint32)
        rounds = ctypes.c_int(0)
        self._check(self._lib.rtiow_debug_scatter(self._h, form, n, real.ctypes.data, ints.ctypes.data_as(_i32p), st.ctypes.data_as(_u32p),
                                                  out.ctypes.data, oi.ctypes.data_as(_i32p), os_.ctypes.data_as(_u32p), ctypes.byref(rounds)))
        return {"status": oi[:, 0].copy(), "col": out[:, 0:3].copy(), "O": out[:, 3:6].copy(), "D": out[:, 6:9].copy(), "atten": out[:, 9:12].copy(),
                "depth": oi[:, 1].copy(), "trips": oi[:, 2].copy(), "flags": oi[:, 3].copy(), "states": os_, "rounds_per_trip": rounds.value}

    def set_schedule(self, schedule, waves_per_simd=0):
        self._check(self._lib.rtiow_set_schedule(self._h, schedule, waves_per_simd))

    @property
    def local_rows(self):
        n = ctypes.c_int(0)
        self._check(self._lib.rtiow_local_rows(self._h, ctypes.byref(n)))
        return n.value

    def local_row_map(self):
        rows = np.zeros(self.local_rows, np.int32)
        if len(rows):
            self._check(self._lib.rtiow_local_row_map(self._h, rows.ctypes.data_as(_i32p)))
        return rows

    def init_rng(self, seed=1227):
        self._check(self._lib.rtiow_init_rng(self._h, ctypes.c_uint64(seed)))

    def render(self, threads=8, sync=True):
        """render<<<>>> + sync; returns the HIP-event kernel time in ms (None when sync=False)."""
        ms, ms_out = _out(ctypes.c_float, sync)
        self._check(self._lib.rtiow_render(self._h, int(threads), ms_out))
        return ms.value if sync else None

    def render_large(self, sync=True):
        """render() through a uniform grid walked in device memory, for scenes whose tables outgrow a compute
        unit's LDS: the same framebuffer, bit for bit.  Raises RtiowError (RTIOW_E_BADARG) when the grid does not suit the scene -- use
        render() then.  Returns the HIP-event kernel time in ms (None when sync=False)."""
        ms, ms_out = _out(ctypes.c_float, sync)
        self._check(self._lib.rtiow_render_large(self._h, ms_out))
        return ms.value if sync else None

    def large_grid(self):
        """The device grid render_large() uses for the current scene: a dict of usable, nx, nz, cell, rfar, registered, direct,
        index_entries, longest_list and blob_bytes (all 0 when the grid does not suit the scene)."""
        info = LargeGridInfo()
        self._check(self._lib.rtiow_read_large_grid(self._h, ctypes.byref(info)))
        return {name: getattr(info, name) for name, _ in LargeGridInfo._fields_ if name != "reserved"}

    def render_volume(self, sync=True):
        """render() through a three-axis uniform grid walked in device memory, for scenes that fill a volume
        (a particle cloud, a stack of layers), where render_large()'s grid over x and z holds a whole column in every cell: the same
        framebuffer, bit for bit.  Raises RtiowError (RTIOW_E_BADARG) when the grid does not suit the scene -- use render() then.
        Returns the HIP-event kernel time in ms (None when sync=False)."""
        ms, ms_out = _out(ctypes.c_float, sync)
        self._check(self._lib.rtiow_render_volume(self._h, ms_out))
        return ms.value if sync else None

    def volume_grid(self):
        """The volume grid render_volume() uses for the current scene: a dict of usable, nx, ny, nz, cell, rfar, registered, direct,
        index_entries, occupied_cells, longest_list and blob_bytes (all 0 when the grid does not suit the scene)."""
        info = VolumeGridInfo()
        self._check(self._lib.rtiow_read_volume_grid(self._h, ctypes.byref(info)))
        return {name: getattr(info, name) for name, _ in VolumeGridInfo._fields_ if name != "reserved"}

    # The preview chain on large scenes: each the twin of the method it is named after, with the scene read
    # through the device grid of render_large().  Same buffers, state, refusals and bits; the two are interchangeable at every point of a
    # session.  RtiowError (RTIOW_E_BADARG) when the grid does not suit the scene -- use the twin then.  The calls remember nothing: a
    # filter that finds the guides or the layers stale renders them through the handle's scene source, so call these after each change
    # of camera or scene.
    def accumulate_large(self, samples, sync=True):
        """accumulate() through the device grid.  Returns the HIP-event kernel time in ms (None when sync=False)."""
        ms, ms_out = _out(ctypes.c_float, sync)
        self._check(self._lib.rtiow_accumulate_large(self._h, int(samples), ms_out))
        return ms.value if sync else None

    def accumulate_adaptive_large(self, samples, rel_error, min_samples=0, max_samples=2 ** 31 - 1, sync=True):
        """accumulate_adaptive() through the device grid.  Returns (kernel ms or None when sync=False, active pixels)."""
        active = ctypes.c_int(0)
        ms, ms_out = _out(ctypes.c_float, sync)
        self._check(self._lib.rtiow_accumulate_adaptive_large(self._h, int(samples), int(min_samples), float(rel_error), int(max_samples),
                                                              ms_out, ctypes.byref(active)))
        return (ms.value if sync else None), active.value

    def accumulate_budget_large(self, samples=BUDGET_CHUNK, target=BUDGET_TARGET, min_samples=BUDGET_MIN_SAMPLES, max_samples=2 ** 31 - 1, sync=True):
        """accumulate_budget() through the device grid.  Returns (kernel ms or None when sync=False, active pixels)."""
        active = ctypes.c_int(0)
        ms, ms_out = _out(ctypes.c_float, sync)
        self._check(self._lib.rtiow_accumulate_budget_large(self._h, int(samples), int(min_samples), float(target), int(max_samples),
                                                            ms_out, ctypes.byref(active)))
        return (ms.value if sync else None), active.value

    def render_guides_large(self, sync=True):
        """render_guides() through the device grid: the first-hit guides, the lens guides or the specular chain, the motion plane and the
        edit influence, as render_guides() renders them.  Returns the kernel ms (None when sync=False)."""
        ms, ms_out = _out(ctypes.c_float, sync)
        self._check(self._lib.rtiow_render_guides_large(self._h, ms_out))
        return ms.value if sync else None

    def render_coverage_large(self, subsamples_per_side=COVERAGE_GRID, sync=True):
        """render_coverage() through the device grid.  Returns the kernel ms (None when sync=False)."""
        ms, ms_out = _out(ctypes.c_float, sync)
        self._check(self._lib.rtiow_render_coverage_large(self._h, int(subsamples_per_side), ms_out))
        self._coverage_grid = int(subsamples_per_side)
        return ms.value if sync else None

    # A session on a volume scene: each the twin of the method it is named after, with the scene read through
    # the volume grid of render_volume().  Same buffers, state, refusals and bits; a _volume method, its twin and its _large twin are
    # interchangeable at every point of a session.  RtiowError (RTIOW_E_BADARG) when the grid does not suit the scene -- use the twin
    # then.  The calls remember nothing: a filter that finds the guides or the layers stale renders them through the handle's scene
    # source, so call these after each change of camera or scene.
    def accumulate_volume(self, samples, sync=True):
        """accumulate() through the volume grid.  Returns the HIP-event kernel time in ms (None when sync=False)."""
        ms, ms_out = _out(ctypes.c_float, sync)
        self._check(self._lib.rtiow_accumulate_volume(self._h, int(samples), ms_out))
        return ms.value if sync else None

    def accumulate_adaptive_volume(self, samples, rel_error, min_samples=0, max_samples=2 ** 31 - 1, sync=True):
        """accumulate_adaptive() through the volume grid.  Returns (kernel ms or None when sync=False, active pixels)."""
        active = ctypes.c_int(0)
        ms, ms_out = _out(ctypes.c_float, sync)
        self._check(self._lib.rtiow_accumulate_adaptive_volume(self._h, int(samples), int(min_samples), float(rel_error), int(max_samples),
                                                               ms_out, ctypes.byref(active)))
        return (ms.value if sync else None), active.value

    def accumulate_budget_volume(self, samples=BUDGET_CHUNK, target=BUDGET_TARGET, min_samples=BUDGET_MIN_SAMPLES, max_samples=2 ** 31 - 1, sync=True):
        """accumulate_budget() through the volume grid.  Returns (kernel ms or None when sync=False, active pixels)."""
        active = ctypes.c_int(0)
        ms, ms_out = _out(ctypes.c_float, sync)
        self._check(self._lib.rtiow_accumulate_budget_volume(self._h, int(samples), int(min_samples), float(target), int(max_samples),
                                                             ms_out, ctypes.byref(active)))
        return (ms.value if sync else None), active.value

    def render_guides_volume(self, sync=True):
        """render_guides() through the volume grid: the first-hit guides, the lens guides or the specular chain, the motion plane and the
        edit influence, as render_guides() renders them.  Returns the kernel ms (None when sync=False)."""
        ms, ms_out = _out(ctypes.c_float, sync)
        self._check(self._lib.rtiow_render_guides_volume(self._h, ms_out))
        return ms.value if sync else None

    def render_coverage_volume(self, subsamples_per_side=COVERAGE_GRID, sync=True):
        """render_coverage() through the volume grid.  Returns the kernel ms (None when sync=False)."""
        ms, ms_out = _out(ctypes.c_float, sync)
        self._check(self._lib.rtiow_render_coverage_volume(self._h, int(subsamples_per_side), ms_out))
        self._coverage_grid = int(subsamples_per_side)
        return ms.value if sync else None

    def accumulate(self, samples, threads=0, sync=True):
        """Progressive rendering: add `samples` samples per pixel to the accumulation and write the preview to the framebuffer (bit for bit
        what render() gives with samples_per_pixel = accumulated_samples).  Returns the HIP-event kernel time in ms (None when sync=False)."""
        ms, ms_out = _out(ctypes.c_float, sync)
        self._check(self._lib.rtiow_accumulate(self._h, int(samples), int(threads), ms_out))
        return ms.value if sync else None

    def reset_accumulation(self):
        """The next accumulate() starts a new image from the RNG states of init_rng."""
        self._check(self._lib.rtiow_accumulate_reset(self._h))

    @property
    def accumulated_samples(self):
        n = ctypes.c_int(0)
        self._check(self._lib.rtiow_accumulated_samples(self._h, ctypes.byref(n)))
        return n.value

    def accumulate_adaptive(self, samples, rel_error, min_samples=0, max_samples=2 ** 31 - 1, sync=True):
        """Adaptive progressive rendering: `samples` more samples for every pixel that is still active -- its count below min_samples
        or its relative error (adaptive_state) above rel_error, and count + samples <= max_samples -- and the preview of every pixel in
        the framebuffer (bit for bit what render() gives that pixel with samples_per_pixel = its count).  Returns (kernel ms or None when
        sync=False, active pixels); 0 active pixels means converged.  The call blocks once to read the active count back."""
        active = ctypes.c_int(0)
        ms, ms_out = _out(ctypes.c_float, sync)
        self._check(self._lib.rtiow_accumulate_adaptive(self._h, int(samples), int(min_samples), float(rel_error), int(max_samples),
                                                        ms_out, ctypes.byref(active)))
        return (ms.value if sync else None), active.value

    def accumulate_with_variance(self, samples, sync=True):
        """Uniform sampling that keeps the second moment variance() and denoise_variance() need: an adaptive chunk in which every pixel
        is active (min_samples and max_samples at their largest, rel_error 0).  The preview is accumulate()'s bit for bit; the chunk costs
        a few per cent more than a plain one plus the select and finish passes and, like every adaptive
        chunk, is not ranked by cost.  Returns the kernel ms (None when sync=False)."""
        return self.accumulate_adaptive(samples, 0.0, min_samples=2 ** 31 - 1, max_samples=2 ** 31 - 1, sync=sync)[0]

    def adaptive_state(self):
        """(counts, rel_err): each pixel's sample count (int32) and relative standard error of its mean luminance (float32, +inf below
        two samples), local_rows x width."""
        shape = (self.local_rows, self.width)
        counts, err = np.zeros(shape, np.int32), np.zeros(shape, np.float32)
        self._check(self._lib.rtiow_read_adaptive_state(self._h, counts.ctypes.data_as(_i32p), err.ctypes.data_as(_f32p), counts.size))
        return counts, err

    def read_linear(self):
        """The linear (pre-gamma) mean colour of the accumulation, [local_rows, W, 3]: acc * ((T)1 / (T)n) per pixel, n its count."""
        out = self._plane(3)
        self._check(self._lib.rtiow_read_linear(self._h, out.ctypes.data if out.size else None, out.nbytes))
        return out

    def render_guides(self, sync=True):
        """First-hit guide buffers for the current camera, scene and shard; returns the kernel ms (None when sync=False)."""
        ms, ms_out = _out(ctypes.c_float, sync)
        self._check(self._lib.rtiow_render_guides(self._h, ms_out))
        return ms.value if sync else None

    def _read_fresh_guides(self, fn, *args):
        """fn(h, *args) for the two guide reads; RTIOW_E_STATE (stale or never rendered) renders the guides and reads again."""
        rc = fn(self._h, *args)
        if rc == -2:
            self.render_guides()
            rc = fn(self._h, *args)
        self._check(rc)

    def guides(self):
        """(normal [rows, W, 3], albedo [rows, W, 3], depth [rows, W]) of the first hit of each pixel's centre ray (zeros on a miss);
        renders them first when they are stale (after set_scene, set_camera or set_shard)."""
        normal, albedo, depth = self._plane(3), self._plane(3), self._plane()
        self._read_fresh_guides(self._lib.rtiow_read_guides, normal.ctypes.data, albedo.ctypes.data, depth.ctypes.data, depth.size)
        return normal, albedo, depth

    def set_guide_mode(self, mode, max_bounces=GUIDE_MAX_BOUNCES, max_fuzz=GUIDE_MAX_FUZZ):
        """What denoise(), denoise_variance() and denoise_history() steer by.  GUIDES_FIRST_HIT (default): the
        first-hit guides.  GUIDES_SPECULAR: guides that follow each centre ray through glass and through metals with fuzz <= max_fuzz
        (float("inf"): every metal) to the first other surface, at most max_bounces (1..16) times.  The history calls keep the first-hit
        guides.  A change makes the guides and the denoised image stale; the knob survives set_scene, set_camera and set_shard."""
        self._check(self._lib.rtiow_set_guide_mode(self._h, int(mode), int(max_bounces), float(max_fuzz)))

    def set_guide_lens(self, samples_per_side=GUIDE_LENS_GRID):
        """Filter guides as the aperture sees them: the mean of the guide mode's values over a fixed
        samples_per_side x samples_per_side lattice of points on the camera's defocus disk (2 or 4; 0 turns it off, which is how a handle
        starts).  Inert with a pinhole camera (defocus_angle <= 0).  The first-hit guides, the history and the coverage layers are
        untouched.  A change makes the guides and the denoised image stale; the knob survives set_scene, set_camera and set_shard."""
        self._check(self._lib.rtiow_set_guide_lens(self._h, int(samples_per_side)))

    def filter_guides(self):
        """(normal [rows, W, 3], albedo [rows, W, 3], depth [rows, W], bounces [rows, W] int32) of the guides the filters read: guides()
        and zeros in GUIDES_FIRST_HIT mode, the end of each pixel's specular chain in GUIDES_SPECULAR mode; with set_guide_lens() in
        effect their mean over the lens lattice and the largest bounce count.  Renders stale guides first."""
        normal, albedo, depth, bounces = self._plane(3), self._plane(3), self._plane(), self._plane(dtype=np.int32)
        self._read_fresh_guides(self._lib.rtiow_read_filter_guides, normal.ctypes.data, albedo.ctypes.data, depth.ctypes.data,
                                bounces.ctypes.data_as(_i32p), depth.size)
        return normal, albedo, depth, bounces

    def denoise(self, levels=DENOISE_LEVELS, sigma_color=DENOISE_SIGMA_COLOR, sigma_normal=DENOISE_SIGMA_NORMAL,
                sigma_albedo=DENOISE_SIGMA_ALBEDO, sigma_depth=DENOISE_SIGMA_DEPTH, sync=True):
        """Edge-avoiding a-trous filter of the accumulation: returns the gamma-encoded denoised image
        [rows, W, 3] (sync=True), or None after enqueueing the work (sync=False; read_denoised() / denoised_device_ptr() later).
        The framebuffer and the accumulation are untouched.  sigma = float("inf") turns a term off."""
        _, ms_out = _out(ctypes.c_float, sync)
        self._check(self._lib.rtiow_denoise(self._h, int(levels), float(sigma_color), float(sigma_normal), float(sigma_albedo),
                                            float(sigma_depth), ms_out))
        return self.read_denoised() if sync else None

    def variance(self):
        """The estimated variance of each pixel's mean luminance, [local_rows, W] (0 below two samples), from the second moment an
        adaptive accumulation keeps: adaptive_state()'s rel_err is sqrt(variance) / (mean luminance + 1e-3)."""
        out = self._plane()
        self._check(self._lib.rtiow_read_variance(self._h, out.ctypes.data if out.size else None, out.size))
        return out

    def denoise_variance(self, levels=DENOISE_LEVELS, sigma_variance=DENOISE_SIGMA_VARIANCE, sigma_normal=DENOISE_SIGMA_NORMAL,
                         sigma_albedo=DENOISE_SIGMA_ALBEDO, sigma_depth=DENOISE_SIGMA_DEPTH, sync=True):
        """Variance-guided a-trous filter of an adaptive accumulation: denoise() with the colour edge-stop
        of every pixel set by its measured variance(), sigma_variance standard deviations wide, so it follows the noise as samples
        accumulate.  Needs accumulate_adaptive() or accumulate_with_variance() chunks.  Returns and stores its image like denoise()."""
        _, ms_out = _out(ctypes.c_float, sync)
        self._check(self._lib.rtiow_denoise_variance(self._h, int(levels), float(sigma_variance), float(sigma_normal), float(sigma_albedo),
                                                     float(sigma_depth), ms_out))
        return self.read_denoised() if sync else None

    def history_reset(self):
        """Forget the temporal history: the next history_update() finds no base."""
        self._check(self._lib.rtiow_history_reset(self._h))

    def history_update(self, depth_tol=HISTORY_DEPTH_TOL, normal_cos=HISTORY_NORMAL_COS, max_history=HISTORY_MAX, sync=True):
        """Temporal reprojection: combine the history committed from an earlier camera with the whole
        current accumulation into the temporal image history() reads.  A base sample is carried where it reprojects into the frame
        onto the same surface: relative depth within depth_tol, normals at least normal_cos apart in cosine; a pixel's history
        length is capped at max_history samples (float("inf"): no cap).  Call it after any chunk: nothing is counted twice.
        Returns the number of pixels that carried history (None when sync=False)."""
        (_, ms_out), (n, n_out) = _out(ctypes.c_float, sync), _out(ctypes.c_uint64, sync)
        self._check(self._lib.rtiow_history_update(self._h, float(depth_tol), float(normal_cos), float(max_history), ms_out, n_out))
        return int(n.value) if sync else None

    def history_update_clipped(self, clip_radius=HISTORY_CLIP_RADIUS, clip_gamma=HISTORY_CLIP_GAMMA, depth_tol=HISTORY_DEPTH_TOL,
                               normal_cos=HISTORY_NORMAL_COS, max_history=HISTORY_MAX, sync=True):
        """history_update() with the gathered history colour clamped, per channel, to mean +- clip_gamma standard deviations of the
        current accumulation over the (2 clip_radius + 1)^2 pixels around each pixel: a history the
        current frame contradicts -- a reflection reprojected as if painted on its mirror -- is pulled to what the frame sees.  History
        lengths, and so history_plan(), are history_update()'s.  clip_radius 1..3; clip_gamma >= 0 (float("inf"): no clamp).
        Returns (pixels that carried history, those of them the clamp changed), or None when sync=False."""
        (_, ms_out), (n, n_out), (k, k_out) = _out(ctypes.c_float, sync), _out(ctypes.c_uint64, sync), _out(ctypes.c_uint64, sync)
        self._check(self._lib.rtiow_history_update_clipped(self._h, float(depth_tol), float(normal_cos), float(max_history), int(clip_radius),
                                                           float(clip_gamma), ms_out, n_out, k_out))
        return (int(n.value), int(k.value)) if sync else None

    def history_plan(self, depth_tol=HISTORY_DEPTH_TOL, normal_cos=HISTORY_NORMAL_COS, max_history=HISTORY_MAX, sync=True):
        """The history length every pixel of the current camera will carry: history_update()'s m for the
        same three arguments, before any sample of the frame is traced.  It needs scene and camera only, is what accumulate_budget()
        samples by, and goes stale with the temporal image.  Returns the number of pixels with m > 0 (None when sync=False)."""
        (_, ms_out), (n, n_out) = _out(ctypes.c_float, sync), _out(ctypes.c_uint64, sync)
        self._check(self._lib.rtiow_history_plan(self._h, float(depth_tol), float(normal_cos), float(max_history), ms_out, n_out))
        return int(n.value) if sync else None

    def history_plan_lengths(self):
        """The plan of history_plan(), [H, W]: each pixel's history length m in samples."""
        length = self._plane()
        self._check(self._lib.rtiow_read_history_plan(self._h, length.ctypes.data, length.size))
        return length

    def accumulate_budget(self, samples=BUDGET_CHUNK, target=BUDGET_TARGET, min_samples=BUDGET_MIN_SAMPLES, max_samples=2 ** 31 - 1, sync=True):
        """accumulate_adaptive() with the rule of INTEGRATION.md section 13: `samples` more samples for every pixel whose count is below
        min_samples or whose count plus planned history length (history_plan) is below target, and count + samples <= max_samples.
        The loop of a moving camera: set_camera, init_rng, history_plan, accumulate_budget until it returns 0 active pixels,
        history_update with the plan's arguments, history_commit.  Alternates freely with accumulate_adaptive().  Returns (kernel ms or
        None when sync=False, active pixels)."""
        active = ctypes.c_int(0)
        ms, ms_out = _out(ctypes.c_float, sync)
        self._check(self._lib.rtiow_accumulate_budget(self._h, int(samples), int(min_samples), float(target), int(max_samples),
                                                      ms_out, ctypes.byref(active)))
        return (ms.value if sync else None), active.value

    def history_commit(self):
        """Make the temporal image, the current guides and the current camera the base of later updates (buffers change owners, nothing
        is copied).  Then move the camera: the temporal image and the guides are stale after the call."""
        self._check(self._lib.rtiow_history_commit(self._h))

    def history_commit_filtered(self, sigma_color=HISTORY_FEEDBACK_SIGMA_COLOR, sigma_normal=DENOISE_SIGMA_NORMAL, sigma_albedo=DENOISE_SIGMA_ALBEDO,
                                sigma_depth=DENOISE_SIGMA_DEPTH, feedback=HISTORY_FEEDBACK, sync=True):
        """history_commit() of a filtered temporal image: one level of denoise_history()'s filter at step 1,
        over the pixels that hold samples, replaces the colour before it becomes the base, blended with the unfiltered colour by
        `feedback` in (0, 1] (1: the filtered colour alone); the lengths are kept, so history_plan() predicts as before.  The filter
        steers by the filter guides of the current guide mode; the base keeps the first-hit guides.  Returns the kernel time in ms
        (None when sync=False)."""
        ms, ms_out = _out(ctypes.c_float, sync)
        self._check(self._lib.rtiow_history_commit_filtered(self._h, float(sigma_color), float(sigma_normal), float(sigma_albedo), float(sigma_depth),
                                                            float(feedback), ms_out))
        return ms.value if sync else None

    def history_base(self):
        """(rgb [H, W, 3] linear, length [H, W]) of the base the last history_commit() or history_commit_filtered() left."""
        rgb, length = self._plane(3), self._plane()
        self._check(self._lib.rtiow_read_history_base(self._h, rgb.ctypes.data, length.ctypes.data, length.size))
        return rgb, length

    def scene_motion(self):
        """(prev_point [rows, W, 3], carry [rows, W] int32, ids [rows, W] int32) of the motion plane while an edit_scene() is in effect:
        the point of the scene the base was committed under that each pixel's first hit came from, whether that surface carries history
        (0: its material changed) and the sphere index (-1: the sky).  Renders stale guides, and the plane with them, first."""
        prev_point, carry, ids = self._plane(3), self._plane(dtype=np.int32), self._plane(dtype=np.int32)
        self._read_fresh_guides(self._lib.rtiow_read_scene_motion, prev_point.ctypes.data, carry.ctypes.data_as(_i32p), ids.ctypes.data_as(_i32p),
                                ids.size)
        return prev_point, carry, ids

    def set_edit_influence(self, kappa=EDIT_INFLUENCE_KAPPA):
        """Shorten the history where an edit_scene() changes the light: with kappa > 0 every pixel's history
        length is multiplied by 1 - min(1, kappa * s), s the share of the pixel's surroundings that the edited spheres occupy before and
        after the edit (edit_influence()); float("inf") drops the history wherever s > 0; 0 turns it off, which is how a handle starts.
        A change makes the motion plane, the guides, the plan, the temporal image and the denoised image stale; the knob survives
        set_scene, set_camera and set_shard."""
        self._check(self._lib.rtiow_set_edit_influence(self._h, float(kappa)))

    def edit_influence(self):
        """lambda [rows, W] of the influence plane while an edit_scene() is in effect and set_edit_influence() is on: how much of each
        pixel's history the updates and the plan drop (0: none, 1: all).  Renders stale guides, and the planes with them, first."""
        lam = self._plane()
        self._read_fresh_guides(self._lib.rtiow_read_edit_influence, lam.ctypes.data, lam.size)
        return lam

    def render_coverage(self, subsamples_per_side=COVERAGE_GRID, sync=True):
        """Sub-pixel coverage layers for the current camera, scene and shard: which first-hit spheres share
        each pixel, from subsamples_per_side^2 (2 or 4 a side) primary rays on a lattice inside it.  Returns the kernel ms (None when
        sync=False)."""
        ms, ms_out = _out(ctypes.c_float, sync)
        self._check(self._lib.rtiow_render_coverage(self._h, int(subsamples_per_side), ms_out))
        self._coverage_grid = int(subsamples_per_side)
        return ms.value if sync else None

    def coverage(self):
        """(ids [rows, W, 2] int32, counts [rows, W, 2] int32, normal [rows, W, 2, 3], depth [rows, W, 2]) of the two coverage layers of
        each pixel: sphere index (-1: the sky; -2: no second layer, the pixel is pure), sub-samples covered, their mean normal and hit
        distance.  Renders them first, at the subsamples_per_side of the last render_coverage() (COVERAGE_GRID before any), when they
        are stale (after set_scene, set_camera or set_shard)."""
        ids, counts, normal, depth = self._plane(2, dtype=np.int32), self._plane(2, dtype=np.int32), self._plane(2, 3), self._plane(2)
        args = (ids.ctypes.data_as(_i32p), counts.ctypes.data_as(_i32p), normal.ctypes.data, depth.ctypes.data, ids.size // 2)
        if self._coverage_is_stale():
            self.render_coverage(getattr(self, "_coverage_grid", COVERAGE_GRID))
        self._check(self._lib.rtiow_read_coverage(self._h, *args))
        return ids, counts, normal, depth

    def _coverage_is_stale(self):
        return self._lib.rtiow_read_coverage(self._h, None, None, None, None, self.local_rows * self.width) == -2

    def resolve_edges(self, radius=EDGE_RADIUS, sigma_normal=EDGE_SIGMA_NORMAL, sigma_depth=EDGE_SIGMA_DEPTH, prior=EDGE_PRIOR, sync=True):
        """Rebuild the silhouette pixels of the denoised image in place: every pixel that two first-hit
        spheres share (render_coverage) becomes the coverage-weighted sum of what the filter produced on the pure pixels of each of its
        layers within `radius` (1..3), weighted by first-hit normal and depth (float("inf") turns a term off), blended with its own
        filtered value by prior / (prior + the samples behind it) (float("inf"): the rebuilt colour alone).  Call it once after denoise(),
        denoise_variance(), denoise_history() or denoise_history_variance() and read the result with read_denoised(); before
        history_commit() when the filter read the temporal image.  Stale layers are rendered first, at the subsamples_per_side of the
        last render_coverage() (COVERAGE_GRID before any).  Returns the number of pixels rewritten (None when sync=False)."""
        if self._coverage_is_stale():
            self.render_coverage(getattr(self, "_coverage_grid", COVERAGE_GRID), sync=False)
        (_, ms_out), (n, n_out) = _out(ctypes.c_float, sync), _out(ctypes.c_uint64, sync)
        self._check(self._lib.rtiow_resolve_edges(self._h, int(radius), float(sigma_normal), float(sigma_depth), float(prior), ms_out, n_out))
        return int(n.value) if sync else None

    def upscale(self, factor=UPSCALE_FACTOR, source=UPSCALE_DENOISED, sigma_normal=UPSCALE_SIGMA_NORMAL, sigma_albedo=UPSCALE_SIGMA_ALBEDO,
                sigma_depth=UPSCALE_SIGMA_DEPTH, use_coverage=UPSCALE_COVERAGE, sync=True):
        """A preview `factor` (2..4) times as wide and as high as the traced frame: every output pixel traces
        one primary ray of its own and gathers the four traced pixels around it -- of the denoised image (UPSCALE_DENOISED, after any
        filter or resolve_edges()), the accumulation (UPSCALE_LINEAR) or the temporal image (UPSCALE_HISTORY) -- each weighed bilinearly,
        by first-hit normal, albedo and depth against what its ray hit (float("inf") turns a term off) and, with use_coverage, by the
        share of the tap that is the surface the output pixel sees (render_coverage).  Stale guides and layers are rendered first, the
        layers at the subsamples_per_side of the last render_coverage() (COVERAGE_GRID before any).  Read the image with read_upscaled();
        it stays current until the next set_scene, edit_scene, set_camera or set_shard.  Returns the number of output pixels the share
        decided (None when sync=False)."""
        if use_coverage and self._coverage_is_stale():
            self.render_coverage(getattr(self, "_coverage_grid", COVERAGE_GRID), sync=False)
        (_, ms_out), (n, n_out) = _out(ctypes.c_float, sync), _out(ctypes.c_uint64, sync)
        self._check(self._lib.rtiow_upscale(self._h, int(factor), int(source), float(sigma_normal), float(sigma_albedo), float(sigma_depth),
                                            int(use_coverage), ms_out, n_out))
        return int(n.value) if sync else None

    def upscale_wide(self, factor=UPSCALE_FACTOR, source=UPSCALE_DENOISED, sigma_normal=UPSCALE_WIDE_SIGMA_NORMAL, sigma_albedo=UPSCALE_WIDE_SIGMA_ALBEDO,
                     sigma_depth=UPSCALE_WIDE_SIGMA_DEPTH, use_coverage=UPSCALE_WIDE_COVERAGE, sync=True):
        """upscale() with a wider support: every output pixel gathers the 4 x 4 traced pixels around it under the
        cubic B-spline where upscale() gathers 2 x 2 bilinearly; the ray, the sources, the edge-stops, the share, the count returned and the
        image's life are upscale()'s.  With every sigma float("inf") and no share it is the unguided B-spline interpolation.  It writes the
        buffer upscale() writes: read_upscaled() serves whichever of the two ran last."""
        if use_coverage and self._coverage_is_stale():
            self.render_coverage(getattr(self, "_coverage_grid", COVERAGE_GRID), sync=False)
        (_, ms_out), (n, n_out) = _out(ctypes.c_float, sync), _out(ctypes.c_uint64, sync)
        self._check(self._lib.rtiow_upscale_wide(self._h, int(factor), int(source), float(sigma_normal), float(sigma_albedo), float(sigma_depth),
                                                 int(use_coverage), ms_out, n_out))
        return int(n.value) if sync else None

    # Guided upscaling on large scenes: the twins of upscale() and upscale_wide() with every output pixel's ray
    # traced through the device grid of render_large().  Same buffer, state, refusals and bits; RtiowError (RTIOW_E_BADARG) when the grid
    # does not suit the scene -- use the twin then.  Stale guides and layers are rendered through the grid as well.
    def upscale_large(self, factor=UPSCALE_FACTOR, source=UPSCALE_DENOISED, sigma_normal=UPSCALE_SIGMA_NORMAL, sigma_albedo=UPSCALE_SIGMA_ALBEDO,
                      sigma_depth=UPSCALE_SIGMA_DEPTH, use_coverage=UPSCALE_COVERAGE, sync=True):
        """upscale() through the device grid.  Returns the number of output pixels the share decided (None when sync=False)."""
        if use_coverage and self._coverage_is_stale():
            self.render_coverage_large(getattr(self, "_coverage_grid", COVERAGE_GRID), sync=False)
        (_, ms_out), (n, n_out) = _out(ctypes.c_float, sync), _out(ctypes.c_uint64, sync)
        self._check(self._lib.rtiow_upscale_large(self._h, int(factor), int(source), float(sigma_normal), float(sigma_albedo), float(sigma_depth),
                                                  int(use_coverage), ms_out, n_out))
        return int(n.value) if sync else None

    def upscale_wide_large(self, factor=UPSCALE_FACTOR, source=UPSCALE_DENOISED, sigma_normal=UPSCALE_WIDE_SIGMA_NORMAL, sigma_albedo=UPSCALE_WIDE_SIGMA_ALBEDO,
                           sigma_depth=UPSCALE_WIDE_SIGMA_DEPTH, use_coverage=UPSCALE_WIDE_COVERAGE, sync=True):
        """upscale_wide() through the device grid.  Returns the number of output pixels the share decided (None when sync=False)."""
        if use_coverage and self._coverage_is_stale():
            self.render_coverage_large(getattr(self, "_coverage_grid", COVERAGE_GRID), sync=False)
        (_, ms_out), (n, n_out) = _out(ctypes.c_float, sync), _out(ctypes.c_uint64, sync)
        self._check(self._lib.rtiow_upscale_wide_large(self._h, int(factor), int(source), float(sigma_normal), float(sigma_albedo), float(sigma_depth),
                                                       int(use_coverage), ms_out, n_out))
        return int(n.value) if sync else None

    # Guided upscaling on volume scenes: the twins of upscale() and upscale_wide() with every output pixel's ray
    # traced through the volume grid of render_volume().  Same buffer, state, refusals and bits; RtiowError (RTIOW_E_BADARG) when the grid
    # does not suit the scene -- use the twin then.  Stale guides and layers are rendered through the volume grid as well.
    def upscale_volume(self, factor=UPSCALE_FACTOR, source=UPSCALE_DENOISED, sigma_normal=UPSCALE_SIGMA_NORMAL, sigma_albedo=UPSCALE_SIGMA_ALBEDO,
                       sigma_depth=UPSCALE_SIGMA_DEPTH, use_coverage=UPSCALE_COVERAGE, sync=True):
        """upscale() through the volume grid.  Returns the number of output pixels the share decided (None when sync=False)."""
        if use_coverage and self._coverage_is_stale():
            self.render_coverage_volume(getattr(self, "_coverage_grid", COVERAGE_GRID), sync=False)
        (_, ms_out), (n, n_out) = _out(ctypes.c_float, sync), _out(ctypes.c_uint64, sync)
        self._check(self._lib.rtiow_upscale_volume(self._h, int(factor), int(source), float(sigma_normal), float(sigma_albedo), float(sigma_depth),
                                                   int(use_coverage), ms_out, n_out))
        return int(n.value) if sync else None

    def upscale_wide_volume(self, factor=UPSCALE_FACTOR, source=UPSCALE_DENOISED, sigma_normal=UPSCALE_WIDE_SIGMA_NORMAL, sigma_albedo=UPSCALE_WIDE_SIGMA_ALBEDO,
                            sigma_depth=UPSCALE_WIDE_SIGMA_DEPTH, use_coverage=UPSCALE_WIDE_COVERAGE, sync=True):
        """upscale_wide() through the volume grid.  Returns the number of output pixels the share decided (None when sync=False)."""
        if use_coverage and self._coverage_is_stale():
            self.render_coverage_volume(getattr(self, "_coverage_grid", COVERAGE_GRID), sync=False)
        (_, ms_out), (n, n_out) = _out(ctypes.c_float, sync), _out(ctypes.c_uint64, sync)
        self._check(self._lib.rtiow_upscale_wide_volume(self._h, int(factor), int(source), float(sigma_normal), float(sigma_albedo), float(sigma_depth),
                                                        int(use_coverage), ms_out, n_out))
        return int(n.value) if sync else None

    def read_upscaled(self):
        """The image of the last upscale(), upscale_wide() or _large / _volume twin of theirs, [factor * rows, factor * W, 3], gamma-encoded like the preview."""
        _, nbytes = self.upscaled_device_ptr()
        F = math.isqrt(nbytes // (self.local_rows * self.width * 3 * np.dtype(self.dtype).itemsize))     # the buffer holds F x F traced frames
        out = np.empty((F * self.local_rows, F * self.width, 3), self.dtype)
        self._check(self._lib.rtiow_read_upscaled(self._h, out.ctypes.data, out.nbytes))
        return out

    def upscaled_device_ptr(self):
        """(device address, bytes) of the last upscale() output."""
        return self._device_ptr(self._lib.rtiow_upscaled_device_ptr)

    def history(self):
        """(rgb [H, W, 3] linear, length [H, W]) of the temporal image: the blended colour and its history length in samples."""
        rgb, length = self._plane(3), self._plane()
        self._check(self._lib.rtiow_read_history(self._h, rgb.ctypes.data, length.ctypes.data, length.size))
        return rgb, length

    def history_device_ptr(self):
        """(device address, bytes) of the temporal image, H x W x 4 T: {C.rgb, M}."""
        return self._device_ptr(self._lib.rtiow_history_device_ptr)

    def denoise_history(self, levels=DENOISE_LEVELS, sigma_color=DENOISE_SIGMA_COLOR, sigma_normal=DENOISE_SIGMA_NORMAL,
                        sigma_albedo=DENOISE_SIGMA_ALBEDO, sigma_depth=DENOISE_SIGMA_DEPTH, sync=True):
        """denoise() of the temporal image instead of the accumulation: the same filter, level 0 reading history()'s colour.  Returns
        and stores its image like denoise()."""
        _, ms_out = _out(ctypes.c_float, sync)
        self._check(self._lib.rtiow_denoise_history(self._h, int(levels), float(sigma_color), float(sigma_normal), float(sigma_albedo),
                                                    float(sigma_depth), ms_out))
        return self.read_denoised() if sync else None

    def denoise_history_variance(self, levels=DENOISE_LEVELS, sigma_variance=HISTORY_SIGMA_VARIANCE, sigma_normal=DENOISE_SIGMA_NORMAL,
                                 sigma_albedo=DENOISE_SIGMA_ALBEDO, sigma_depth=DENOISE_SIGMA_DEPTH, variance_radius=HISTORY_VARIANCE_RADIUS, sync=True):
        """denoise_variance() of the temporal image: level 0 reads history()'s colour and history_variance(),
        i.e. the frame's measured variance() scaled by the update's blend weight n / length where the accumulation measured one, and
        the spread of the temporal image's luminance over the (2 variance_radius + 1)^2 pixels around the pixel elsewhere (plain
        chunks: everywhere).  Call it after history_update() or history_update_clipped() and before the next chunk.  variance_radius
        1..3.  Returns and stores its image like denoise()."""
        _, ms_out = _out(ctypes.c_float, sync)
        self._check(self._lib.rtiow_denoise_history_variance(self._h, int(levels), float(sigma_variance), float(sigma_normal), float(sigma_albedo),
                                                             float(sigma_depth), int(variance_radius), ms_out))
        return self.read_denoised() if sync else None

    def history_variance(self):
        """The variance plane [H, W] the last denoise_history_variance() filtered the temporal image by."""
        out = self._plane()
        self._check(self._lib.rtiow_read_history_variance(self._h, out.ctypes.data, out.size))
        return out

    def read_denoised(self):
        out = self._plane(3)
        self._check(self._lib.rtiow_read_denoised(self._h, out.ctypes.data, out.nbytes))
        return out

    def denoised_device_ptr(self):
        """(device address, bytes) of the last denoise() output."""
        return self._device_ptr(self._lib.rtiow_denoised_device_ptr)

    def count_segments(self, threads=8):
        """Untimed render that also counts path segments (hit_world calls)."""
        n = ctypes.c_uint64(0)
        self._check(self._lib.rtiow_count_segments(self._h, int(threads), ctypes.byref(n)))
        return n.value

    def bind_framebuffer(self, device_ptr, nbytes):
        self._check(self._lib.rtiow_bind_framebuffer(self._h, ctypes.c_void_p(int(device_ptr)), nbytes))

    def framebuffer_device_ptr(self):
        return self._device_ptr(self._lib.rtiow_framebuffer_device_ptr)

    def read_framebuffer(self):
        out = self._plane(3)
        if out.size:
            self._check(self._lib.rtiow_read_framebuffer(self._h, out.ctypes.data, out.nbytes))
        return out

    def read_levels(self):
        """(levels uint8 [rows, W, 3], nan_channels): the writer's quantisation done on the device (rtiow_read_levels)."""
        out = self._plane(3, dtype=np.uint8)
        nans = ctypes.c_uint64(0)
        self._check(self._lib.rtiow_read_levels(self._h, out.ctypes.data_as(_u8p), out.nbytes, ctypes.byref(nans)))
        return out, int(nans.value)

    def _need_debug(self):
        if not getattr(self, "_debug", False):
            raise RtiowError(-101, "test hook: librtiow_hip.so does not export it -- construct Renderer(device, precision, debug=True) (librtiow_hip_debug.so)")

    def synchronize(self):
        self._check(self._lib.rtiow_synchronize(self._h))

    def stats(self):
        st = Stats()
        self._check(self._lib.rtiow_get_stats(self._h, ctypes.byref(st)))
        return {name: getattr(st, name) for name, _ in Stats._fields_}

    # -- test hooks
    def debug_read_rng(self):
        self._need_debug()
        n = self.local_rows * self.width
        out = np.zeros((n, 6), np.uint32)
        self._check(self._lib.rtiow_debug_read_rng(self._h, out.ctypes.data_as(_u32p), out.size))
        return out

    def debug_read_costs(self):
        """(own, smoothed) prepass cost maps of the last ranking (the last sorted render's own, or the one whose order it reused), each local_rows x width."""
        self._need_debug()
        own = np.zeros((self.local_rows, self.width), np.uint32)
        smoothed = np.zeros_like(own)
        self._check(self._lib.rtiow_debug_read_costs(self._h, own.ctypes.data_as(_u32p), smoothed.ctypes.data_as(_u32p), own.size))
        return own, smoothed

    def debug_read_order(self):
        """What the hand-out order buffer holds now (rtiow_debug_read_order): (info, order, slot_of, keys).  info: a dict of
        ORDER_INFO_FIELDS; order: int32 [total_slots], slot -> (local row << 16 | column) or -1; slot_of: int32 [local_rows, W] for the
        ranking of a render, else None; keys: uint32 [local_rows, W] for a ranking, None for an adaptive list.  Raises RtiowError
        (RTIOW_E_STATE) when nothing has written an order."""
        self._need_debug()
        raw = np.zeros(12, np.int32)
        self._check(self._lib.rtiow_debug_read_order(self._h, raw.ctypes.data_as(_i32p), None, 0, None, None, 0))
        info = dict(zip(ORDER_INFO_FIELDS, (int(v) for v in raw)))
        shape = (info["local_rows"], info["W"])
        order = np.zeros(max(info["total_slots"], 1), np.int32)
        slot_of = np.zeros(shape, np.int32) if info["kind"] == ORDER_RENDER else None
        keys = np.zeros(shape, np.uint32) if info["kind"] in (ORDER_RENDER, ORDER_ACCUMULATE) else None
        self._check(self._lib.rtiow_debug_read_order(self._h, raw.ctypes.data_as(_i32p), order.ctypes.data_as(_i32p), order.size,
                                                     slot_of.ctypes.data_as(_i32p) if slot_of is not None else None,
                                                     keys.ctypes.data_as(_u32p) if keys is not None else None, shape[0] * shape[1]))
        return info, order[:info["total_slots"]], slot_of, keys

    def debug_read_chunk_costs(self):
        """uint32 [local_rows, W]: the path segments each pixel ran in the last accumulate() chunk (the next chunk's ranking smooths them)."""
        self._need_debug()
        out = np.zeros((self.local_rows, self.width), np.uint32)
        self._check(self._lib.rtiow_debug_read_chunk_costs(self._h, out.ctypes.data_as(_u32p), out.size))
        return out

    def debug_poison_staged(self):
        """Fill the staging buffer of the sorted schedule's staged stores with 0xff bytes (NaN in both precisions), on the handle's stream."""
        self._need_debug()
        self._check(self._lib.rtiow_debug_poison_staged(self._h))

    def debug_timeline(self, threads=0):
        self._need_debug()
        out = np.zeros((16384, 8), np.uint64)
        n = ctypes.c_int(0)
        self._check(self._lib.rtiow_debug_timeline(self._h, int(threads), out.ctypes.data_as(_u64p), out.size, ctypes.byref(n)))
        return out[: n.value]

    def debug_pixel_times(self, threads=0):
        """uint32 [rows, W, 4]: per pixel {taken, finished (100 MHz ticks), segments, wave} in the last launch that rendered it."""
        self._need_debug()
        out = np.zeros((self.local_rows, self.width, 4), np.uint32)
        self._check(self._lib.rtiow_debug_pixel_times(self._h, int(threads), out.ctypes.data_as(_u32p), out.size))
        return out

    def debug_ops(self, op, a, b=None, c=None):
        self._need_debug()
        a = np.ascontiguousarray(a, self.dtype)
        b = np.ascontiguousarray(b if b is not None else a, self.dtype)
        c = np.ascontiguousarray(c if c is not None else a, self.dtype)
        out = np.empty_like(a)
        self._check(self._lib.rtiow_debug_ops(self._h, op, a.size, a.ctypes.data, b.ctypes.data, c.ctypes.data, out.ctypes.data))
        return out


def debug_large_grid_plan(center_radius, centre=None, tables=False):
    """The device grid's plan (render_large) for spheres [n, 4] = {cx, cy, cz, r} around `centre` (default: the library's own recentring
    point, the centroid of the finite spheres with r < 100 rounded to fp32), on the host: no GPU needed.  A dict of usable, nx, nz,
    registered, direct, index_entries, longest_list, x0, z0, cell, ylo, yhi, rfar, eps, cmax; tables=True adds cells [nz, nx, 2]
    ({first, count}), indices, direct_list and halfwidth."""
    lib = load_hip_library(debug=True)
    cr = np.ascontiguousarray(center_radius, np.float64).reshape(-1, 4)
    n = len(cr)
    if centre is None:
        keep = (cr[:, 3] < 100.0) & np.isfinite(cr[:, :3]).all(axis=1)
        centre = cr[keep, :3].mean(axis=0).astype(np.float32) if keep.any() else np.zeros(3)
    centre = np.ascontiguousarray(centre, np.float64)
    dims, params = (ctypes.c_int32 * 6)(), (ctypes.c_double * 8)()
    args = (n, cr.ctypes.data_as(_f64p), centre.ctypes.data_as(_f64p), dims, params)
    rc = lib.rtiow_debug_large_grid_plan(*args, None, 0, None, 0, None, 0, None)
    if rc < 0:
        raise RtiowError(rc, "rtiow_debug_large_grid_plan")
    out = dict(zip(("nx", "nz", "registered", "direct", "index_entries", "longest_list"), dims), usable=bool(rc))
    out.update(zip(("x0", "z0", "cell", "ylo", "yhi", "rfar", "eps", "cmax"), params))
    if tables and out["nx"] > 0:
        cells = np.zeros((out["nz"], out["nx"], 2), np.uint32); indices = np.zeros(max(1, out["index_entries"]), np.uint32)
        direct = np.zeros(max(1, out["direct"]), np.int32); half = np.zeros(n, np.float64)
        rc = lib.rtiow_debug_large_grid_plan(*args, cells.ctypes.data_as(_u32p), cells.size, indices.ctypes.data_as(_u32p), indices.size,
                                             direct.ctypes.data_as(_i32p), direct.size, half.ctypes.data_as(_f64p))
        if rc < 0:
            raise RtiowError(rc, "rtiow_debug_large_grid_plan")
        out.update(cells=cells, indices=indices[:out["index_entries"]], direct_list=direct[:out["direct"]], halfwidth=half)
    return out


def debug_volume_grid_plan(center_radius, centre=None, tables=False, max_cells=0):
    """The volume grid's plan (render_volume) for spheres [n, 4] = {cx, cy, cz, r} around `centre` (default: the library's own recentring
    point, the centroid of the finite spheres with r < 100 rounded to fp32), on the host: no GPU needed.  max_cells = 0: the library's
    cap on nx ny nz.  A dict of usable, nx, ny, nz, registered, direct, index_entries, longest_list, occupied_cells, x0, y0, z0, cell,
    rfar, eps, cmax; tables=True adds cells [ny, nz, nx, 2] ({first, count}), indices, direct_list and halfwidth."""
    lib = load_hip_library(debug=True)
    cr = np.ascontiguousarray(center_radius, np.float64).reshape(-1, 4)
    n = len(cr)
    if centre is None:
        keep = (cr[:, 3] < 100.0) & np.isfinite(cr[:, :3]).all(axis=1)
        centre = cr[keep, :3].mean(axis=0).astype(np.float32) if keep.any() else np.zeros(3)
    centre = np.ascontiguousarray(centre, np.float64)
    dims, params = (ctypes.c_int32 * 8)(), (ctypes.c_double * 8)()
    args = (n, cr.ctypes.data_as(_f64p), centre.ctypes.data_as(_f64p), int(max_cells), dims, params)
    rc = lib.rtiow_debug_volume_grid_plan(*args, None, 0, None, 0, None, 0, None)
    if rc < 0:
        raise RtiowError(rc, "rtiow_debug_volume_grid_plan")
    out = dict(zip(("nx", "ny", "nz", "registered", "direct", "index_entries", "longest_list", "occupied_cells"), dims), usable=bool(rc))
    out.update(zip(("x0", "y0", "z0", "cell", "rfar", "eps", "cmax"), params))
    if tables and out["nx"] > 0:
        cells = np.zeros((out["ny"], out["nz"], out["nx"], 2), np.uint32); indices = np.zeros(max(1, out["index_entries"]), np.uint32)
        direct = np.zeros(max(1, out["direct"]), np.int32); half = np.zeros(n, np.float64)
        rc = lib.rtiow_debug_volume_grid_plan(*args, cells.ctypes.data_as(_u32p), cells.size, indices.ctypes.data_as(_u32p), indices.size,
                                              direct.ctypes.data_as(_i32p), direct.size, half.ctypes.data_as(_f64p))
        if rc < 0:
            raise RtiowError(rc, "rtiow_debug_volume_grid_plan")
        out.update(cells=cells, indices=indices[:out["index_entries"]], direct_list=direct[:out["direct"]], halfwidth=half)
    return out


def debug_gather_schedule(devices, rows, width, precision=32, mode=GATHER_RCCL, fail_at=-1, fallback=False):
    """The exchange's schedule (rtiow_group_gather's own) run against a recorder: (list of 8-tuples, return code).
    Host only -- no GPU, no RCCL.  Record layout: csrc/rtiow_group.hip, rtiow_debug_gather_schedule.
    fallback=True: with RTIOW_GATHER_AUTO's chain (a transport that fails at gather time -> drain -> the next one, from the top);
    the last record is then (12, -1, transport that carried the image, ...)."""
    lib = load_hip_library(debug=True)
    n = len(devices)
    cap = 3 * (16 * n + 16) + 8
    if fallback:
        mode = int(mode) | 0x100
    rec = (ctypes.c_int64 * (8 * cap))()
    rc = ctypes.c_int(0)
    got = lib.rtiow_debug_gather_schedule(n, (ctypes.c_int * n)(*devices), (ctypes.c_int * n)(*rows), int(width), int(precision), int(mode), int(fail_at),
                                          rec, cap, ctypes.byref(rc))
    if got < 0:
        raise RtiowError(got, "rtiow_debug_gather_schedule: bad arguments")
    return [tuple(rec[8 * k: 8 * k + 8]) for k in range(got)], rc.value


class RendererGroup:
    """Several GPUs of one node driven from this process (rtiow_group_*, include/rtiow.h): interleaved
    row strips, one exchange to device 0 after the render (RCCL, or peer copies), de-interleaved there.
    `devices` may repeat a device: the ranks then share it (how the N-rank logic is tested on one GPU).

    STDOUT: RCCL prints a version banner ("RCCL version : ...") on the process's stdout when its first communicator is created, i.e.
    inside this constructor's rtiow_group_create on distinct devices.  The library does not touch file descriptors; a
    caller whose stdout is data passes quiet_stdout=True, which points fd 1 at stderr for the duration of the constructor (process-wide:
    only for callers with no other thread writing to stdout), or does the same around the call itself (bench.py, the executables)."""

    def __init__(self, ngpus=1, precision=32, strip_rows=8, gather=GATHER_AUTO, devices=None, quiet_stdout=False):
        saved = -1
        if quiet_stdout:
            sys.stdout.flush()
            saved = os.dup(1)
            os.dup2(2, 1)
        try:
            self._create(ngpus, precision, strip_rows, gather, devices)
        finally:
            if saved >= 0:
                sys.stdout.flush()
                os.dup2(saved, 1)
                os.close(saved)

    def _create(self, ngpus, precision, strip_rows, gather, devices):
        self._lib = load_hip_library()
        self.precision, self.dtype, self.ngpus = precision, _dtype(precision), int(ngpus)
        self._g = ctypes.c_void_p()
        devs = (ctypes.c_int * self.ngpus)(*[int(d) for d in devices]) if devices is not None else None
        if devices is not None and len(devices) != self.ngpus:
            raise ValueError("devices must list one device per rank")
        rc = self._lib.rtiow_group_create(self.ngpus, devs, int(precision), int(strip_rows), int(gather), ctypes.byref(self._g))
        if rc:
            self._g = None
            why = self._lib.rtiow_group_create_error().decode(errors="replace")
            raise RtiowError(rc, "rtiow_group_create(%d GPUs) failed: %s" % (self.ngpus, why or "are that many GPUs visible?"))
        self.width = self.height = 0

    def _check(self, rc):
        if rc:
            raise RtiowError(rc, self._lib.rtiow_group_last_error_string(self._g).decode(errors="replace"))

    def close(self):
        if getattr(self, "_g", None):
            self._lib.rtiow_group_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_scene(self, scene):
        self._check(_set_scene(self._lib.rtiow_group_set_scene, self._g, scene, self.dtype))

    def set_camera(self, cam):
        want = CameraF64 if self.precision == 64 else CameraF32
        if not isinstance(cam, want):
            raise TypeError("camera precision does not match the group")
        self._check(self._lib.rtiow_group_set_camera(self._g, ctypes.addressof(cam)))
        self.width, self.height = cam.img_width, cam.img_height

    def set_scene_source(self, source):
        self._check(self._lib.rtiow_group_set_scene_source(self._g, source))

    def set_schedule(self, schedule, waves_per_simd=0):
        self._check(self._lib.rtiow_group_set_schedule(self._g, schedule, waves_per_simd))

    def init_rng(self, seed=1227):
        self._check(self._lib.rtiow_group_init_rng(self._g, ctypes.c_uint64(seed)))

    def render(self, threads=8):
        """All devices render their strips; returns the slowest device's HIP-event kernel time (ms)."""
        ms = ctypes.c_float(0)
        self._check(self._lib.rtiow_group_render(self._g, int(threads), ctypes.byref(ms)))
        return ms.value

    def gather(self):
        self._check(self._lib.rtiow_group_gather(self._g))

    def member(self, rank):
        """Rank `rank`'s own handle as a borrowed Renderer (per-device stats, count_segments, knobs)."""
        h = ctypes.c_void_p()
        self._check(self._lib.rtiow_group_member(self._g, int(rank), ctypes.byref(h)))
        return Renderer._borrow(self._lib, h, self.precision, self.width, self.height)

    def read_framebuffer(self):
        """Exchange + de-interleave on device 0, then the full [H, W, 3] image."""
        out = np.empty((self.height, self.width, 3), self.dtype)
        self._check(self._lib.rtiow_group_read_framebuffer(self._g, out.ctypes.data, out.nbytes))
        return out

    def stats(self):
        st = GroupStats()
        self._check(self._lib.rtiow_group_get_stats(self._g, ctypes.byref(st)))
        d = {name: getattr(st, name) for name, _ in GroupStats._fields_ if name != "kernel_ms"}
        d["kernel_ms"] = [st.kernel_ms[k] for k in range(min(st.ngpus, GROUP_MAX_STATS))]
        d["transport_note"] = self._lib.rtiow_group_transport_note(self._g).decode(errors="replace")
        return d
