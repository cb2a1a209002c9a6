"""What drives a Renderer in the preview-chain tests and in the scripts/history_*_probe.py measurements: setting a handle up, sampling,
reading its state as tests/preview_model.py takes it, the checks of an update against the model, and the walks the quality tests and the
probes share.  `rt` is the package, handed in by the caller; nothing here imports it."""
import math

import numpy as np

from tests.preview_model import as_base, clipped_np, luminance, same_bits, update_np

E_BADARG, E_STATE = -1, -2
INF = float("inf")
LOOKFROM = (13.0, 2.0, 3.0)
SLACK = 1.15                 # the quality tests allow 15 % over the values their probes measured
# (base view, current view) of every plan of tests/test_history_budget.py; tests/test_preview_views.py counts their classes of pixel
# on the CPU
BUDGET_PAIRS = (("home", "orbit"), ("home", "dolly"), ("home", "roll"), ("orbit", "home"), ("roll", "home"))
# The base of those tests is committed after the adaptive pattern of sample(): every pixel 4 or 8 samples.  Caps: below both counts
# (every covered pixel at the cap), between them (all three classes in one plan), and the default 16 (every covered pixel below).
CAP_LOW, CAP_MIX = 2.5, 6.0


def history_defaults(rt):
    return (rt.api.HISTORY_DEPTH_TOL, rt.api.HISTORY_NORMAL_COS, rt.api.HISTORY_MAX)


def guide_sigmas(rt):
    return (rt.api.DENOISE_SIGMA_NORMAL, rt.api.DENOISE_SIGMA_ALBEDO, rt.api.DENOISE_SIGMA_DEPTH)


# ---- views

def orbit(deg, lookfrom=LOOKFROM):
    """lookfrom turned by `deg` degrees about the y axis."""
    a = math.radians(deg)
    x, y, z = lookfrom
    return (x * math.cos(a) + z * math.sin(a), y, -x * math.sin(a) + z * math.cos(a))


def moves(rt, prec, W, H, B=10):
    """The reference's view and three small moves of it: an orbit, a dolly towards the scene and a roll."""
    look = lambda **kw: rt.camera_look(prec, W, H, 1, B, **kw)
    return {"home": look(), "orbit": look(lookfrom=orbit(1.5)), "dolly": look(lookfrom=tuple(0.96 * v for v in LOOKFROM)),
            "roll": look(vup=(0.05, 1.0, 0.02))}


def budget_moves(rt, prec, W, H, B=10):
    """The home view and the orbit of moves(), with a dolly and a roll of their own.  moves()'s dolly (4 % towards the scene) and roll
    (vup tilted mostly along the view axis) leave under 1 % of these frames without history; a dolly 4 % AWAY from the scene brings a
    border into view and vup tilted across the view axis rolls the frame by about 6 degrees, which leave 4 to 10 %
    (tests/test_preview_views.py counts them on the CPU)."""
    cams = moves(rt, prec, W, H, B)
    cams["dolly"] = rt.camera_look(prec, W, H, 1, B, lookfrom=tuple(1.04 * v for v in LOOKFROM))
    cams["roll"] = rt.camera_look(prec, W, H, 1, B, vup=(0.0, 1.0, 0.1))
    return cams


# ---- a handle, set up and sampled

def begin(r, rt, prec, scene_id, cam, source=3, sched=None, shard=None, seed=1227):
    """scene_id: a built-in scene's id, or scene tables as they are (tests/range_scene.py)."""
    r.set_camera(cam)
    r.set_scene(scene_id if isinstance(scene_id, dict) else rt.build_scene(scene_id, prec))
    r.set_scene_source(source)
    if sched is not None:
        r.set_schedule(sched, 0)
    if shard:
        r.set_shard(*shard)
    r.init_rng(seed)


def setup(r, rt, prec, scene_id, W, H, S=1, B=25, source=3, sched=None, shard=None, seed=1227):
    begin(r, rt, prec, scene_id, rt.camera(prec, W, H, S, B), source, sched, shard, seed)


def one_shot(rt, prec, scene_id, W, H, S, B, source=3, sched=2, shard=None):
    with rt.Renderer(0, prec) as r:
        setup(r, rt, prec, scene_id, W, H, S, B, source, sched, shard)
        r.render(0)
        return r.read_framebuffer()


def move(r, cam, seed=1227):
    r.set_camera(cam)
    r.init_rng(seed)


def run_mixed(r, calls):
    """min_samples = 4, samples = 4: the first call runs everyone, later calls use the frame's median error after it as the threshold (a
    mix of counts).  Returns the thresholds so that other configurations can replay the same calls."""
    r.accumulate_adaptive(4, 0.0, min_samples=4)
    thr = None
    for _ in range(calls - 1):
        if thr is None:
            thr = float(np.median(r.adaptive_state()[1]))
        r.accumulate_adaptive(4, thr, min_samples=4)
    return [thr] * (calls - 1)


def sample(r, adaptive, calls=2):
    """Plain chunks, or run_mixed's pattern: everyone 4 samples, then the median error as the threshold (a mix of counts)."""
    if not adaptive:
        for _ in range(calls):
            r.accumulate(3)
        return
    r.accumulate_adaptive(4, 0.0, min_samples=4)
    thr = float(np.median(r.adaptive_state()[1]))
    for _ in range(calls - 1):
        r.accumulate_adaptive(4, thr, min_samples=4)


def state(r, adaptive):
    """What section 11 reads of the current frame: colour and count of rtiow_read_linear, normal and depth of the guides."""
    c = r.read_linear()
    n = r.adaptive_state()[0] if adaptive else np.full(c.shape[:2], r.accumulated_samples, np.int32)
    normal, _, depth = r.guides()
    return {"c": c, "n": n, "N": normal, "t": depth}


def filter_state(r):
    n, a, z, _ = r.filter_guides()
    return n, a, z


# ---- a handle against the model

def check_against_err(r, where):
    """Section 10's plane: sqrt(V) / (m + 1e-3) is the published err where n >= 2, and V == 0 exactly where n < 2."""
    counts, err = r.adaptive_state()
    V = r.variance()
    assert V.dtype == r.dtype and V.shape == counts.shape, where
    assert (V >= 0).all() and np.isfinite(V).all(), where
    assert (V[counts < 2] == 0).all(), where
    m = luminance(r.read_linear().astype(np.float64))
    have = counts >= 2
    assert have.any() or (counts < 2).all(), where
    np.testing.assert_allclose(np.sqrt(V.astype(np.float64))[have] / (m[have] + 1e-3), err[have].astype(np.float64), rtol=1e-5, atol=1e-12,
                               err_msg=str(where))
    return counts, V


def check_update(r, cam, cur, base, params, where, same=same_bits):
    """history() and the pixel count after an update with `params` against the model; returns the model's.  same: how colours are
    compared -- same_bits_nan where a colour can be NaN (tests/test_number_range.py); lengths and counts are always compared strictly."""
    count = r.history_update(*params)
    rgb, length = r.history()
    want_c, want_m, want_count = update_np(cam, cur, base, *params)
    assert same_bits(length, want_m), where
    assert same(rgb, want_c), where
    assert count == want_count, (where, count, want_count)
    return want_c, want_m, want_count


def check_clipped(r, cam, cur, base, params, radius, gamma, where, same=same_bits):
    """A plain update, then the clipped one with the same three arguments, against each other and against the model; the clipped
    image is what the handle holds afterwards.  Returns the model's.  same: as in check_update."""
    plain_count = r.history_update(*params)
    plain_rgb, plain_len = r.history()
    count, clipped = r.history_update_clipped(radius, gamma, *params)
    rgb, length = r.history()
    want = clipped_np(cam, cur, base, params, radius, gamma, same)
    assert same_bits(length, want["M"]), where
    assert same(rgb, want["C"]), where
    assert (count, clipped) == (want["reprojected"], want["clipped"]), (where, count, clipped, want["reprojected"], want["clipped"])
    assert same_bits(length, plain_len) and count == plain_count, where
    assert same(plain_rgb, want["plain_C"]), where
    keep = ~want["mask"]
    assert same(np.ascontiguousarray(rgb[keep]), np.ascontiguousarray(plain_rgb[keep])), where
    return want


def commit_base(r, cam, params):
    """The current accumulation becomes the base (no base before it); returns it as the model takes it."""
    cur = state(r, True)
    c0, m0, _ = check_update(r, cam, cur, None, params, "the base frame")
    r.history_commit()
    return as_base(cam, cur, c0, m0)


# ---- the walks of the quality tests and of scripts/history_*_probe.py

def orbit_reference(rt, scene_id, frames=8, step_deg=0.5, W=320, H=180, B=50, prec=32, ref_samples=1024):
    """The linear image of ref_samples samples at the last camera of orbit_walk."""
    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, scene_id, rt.camera_look(prec, W, H, 1, B, lookfrom=orbit(step_deg * (frames - 1))))
        r.accumulate(ref_samples)
        return r.read_linear().astype(np.float64)


def orbit_walk(rt, scene_id, frames=8, step_deg=0.5, spp=4, W=320, H=180, B=50, prec=32, params=None, ref=None):
    """`frames` cameras, lookfrom turned step_deg about the y axis per frame, spp samples each with independent noise
    (init_rng(1227 + frame)), update and commit every frame.  Returns the linear images of the last frame: reference (orbit_reference),
    noisy accumulation, temporal image, denoise() and denoise_history() (both squared back to linear)."""
    params = params or history_defaults(rt)
    cams = [rt.camera_look(prec, W, H, 1, B, lookfrom=orbit(step_deg * k)) for k in range(frames)]
    out = {"ref": ref if ref is not None else orbit_reference(rt, scene_id, frames, step_deg, W, H, B, prec)}
    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, scene_id, cams[0])
        for k, cam in enumerate(cams):
            move(r, cam, 1227 + k)
            r.accumulate(spp)
            out["reprojected"] = r.history_update(*params)
            if k == frames - 1:
                out["noisy"] = r.read_linear().astype(np.float64)
                out["temporal"] = r.history()[0].astype(np.float64)
                out["denoise"] = r.denoise().astype(np.float64) ** 2
                out["denoise_history"] = r.denoise_history().astype(np.float64) ** 2
            else:
                r.history_commit()
    return out


def clip_walk(rt, scene_id, step_deg, clip, max_history=None, frames=8, spp=4, W=320, H=180, B=50, prec=32, denoise=True):
    """orbit_walk with history_update_clipped(*clip) in place of history_update (clip = None: the plain update).  Returns the linear
    images of the last frame: temporal image and denoise_history() of it (squared back to linear)."""
    a = rt.api
    params = (a.HISTORY_DEPTH_TOL, a.HISTORY_NORMAL_COS, a.HISTORY_MAX if max_history is None else max_history)
    cams = [rt.camera_look(prec, W, H, 1, B, lookfrom=orbit(step_deg * k)) for k in range(frames)]
    out = {}
    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, scene_id, cams[0])
        for k, cam in enumerate(cams):
            move(r, cam, 1227 + k)
            r.accumulate(spp)
            if clip is None:
                out["reprojected"], out["clipped"] = r.history_update(*params), 0
            else:
                out["reprojected"], out["clipped"] = r.history_update_clipped(*clip, *params)
            if k == frames - 1:
                out["temporal"] = r.history()[0].astype(np.float64)
                if denoise:
                    out["denoise_history"] = r.denoise_history().astype(np.float64) ** 2
            else:
                r.history_commit()
    return out


def feedback_walk(rt, scene_id, step_deg, clip, commit, frames=8, spp=4, W=320, H=180, B=50, prec=32, each_frame=None):
    """clip_walk with the commit chosen: commit = None is history_commit(), otherwise the keyword arguments of
    history_commit_filtered() ({}: its defaults).  clip = None: the plain update.  Returns the linear images of the last frame -- temporal
    image and denoise_history() of it (squared back to linear) -- and its length plane; each_frame(k, r), if given, is called after every
    update."""
    params = history_defaults(rt)
    cams = [rt.camera_look(prec, W, H, 1, B, lookfrom=orbit(step_deg * k)) for k in range(frames)]
    out = {}
    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, scene_id, cams[0])
        for k, cam in enumerate(cams):
            move(r, cam, 1227 + k)
            r.accumulate(spp)
            if clip is None:
                out["reprojected"] = r.history_update(*params)
            else:
                out["reprojected"] = r.history_update_clipped(*clip, *params)[0]
            if each_frame is not None:
                each_frame(k, r)
            if k == frames - 1:
                rgb, length = r.history()
                out["temporal"], out["length"] = rgb.astype(np.float64), length.astype(np.float64)
                out["denoise_history"] = r.denoise_history().astype(np.float64) ** 2
            elif commit is None:
                r.history_commit()
            else:
                r.history_commit_filtered(**commit)
    return out


def walk(rt, scene_id, sample, params=None, frames=8, step_deg=0.5, W=320, H=180, B=50, prec=32):
    """orbit_walk with the frame's sampling left to `sample(r)`: `frames` cameras, lookfrom turned step_deg about the y axis per frame,
    independent noise (init_rng(1227 + frame)), the plan, the samples, update and commit every frame.  Returns the primary rays of the
    whole walk (summed from stats()), the temporal image of the last frame and that frame's plan."""
    params = params or history_defaults(rt)
    cams = [rt.camera_look(prec, W, H, 1, B, lookfrom=orbit(step_deg * k)) for k in range(frames)]
    out = {"rays": 0}
    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, scene_id, cams[0])
        for k, cam in enumerate(cams):
            move(r, cam, 1227 + k)
            r.history_plan(*params)
            out["rays"] += sample(r)
            r.history_update(*params)
            if k == frames - 1:
                out["temporal"] = r.history()[0].astype(np.float64)
                out["plan"] = r.history_plan_lengths()
            else:
                r.history_commit()
    return out


def uniform_sampler(spp=4):
    def sample(r):
        r.accumulate(spp)
        return r.stats()["primary_rays"]
    return sample


def budget_sampler(chunk, target, min_samples):
    def sample(r):
        rays = 0
        while True:
            active = r.accumulate_budget(chunk, target, min_samples)[1]
            rays += r.stats()["primary_rays"]
            if active == 0:
                return rays
    return sample


def compare(uniform, budget, ref):
    """{rays, frame, disoccluded}: budget / uniform of the walk's primary rays, the whole-frame MSE and the MSE over the pixels without
    history in the last frame's plan (the budget walk's; the uniform walk's is the same set wherever both bases are non-empty)."""
    gone = budget["plan"] == 0
    mse = lambda w, sel: float(np.mean((w["temporal"][sel] - ref[sel]) ** 2))
    everything = np.ones_like(gone)
    return {"rays": budget["rays"] / uniform["rays"], "frame": mse(budget, everything) / mse(uniform, everything),
            "disoccluded": mse(budget, gone) / mse(uniform, gone), "disoccluded_pixels": int(gone.sum()),
            "mse_uniform": mse(uniform, everything), "mse_budget": mse(budget, everything),
            "mse_uniform_disoccluded": mse(uniform, gone), "mse_budget_disoccluded": mse(budget, gone),
            "rays_uniform": int(uniform["rays"]), "rays_budget": int(budget["rays"])}
