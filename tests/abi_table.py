"""What tests/test_abi.py holds the progressive-preview part of the C-ABI and its Python wrappers to.  Data only, written by hand from
include/rtiow.h and the wrappers' documented signatures -- not read from raytracingincuda_amd/api.py, which is what it checks.
A new call adds one row to SYMBOLS and its wrapper's rows below."""

# symbol of include/rtiow.h -> (number of parameters, the arguments of a call with a NULL handle: it answers -1 before any device work)
SYMBOLS = {
    "rtiow_accumulate_reset": (1, (None,)),
    "rtiow_accumulate": (4, (None, 4, 0, None)),
    "rtiow_accumulated_samples": (2, (None, None)),
    "rtiow_accumulate_adaptive": (7, (None, 4, 0, 0.1, 100, None, None)),
    "rtiow_read_adaptive_state": (4, (None, None, None, 0)),
    "rtiow_read_linear": (3, (None, None, 0)),
    "rtiow_render_guides": (2, (None, None)),
    "rtiow_read_guides": (5, (None, None, None, None, 0)),
    "rtiow_denoise": (7, (None, 5, 1.0, 1.0, 1.0, 1.0, None)),
    "rtiow_read_denoised": (3, (None, None, 0)),
    "rtiow_denoised_device_ptr": (3, (None, None, None)),
    "rtiow_read_variance": (3, (None, None, 0)),
    "rtiow_denoise_variance": (7, (None, 5, 4.0, 1.0, 1.0, 1.0, None)),
    "rtiow_history_reset": (1, (None,)),
    "rtiow_history_update": (6, (None, 0.1, 0.9, 32.0, None, None)),
    "rtiow_history_commit": (1, (None,)),
    "rtiow_read_history": (4, (None, None, None, 0)),
    "rtiow_history_device_ptr": (3, (None, None, None)),
    "rtiow_denoise_history": (7, (None, 5, 1.0, 1.0, 1.0, 1.0, None)),
    "rtiow_set_guide_mode": (4, (None, 1, 8, 0.0)),
    "rtiow_read_filter_guides": (6, (None, None, None, None, None, 0)),
    "rtiow_history_plan": (6, (None, 0.1, 0.9, 16.0, None, None)),
    "rtiow_read_history_plan": (3, (None, None, 0)),
    "rtiow_accumulate_budget": (7, (None, 2, 1, 16.0, 100, None, None)),
    "rtiow_history_update_clipped": (9, (None, 0.1, 0.9, 16.0, 1, 0.75, None, None, None)),
    "rtiow_denoise_history_variance": (8, (None, 5, 4.0, 0.1, 0.2, 0.05, 1, None)),
    "rtiow_read_history_variance": (3, (None, None, 0)),
    "rtiow_history_commit_filtered": (7, (None, 0.1, 0.1, 0.2, 0.05, 1.0, None)),
    "rtiow_read_history_base": (4, (None, None, None, 0)),
}

# #define NAME VALUE lines include/rtiow.h must carry, and the api constant of the same value
HEADER_DEFINES = {"RTIOW_ABI_VERSION": (6, "ABI_VERSION"), "RTIOW_GUIDES_FIRST_HIT": (0, "GUIDES_FIRST_HIT"), "RTIOW_GUIDES_SPECULAR": (1, "GUIDES_SPECULAR")}

# Renderer member -> its parameters after self, or None where only its existence is pinned
METHODS = {
    "accumulate": None, "reset_accumulation": None,
    "accumulate_adaptive": None, "adaptive_state": None,
    "read_linear": None, "render_guides": None, "guides": None, "read_denoised": None, "denoised_device_ptr": None,
    "denoise": None,
    "variance": None, "accumulate_with_variance": None,
    "denoise_variance": ("levels", "sigma_variance", "sigma_normal", "sigma_albedo", "sigma_depth", "sync"),
    "history_reset": None, "history": None, "history_device_ptr": None,
    "history_update": ("depth_tol", "normal_cos", "max_history", "sync"),
    "history_commit": (),
    "denoise_history": None,                                  # denoise's, see SAME_AS
    "set_guide_mode": None, "filter_guides": None,
    "history_plan": ("depth_tol", "normal_cos", "max_history", "sync"),
    "history_plan_lengths": None,
    "accumulate_budget": ("samples", "target", "min_samples", "max_samples", "sync"),
    "history_update_clipped": ("clip_radius", "clip_gamma", "depth_tol", "normal_cos", "max_history", "sync"),
    "denoise_history_variance": ("levels", "sigma_variance", "sigma_normal", "sigma_albedo", "sigma_depth", "variance_radius", "sync"),
    "history_variance": (),
    "history_commit_filtered": ("sigma_color", "sigma_normal", "sigma_albedo", "sigma_depth", "feedback", "sync"),
    "history_base": (),
}
PROPERTIES = ("accumulated_samples",)

# (method, parameter, what its default equals: the name of an api constant, or the value itself)
DEFAULTS = [
    ("denoise_variance", "sigma_variance", "DENOISE_SIGMA_VARIANCE"),
    ("history_update", "depth_tol", "HISTORY_DEPTH_TOL"),
    ("history_update", "normal_cos", "HISTORY_NORMAL_COS"),
    ("history_update", "max_history", "HISTORY_MAX"),
    ("history_update", "sync", True),
    ("accumulate_budget", "samples", "BUDGET_CHUNK"),
    ("accumulate_budget", "target", "BUDGET_TARGET"),
    ("accumulate_budget", "min_samples", "BUDGET_MIN_SAMPLES"),
    ("history_update_clipped", "clip_radius", "HISTORY_CLIP_RADIUS"),
    ("history_update_clipped", "clip_gamma", "HISTORY_CLIP_GAMMA"),
    ("denoise_history_variance", "variance_radius", "HISTORY_VARIANCE_RADIUS"),
    ("denoise_history_variance", "sigma_variance", "HISTORY_SIGMA_VARIANCE"),
    ("history_commit_filtered", "sigma_color", "HISTORY_FEEDBACK_SIGMA_COLOR"),
    ("history_commit_filtered", "sigma_normal", "DENOISE_SIGMA_NORMAL"),
    ("history_commit_filtered", "sigma_albedo", "DENOISE_SIGMA_ALBEDO"),
    ("history_commit_filtered", "sigma_depth", "DENOISE_SIGMA_DEPTH"),
    ("history_commit_filtered", "feedback", "HISTORY_FEEDBACK"),
    ("history_commit_filtered", "sync", True),
]

INF = float("inf")
# api constant -> (lowest value the C entry check accepts, whether that bound itself is refused, highest value)
RANGES = {
    "DENOISE_SIGMA_VARIANCE": (0, True, INF),
    "HISTORY_DEPTH_TOL": (0, False, INF),
    "HISTORY_NORMAL_COS": (-1, False, 1),
    "HISTORY_MAX": (0, True, INF),
    "GUIDE_MAX_BOUNCES": (1, False, 16),
    "GUIDE_MAX_FUZZ": (0, False, INF),
    "BUDGET_CHUNK": (1, False, INF),
    "BUDGET_TARGET": (0, True, INF),
    "BUDGET_MIN_SAMPLES": (0, False, INF),
    "HISTORY_CLIP_RADIUS": (1, False, 3),
    "HISTORY_CLIP_GAMMA": (0, False, INF),
    "HISTORY_VARIANCE_RADIUS": (1, False, 3),
    "HISTORY_SIGMA_VARIANCE": (0, True, INF),
    "HISTORY_FEEDBACK_SIGMA_COLOR": (0, True, INF),
    "HISTORY_FEEDBACK": (0, True, 1),
}

# (method, the method it follows, the parameters whose defaults are that method's -- None: its whole parameter list and every default)
SAME_AS = [
    ("denoise_history", "denoise", None),
    ("history_plan", "history_update", None),                 # the plan of the update that follows
    ("denoise_variance", "denoise", ("levels", "sigma_normal", "sigma_albedo", "sigma_depth", "sync")),      # the guide defaults stay
    ("history_update_clipped", "history_update", ("depth_tol", "normal_cos", "max_history", "sync")),
    ("denoise_history_variance", "denoise_variance", ("levels", "sigma_normal", "sigma_albedo", "sigma_depth", "sync")),
    ("history_commit_filtered", "denoise_history", ("sigma_normal", "sigma_albedo", "sigma_depth")),
]
