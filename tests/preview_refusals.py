"""What the preview calls (INTEGRATION.md sections 9 to 16) answer in which state of a handle, stated once: the states, the calls with
their good arguments, the bad arguments and range ends of each, and -- in tests/golden/preview_refusals.txt -- the code and the text of
rtiow_last_error_string for every (state, call, arguments), grouped.  The expected answers were recorded from the library as it was before the
policy moved into csrc/library/preview_state.h (driven through drive() of tests/test_preview_refusals.py) and read against that
library's source; they are not produced by the code under test.

Two consumers: tests/test_preview_state.py feeds the table to tests/native/preview_state_main.cpp, which answers from preview_state.h
alone on the CPU, and tests/test_preview_refusals.py drives it through the library on the GPU."""
import os

NAN, INF = float("nan"), float("inf")
E_BADARG, E_STATE = -1, -2

# fp32, scene 1; a frame that is a multiple of neither 16 nor 8, so every launch has edge tiles; 1 sample per step
PRECISION, SCENE_ID, W, H, MAX_DEPTH = 32, 1, 40, 24, 4
SHARD = (1, 3, 8)                      # rank 1 of 3 in strips of 8 rows: 8 local rows

# ---- states: each a sequence of steps.  scene_camera: rtiow_set_camera (the home view) + rtiow_set_scene; rng: rtiow_init_rng;
# plain / adaptive: one chunk of 1 sample (rtiow_accumulate / rtiow_accumulate_adaptive); update, plan, commit: rtiow_history_update /
# _plan / _commit with their defaults; move: rtiow_set_camera (the orbit view); history_variance: rtiow_denoise_history_variance;
# shard: rtiow_set_shard(*SHARD)
_READY = ("scene_camera", "rng")
_UPDATED = _READY + ("plain", "update")
STATES = {
    "created": (),
    "scene_camera": ("scene_camera",),
    "rng": _READY,
    "plain_chunk": _READY + ("plain",),
    "adaptive_chunk": _READY + ("adaptive",),
    "updated": _UPDATED,
    "updated_chunk": _UPDATED + ("plain",),
    "planned": _READY + ("plan",),
    "committed": _UPDATED + ("commit",),
    "committed_moved": _UPDATED + ("commit", "move", "rng"),
    "history_variance": _UPDATED + ("history_variance",),
    # without a chunk, which tells the calls that look at the shard first from those that look at the accumulation first, and with one
    "sharded": ("scene_camera", "shard", "rng"),
    "sharded_chunk": ("scene_camera", "shard", "rng", "plain"),
}

# ---- calls: name -> (parameters, good values, {parameter: other values to try, one at a time}).  Output pointers are not parameters
# here: the drivers pass what the call needs.  "size": the call's npix or bytes as a difference from the right one.
_SIZE = (("size",), (0,), {"size": (1, -1)})
_NONE = ((), (), {})
_SIGMA = (0.0, -1.0, NAN, INF)
_FILTER = (("levels", "sigma_first", "sigma_normal", "sigma_albedo", "sigma_depth"), (2, 1.0, 1.0, 1.0, 1.0),
           {"levels": (0, 9, 1, 8), "sigma_first": _SIGMA, "sigma_normal": _SIGMA, "sigma_albedo": _SIGMA, "sigma_depth": _SIGMA})
_TOL = (("depth_tol", "normal_cos", "max_history"), (0.1, 0.9, 8.0),
        {"depth_tol": (-0.1, NAN, 0.0, INF), "normal_cos": (1.5, -1.5, NAN, -1.0, 1.0), "max_history": (0.0, -1.0, NAN, 1e-3, INF)})


def _with(base, params, good, more):
    return (base[0] + params, base[1] + good, dict(base[2], **more))


CALLS = {
    "rtiow_read_linear": _SIZE,
    "rtiow_render_guides": _NONE,
    "rtiow_read_guides": _SIZE,
    "rtiow_denoise": _FILTER,
    "rtiow_read_denoised": _SIZE,
    "rtiow_denoised_device_ptr": _NONE,
    "rtiow_read_variance": _SIZE,
    "rtiow_denoise_variance": _FILTER,
    "rtiow_history_reset": _NONE,
    "rtiow_history_update": _TOL,
    "rtiow_history_commit": _NONE,
    "rtiow_read_history": _SIZE,
    "rtiow_history_device_ptr": _NONE,
    "rtiow_denoise_history": _FILTER,
    "rtiow_set_guide_mode": (("mode", "max_bounces", "max_fuzz"), (1, 4, 0.1),
                             {"mode": (-1, 2, 0), "max_bounces": (0, 17, 1, 16), "max_fuzz": (-0.1, NAN, 0.0, INF)}),
    "rtiow_read_filter_guides": _SIZE,
    "rtiow_history_plan": _TOL,
    "rtiow_read_history_plan": _SIZE,
    "rtiow_accumulate_budget": (("samples", "min_samples", "target", "max_samples"), (1, 0, 4.0, 8),
                                {"samples": (0, -1), "min_samples": (-1, 8, 9), "target": (0.0, -1.0, NAN, INF), "max_samples": (-1, 0)}),
    "rtiow_history_update_clipped": _with(_TOL, ("clip_radius", "clip_gamma"), (1, 1.0),
                                          {"clip_radius": (0, 4, 3), "clip_gamma": (-0.1, NAN, 0.0, INF)}),
    "rtiow_denoise_history_variance": _with(_FILTER, ("variance_radius",), (1,), {"variance_radius": (0, 4, 3)}),
    "rtiow_read_history_variance": _SIZE,
    "rtiow_history_commit_filtered": (("sigma_first", "sigma_normal", "sigma_albedo", "sigma_depth", "feedback"), (1.0, 1.0, 1.0, 1.0, 0.5),
                                      {"sigma_first": _SIGMA, "sigma_normal": _SIGMA, "sigma_albedo": _SIGMA, "sigma_depth": _SIGMA,
                                       "feedback": (0.0, -0.5, 1.5, NAN, 1.0, 1e-6)}),
    "rtiow_read_history_base": _SIZE,
}
# The calls that only read: the state is as it was after them whatever they answer.  After any other call that returns 0 the GPU driver
# brings the handle back to the state by going through its steps again.
READ_ONLY = tuple(c for c in CALLS if c.startswith("rtiow_read_") or c.endswith("_device_ptr"))
# Parameters an entry point checks itself, with no word from preview_state.h: the CPU consumer leaves their cases to the GPU test.
OWN_PARAMETERS = ("size", "mode", "max_bounces", "max_fuzz", "samples", "min_samples", "target", "max_samples", "feedback")


def argument_sets(call):
    """The good arguments of `call`, then each parameter's other values in place of its good one: [(varied parameter or None, {name: value})]."""
    params, good, more = CALLS[call]
    out = [(None, dict(zip(params, good)))]
    for p in params:
        out += [(p, dict(zip(params, good), **{p: v})) for v in more.get(p, ())]
    return out


def cases():
    """Every (state, call, varied parameter, arguments), in the order both drivers go through them."""
    return [(s, c, varied, args) for s in STATES for c in CALLS for varied, args in argument_sets(c)]


def spell(args):
    """name=value ..., as the golden file and the native program's input write arguments (nan, inf and -inf as strtod reads them)."""
    return " ".join("%s=%r" % kv for kv in args.items())


def label(varied, args):
    """What names a case of a call in the golden file: the one argument that is not the good one."""
    return "good" if varied is None else spell({varied: args[varied]})


def program_line(state, call, args):
    """One line of input to tests/native/preview_state_main.cpp: steps | call | arguments."""
    return "%s | %s | %s" % (" ".join(STATES[state]), call, spell(args))


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "preview_refusals.txt")


def expected():
    """{(state, call, label): (code, message)} of the golden file; the message of a call that went through is ''.  Its lines are
    `call | labels | states | code | message`: the arguments (label()) that every state answers alike stand together, and so do the
    states that answer them alike (`*`: every state), which is the recording regrouped and nothing else."""
    out = {}
    with open(GOLDEN) as f:
        for line in f:
            call, labels, states, code, message = line.rstrip("\n").split(" | ", 4)
            for state in (STATES if states == "*" else states.split()):
                for case in labels.split():
                    assert (state, call, case) not in out, (state, call, case)
                    out[(state, call, case)] = (int(code), message)
    return out
