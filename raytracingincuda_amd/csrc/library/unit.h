// unit.h -- what every gfx950 translation unit of librtiow_hip.so that launches kernels starts from (rtiow_hip.hip, rtiow_upscale.hip,
// rtiow_upscale_wide.hip, rtiow_large.hip, rtiow_large_preview.hip, rtiow_large_upscale.hip, rtiow_volume.hip,
// rtiow_volume_preview.hip, rtiow_volume_upscale.hip): the system headers, the
// C-ABI and the device and library headers, in the one order all nine are compiled in.  Internal linkage throughout: a template a unit does not call is not instantiated there, so which code object holds
// which kernel is decided by the unit, not here.  A unit includes this first and then only what is its own.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <array>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <mutex>
#include <vector>

#include "rtiow.h"
#ifdef RTIOW_DEBUG_API
#include "rtiow_debug.h"
#endif

#include "../device/xorwow.h"
#include "../device/params.h"
#include "../device/probes.h"
#include "../device/vecmath.h"
#include "../device/sampling.h"
#include "../device/roots.h"
#include "../device/hit_loop.h"
#include "../device/hit_grid.h"
#include "../device/shade.h"
#include "../device/hit_coop.h"
#include "../device/pixel_io.h"
#include "../device/render_kernels.h"
#include "../device/cost_sort.h"
#include "../device/denoise.h"
#include "../device/denoise_variance.h"
#include "../device/history.h"
#include "../device/history_clip.h"
#include "../device/history_feedback.h"
#include "../device/history_budget.h"
#include "../device/temporal_noise.h"
#include "../device/guide_chain.h"
#include "../device/edge_resolve.h"
#include "../device/scene_motion.h"
#include "../device/edit_influence.h"
#include "xorwow_jump.h"
#include "handle.h"
#include "scene_tables.h"
#include "launch.h"             // and through it device/upscale.h and device/upscale_wide.h
#include "pass.h"
