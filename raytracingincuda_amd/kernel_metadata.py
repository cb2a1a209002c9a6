"""Per-kernel resources of rtiow_hip.hip (or another translation unit of the library) for gfx950, read from the compiler's metadata in a device-only listing (no GPU needed: hipcc
cross-compiles).  The register-budget tests and scripts/kernel_resources.py share it."""
import functools
import os
import re
import subprocess
import tempfile

from raytracingincuda_amd import build as b

_META = re.compile(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n\s+\.sgpr_count:\s+(\d+)\n\s+\.sgpr_spill_count:\s+(\d+)\n"
                   r"(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)")


@functools.lru_cache(maxsize=None)
def device_metadata(defines=(), keep=None, source="rtiow_hip.hip"):
    """(metadata, listing text) of rtiow_hip.hip built with the product's flags plus `defines` (a tuple of -D flags), compiled once per
    process and set of arguments.  metadata maps each demangled kernel name to its scratch, sgpr, sgpr_spill, vgpr and vgpr_spill;
    keep: a path to keep the listing at; source: the translation unit under csrc/ (rtiow_upscale.hip holds upscale_kernel,
    rtiow_upscale_wide.hip upscale_wide_kernel)."""
    with tempfile.TemporaryDirectory(prefix="rtiow_isa") as tmp:
        out = keep or os.path.join(tmp, "rtiow_hip.s")
        flags = [f for f in b.HIP_FLAGS if f != "-shared"]
        subprocess.run([b._hipcc()] + flags + list(defines) + ["-S", "--cuda-device-only", "-o", out, os.path.join(b.CSRC, source)],
                       check=True, stderr=subprocess.DEVNULL)
        text = open(out).read()
    found = list(_META.finditer(text))
    names = subprocess.run(["c++filt"], input="\n".join(m.group(1) for m in found), capture_output=True, text=True, check=True).stdout.splitlines()
    meta = {name: {"scratch": int(m.group(2)), "sgpr": int(m.group(3)), "sgpr_spill": int(m.group(4)), "vgpr": int(m.group(5)), "vgpr_spill": int(m.group(6)),
                   "symbol": m.group(1)}
            for m, name in zip(found, names)}
    return meta, text
