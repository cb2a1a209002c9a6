"""The plans of both uniform grids, pinned: tests/golden/grid_plan_digests.json, one SHA-256 per scene (tests/grid_plan_digests.py).

    python tests/golden/make_grid_plan_digests.py [--library path/to/librtiow_hip_debug.so] [--commit REF]

Run it on the commit whose plans are to be kept, BEFORE changing the planning code: with --library, on the test build of another
checkout (for instance a `git archive` of the parent commit, built there), --commit naming the commit that build was made from.
The record names the commit and the library's build id.  Host arithmetic only: no GPU.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "grid_plan_digests.json")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--library", default="")
    ap.add_argument("--commit", default="HEAD")
    a = ap.parse_args()
    if a.library:
        os.environ["RTIOW_HIP_DEBUG_LIBRARY"] = os.path.abspath(a.library)
    import raytracingincuda_amd as rt
    from tests.grid_plan_digests import all_digests
    from tests.oracle_lib import Oracle
    record = {"commit": subprocess.run(["git", "-C", ROOT, "rev-parse", a.commit], check=True, capture_output=True, text=True).stdout.strip(),
              "build_id": rt.load_hip_library(debug=True).rtiow_build_id().decode()}
    record.update(all_digests(rt, Oracle()))
    with open(OUT, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s: %d + %d scenes on %s" % (os.path.relpath(OUT, ROOT), len(record["grid_plan"]), len(record["large_grid_plan"]), record["commit"][:12]))


if __name__ == "__main__":
    main()
