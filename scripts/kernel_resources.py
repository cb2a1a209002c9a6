"""Register / scratch / code-size figures of the render kernels for a set of -D defines, from the compiler's metadata
(no GPU: hipcc cross-compiles gfx950).  Usage: kernel_resources.py [-DNAME=VALUE ...] [--filter substring] [--keep out.s]
[--unit rtiow_large_preview.hip ...] [--json out.json]; --unit: another translation unit under csrc/ than rtiow_hip.hip (repeatable); --json: the kernels
the filter keeps as a record {unit, flags, kernels: {name without namespace and parameters: vgprs, sgprs, spills, scratch, instructions}}."""
import os, sys
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
from raytracingincuda_amd.kernel_metadata import device_metadata

def metadata(defines=(), keep=None, unit="rtiow_hip.hip"):
    meta, text = device_metadata(tuple(defines), keep, unit)
    # static instruction counts per kernel body (lines between the symbol's label and its s_endpgm)
    for v in meta.values():
        k = text.find("\n" + v["symbol"] + ":")
        if k < 0: continue
        e = text.find(".Lfunc_end", k)
        body = text[k:e]
        ins = [l.strip() for l in body.splitlines() if l.startswith("\t") and not l.strip().startswith((".", ";"))]
        v["insts"] = len(ins)
        v["valu"] = sum(1 for l in ins if l.startswith("v_"))
        v["salu"] = sum(1 for l in ins if l.startswith("s_"))
        v["lds"] = sum(1 for l in ins if l.startswith("ds_"))
    return meta

if __name__ == "__main__":
    args = sys.argv[1:]
    filt = "render_"
    keep = None
    if "--filter" in args:
        k = args.index("--filter"); filt = args[k + 1]; del args[k:k + 2]
    if "--keep" in args:
        k = args.index("--keep"); keep = args[k + 1]; del args[k:k + 2]
    units, out_json = [], None
    while "--unit" in args:                                  # --unit may be given more than once: one record of all their kernels
        k = args.index("--unit"); units.append(args[k + 1]); del args[k:k + 2]
    if "--json" in args:
        k = args.index("--json"); out_json = args[k + 1]; del args[k:k + 2]
    units = units or ["rtiow_hip.hip"]
    unit = ", raytracingincuda_amd/csrc/".join(units)
    kept = {}
    for u in units:
        kept.update({name: v for name, v in sorted(metadata(args, keep, u).items()) if filt in name})
    for name, v in kept.items():
        print(name, {k: x for k, x in v.items() if k != "symbol"})
    if out_json:
        import json, re
        short = lambda name: re.sub(r"^void |\(anonymous namespace\)::|\(.*$", "", name)
        record = {"unit": "raytracingincuda_amd/csrc/" + unit, "flags": "the product's (build.HIP_FLAGS)" + (" + " + " ".join(args) if args else ""),
                  "kernels": {short(name): {"vgprs": v["vgpr"], "sgprs": v["sgpr"], "sgpr_spills": v["sgpr_spill"], "vgpr_spills": v["vgpr_spill"],
                                            "scratch_bytes": v["scratch"], "instructions": v.get("insts")} for name, v in kept.items()}}
        with open(out_json, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
