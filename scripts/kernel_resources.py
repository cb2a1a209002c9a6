"""Register / scratch / code-size figures of the render kernels for a set of -D defines, from the compiler's metadata
(no GPU: hipcc cross-compiles gfx950).  Usage: kernel_resources.py [-DNAME=VALUE ...] [--filter substring] [--keep out.s]"""
import os, sys
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
from raytracingincuda_amd.kernel_metadata import device_metadata

def metadata(defines=(), keep=None):
    meta, text = device_metadata(tuple(defines), keep)
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
    for name, v in sorted(metadata(args, keep).items()):
        if filt in name:
            print(name, {k: x for k, x in v.items() if k != "symbol"})
