"""Compare the device code of every kernel between two builds.

    python scripts/isa_diff_render_kernels.py --ref HEAD~1        # the tree at a git ref (exported with git archive) against the working tree
    python scripts/isa_diff_render_kernels.py BEFORE.s AFTER.s    # two `hipcc -S --cuda-device-only` listings
    python scripts/isa_diff_render_kernels.py --ref HEAD~1 --summary    # ... and what changed in each kernel that differs
    python scripts/isa_diff_render_kernels.py --ref HEAD~1 --unit rtiow_upscale.hip    # another translation unit than rtiow_hip.hip

Every function of the older listing is cut from its label to its .Lfunc_end and compared text for text with the newer one's, after the
function-local labels (.LBB<n>_<k>, .Lfunc_end<n>: n follows the order in which the module instantiates the functions) are renumbered
in order of appearance and the comments dropped, so that host code naming the kernels in another order does not count as a change.  This shows that a change
confined to host code or to new kernels (e.g. the ACCUM or ADAPT flag of persistent_body) leaves the existing device code as it was.  A
kernel the older build lacks is listed as new.  Exit status 1 if any of them differ or is missing.

--summary adds, for each kernel that differs, before -> after: the number of instructions, the VGPRs, the SGPR and VGPR spills and the
scratch bytes of the metadata both listings carry, and whether the multiset of floating-point and conversion mnemonics (FP) is the same,
which is what a restatement of the same arithmetic must leave alone.
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tarfile
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LABEL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)*")
FP = re.compile(r"_f32|_f64|rcp|sqrt|div_|floor|cvt")
RESOURCES = (("vgpr", "vgpr_count"), ("sgpr spills", "sgpr_spill_count"), ("vgpr spills", "vgpr_spill_count"), ("scratch", "private_segment_fixed_size"))


def listing(src_root, out, unit="rtiow_hip.hip"):
    from raytracingincuda_amd import build as b
    flags = [f for f in b.HIP_FLAGS if f != "-shared" and not f.startswith("-I")] + ["-I" + os.path.join(src_root, "include")]
    subprocess.run([b._hipcc()] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(src_root, "raytracingincuda_amd", "csrc", unit)],
                   check=True, stderr=subprocess.DEVNULL)
    return out


def normalised(body):
    seen = {}
    body = re.sub(r"[ \t]*;.*$", "", body, flags=re.M)        # assembler comments (they name blocks by their numbers too)
    return LABEL.sub(lambda m: seen.setdefault(m.group(0), ".L#%d" % len(seen)), body)


def bodies(path):
    text = open(path).read()
    out = {}
    for name in re.findall(r"^\s*\.type\s+([^,\s]+),@function", text, re.M):
        m = re.search(r"^%s:" % re.escape(name), text, re.M)
        out[name] = normalised(text[m.start():text.index(".Lfunc_end", m.end())])
    return out


def mnemonics(body):
    """The opcode of every instruction of a normalised body: what is neither a label nor a directive."""
    lines = (l.split() for l in body.splitlines())
    return [l[0] for l in lines if l and not l[0].endswith(":") and not l[0].startswith(".")]


def resources(path):
    """{kernel symbol: {key: value}} of the numbers in the listing's amdhsa.kernels metadata."""
    out = {}
    for entry in re.split(r"^  - ", open(path).read(), flags=re.M)[1:]:
        name = re.search(r"^\s+\.name:\s+(\S+)", entry, re.M)
        if name:
            out[name.group(1)] = {k: int(v) for k, v in re.findall(r"^\s+\.(\w+):\s+(\d+)\s*$", entry, re.M)}
    return out


def summary(name, old, new, res_old, res_new):
    a, b = mnemonics(old), mnemonics(new)
    parts = ["instructions %d -> %d" % (len(a), len(b))]
    parts += ["%s %d -> %d" % (label, res_old[name][key], res_new[name][key]) for label, key in RESOURCES]
    same = collections.Counter(m for m in a if FP.search(m)) == collections.Counter(m for m in b if FP.search(m))
    return "       " + "   ".join(parts) + "   fp/cvt mnemonics " + ("same" if same else "DIFFERENT")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("listings", nargs="*")
    ap.add_argument("--ref", default="")
    ap.add_argument("--summary", action="store_true")
    ap.add_argument("--unit", default="rtiow_hip.hip")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        if a.ref:
            tar = os.path.join(tmp, "ref.tar")
            subprocess.run(["git", "-C", ROOT, "archive", "-o", tar, a.ref], check=True)
            old_root = os.path.join(tmp, "ref")
            with tarfile.open(tar) as t:
                t.extractall(old_root)
            before, after = listing(old_root, os.path.join(tmp, "before.s"), a.unit), listing(ROOT, os.path.join(tmp, "after.s"), a.unit)
        elif len(a.listings) == 2:
            before, after = a.listings
        else:
            ap.error("give --ref REF or two listings")
        old, new = bodies(before), bodies(after)
        res_old, res_new = (resources(before), resources(after)) if a.summary else ({}, {})
    names = sorted(old)
    dem = dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()))
    diff = [n for n in names if old[n] != new.get(n)]
    print("kernels compared: %d, differing or missing: %d" % (len(names), len(diff)))
    for n in diff:
        print("  DIFF", dem[n])
        if a.summary and n in new:
            print(summary(n, old[n], new[n], res_old, res_new))
    added = [n for n in new if n not in old]
    for d in subprocess.run(["c++filt"], input="\n".join(added), capture_output=True, text=True, check=True).stdout.splitlines():
        print("  new", d)
    return 1 if diff or not names else 0


if __name__ == "__main__":
    sys.exit(main())
