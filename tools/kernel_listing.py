#!/usr/bin/env python
"""Registers, LDS, scratch and occupancy of every kernel of some csrc/*.hip files, from the compiler's own listing (the build's
flags, gfx950, no GPU needed); with ``--against TREE`` also whether each kernel's instructions are those of the same file in
another checkout of the project (a kernel that became a template is matched by its source name to the instantiation whose
mangled template arguments ``--instance`` gives).

    python tools/kernel_listing.py ssal_train_icnet_pool.hip ssal_train_icnet_pyramid.hip ssal_train_icnet_cascade.hip \\
        --against ../parent-checkout --instance ILi1024ELi256EEEv --out profiles/r28_train_icnet_pool_kernels.json
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from semanticsegmentationactivelearning_amd import build  # noqa: E402

META = re.compile(r"\.agpr_count:\s+(\d+).*?\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?"
                  r"\.private_segment_fixed_size:\s+(\d+).*?\.sgpr_count:\s+(\d+).*?\.vgpr_count:\s+(\d+)", re.S)


def listing(tree, name):
    src = os.path.join(tree, "semanticsegmentationactivelearning_amd", "csrc", name)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.check_call(["hipcc"] + build.CFLAGS + ["-S", "--cuda-device-only", src, "-o", out], stderr=subprocess.DEVNULL)
        return open(out).read()


def kernels(text):
    """{mangled name: [instruction lines]}"""
    out = {}
    for m in re.finditer(r"^(_ZN4ssal[^\s:]+):[^\n]*\n(.*?)s_endpgm", text, re.S | re.M):
        body = [line.split(";")[0].strip() for line in m.group(2).split("\n")]
        out[m.group(1)] = [line for line in body if line and not line.startswith(".")]
    return out


def resources(text):
    occ = dict(zip(re.findall(r"\.amdhsa_kernel (\S+)", text), re.findall(r"^; Occupancy: (\d+)", text, re.M)))
    out = {}
    for m in META.finditer(text):
        out[m.group(3)] = {"agpr": int(m.group(1)), "lds_bytes": int(m.group(2)), "scratch_bytes": int(m.group(4)),
                           "sgpr": int(m.group(5)), "vgpr_total": int(m.group(6)),
                           "waves_per_simd": int(occ.get(m.group(3), 0))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("files", nargs="+")
    ap.add_argument("--against", help="another checkout of the project")
    ap.add_argument("--instance", default="", help="template arguments (mangled) of the instantiation an earlier plain kernel became")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    rec = {"flags": build.CFLAGS, "files": {}}
    for name in a.files:
        text = listing(ROOT, name)
        entry = {"kernels": resources(text)}
        if a.against and os.path.exists(os.path.join(a.against, "semanticsegmentationactivelearning_amd", "csrc", name)):
            mine, theirs = kernels(text), kernels(listing(a.against, name))
            stem = lambda k: re.search(r"\d+(k_[a-z0-9_]+?)(?:I|E)", k).group(1)
            by_stem = {stem(k): k for k in mine if a.instance and a.instance in k}
            cmp = {}
            for k in theirs:
                new = k if k in mine else by_stem.get(stem(k))
                cmp[k] = ("no such kernel" if new is None else
                          {"kernel": new, "instructions": len(theirs[k]), "identical": theirs[k] == mine[new]})
            entry["against_other_checkout"] = cmp
        rec["files"][name] = entry
        for k, v in entry["kernels"].items():
            print(name, k, v)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
