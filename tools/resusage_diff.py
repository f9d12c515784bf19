#!/usr/bin/env python3
"""Compare the compiler's kernel-resource-usage remarks of two builds of a translation unit.

    hipcc <the unit's flags> -Rpass-analysis=kernel-resource-usage -c -o /dev/null helm_hip.hip 2> before.txt   (old tree)
    hipcc <the unit's flags> -Rpass-analysis=kernel-resource-usage -c -o /dev/null helm_hip.hip 2> after.txt    (new tree)
    tools/resusage_diff.py LABEL=before.txt:after.txt [LABEL=...] --diff OUT.diff --new OUT_new.txt

Every kernel of `before` is looked up by its mangled name in `after`; its registers, scratch, occupancy, spills and LDS
size must be the same (source positions are ignored: they move when code is added above a kernel).  OUT.diff lists what
differs - empty when no existing kernel changed - and OUT_new.txt the figures of the kernels only `after` has.
Exit status 1 when OUT.diff is not empty."""
import argparse
import re
import sys

REMARK = re.compile(r"remark:\s+(.*?)\s+\[-Rpass-analysis=kernel-resource-usage\]")


def parse(path):
    kernels, cur = {}, None
    for line in open(path, errors="replace"):
        m = REMARK.search(line)
        if not m:
            continue
        text = m.group(1).strip()
        if text.startswith("Function Name:"):
            cur = text.split(":", 1)[1].strip()
            kernels[cur] = []
        elif cur is not None:
            kernels[cur].append(text)
    return kernels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("units", nargs="+", help="LABEL=before.txt:after.txt")
    ap.add_argument("--diff", required=True)
    ap.add_argument("--new", required=True)
    a = ap.parse_args()
    diff, new = [], []
    for unit in a.units:
        label, files = unit.split("=", 1)
        before, after = (parse(f) for f in files.split(":"))
        if not before or not after:
            sys.exit(f"{unit}: no kernel-resource-usage remarks found")
        for name in sorted(before):
            if name not in after:
                diff.append(f"[{label}] {name}: missing after")
            elif after[name] != before[name]:
                diff.append(f"[{label}] {name}")
                diff += [f"-    {x}" for x in before[name] if x not in after[name]]
                diff += [f"+    {x}" for x in after[name] if x not in before[name]]
        for name in sorted(after):
            if name not in before:
                new.append(f"[{label}] {name}")
                new += [f"    {x}" for x in after[name]]
        print(f"{label}: {len(before)} kernels before, {len(after)} after")
    open(a.diff, "w").write("".join(x + "\n" for x in diff))
    open(a.new, "w").write("".join(x + "\n" for x in new))
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
