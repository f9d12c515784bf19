#!/usr/bin/env python3
"""Compare the device assembly of two builds of a translation unit function by function.

    hipcc <the unit's flags> --cuda-device-only -S -o before.s helm_hip.hip   (old tree)
    hipcc <the unit's flags> --cuda-device-only -S -o after.s  helm_hip.hip   (new tree)
    tools/asm_functions_diff.py LABEL=before.s:after.s [LABEL=...]

A plain `diff` of the two files is the stronger statement and is what to use while the functions come in the same order.  The
compiler emits template instantiations in the order the host code first names them, so a change of host code alone can permute
them; then this tool says whether anything else moved.  A function is the text from its `-- Begin function <name>` line (and the
section line before it) to the next function's: code, kernel descriptor and the resource comments behind it; every function of `before` is looked
up by name in `after` and compared line by line after the labels that carry the function's ordinal (`.LBB<n>_`,
`.Lfunc_end<n>`, ...) are made order-free.  The kernels' entries of the `.amdgpu_metadata` note are compared by `.name` in
the same way.  Prints per unit the counts, whether the order is the same, and every name that differs or is missing; exit
status 1 when one does."""
import re
import sys

ORDINAL = re.compile(r"\.?\b(LBB|BB|Lfunc_begin|Lfunc_end|Ltmp|LJTI|LCPI)\d+(?=_|\b)")  # (`BB<n>_`: the loop comments)
BEGIN = re.compile(r"; -- Begin function (\S+)")
TEXT = re.compile(r"^\s*(\.text\s*$|\.section\s+\.text[.,])")
TAIL = re.compile(r"^\s*\.section\s+\.AMDGPU\.gpr_maximums")


def parse(path):
    funcs, order, meta, name, entry, in_meta, held = {}, [], {}, None, None, False, None
    for line in open(path, errors="replace"):
        line = line.rstrip()
        if in_meta:
            if line.startswith("  - "):
                entry = []
                meta[len(meta)] = entry
            elif not line.startswith("    "):
                entry = None
            if entry is not None:
                entry.append(line)
            continue
        if line.strip() == "amdhsa.kernels:":
            in_meta, name = True, None
            continue
        if TEXT.match(line):   # belongs to the function that begins on the next line, if one does
            held = line
            continue
        lines, held = ([held] if held is not None else []) + [line], None
        m = BEGIN.search(line)
        if m:
            name = m.group(1)
            order.append(name)
            funcs[name] = []
        elif TAIL.match(line):
            name = None
        if name is not None:
            # (the comment column moves with the width of the ordinal)
            funcs[name] += [re.sub(r"\s+;", " ;", ORDINAL.sub(lambda q: "." + q.group(1), x)) for x in lines]
    named = {}
    for e in meta.values():
        key = [x.split(":", 1)[1].strip() for x in e if x.strip().startswith(".name:")]
        named[key[-1] if key else str(len(named))] = e
    return funcs, order, named


def main():
    bad = 0
    for unit in sys.argv[1:]:
        label, files = unit.split("=", 1)
        (a, oa, ma), (b, ob, mb) = (parse(f) for f in files.split(":"))
        if not a or not b or not ma or not mb:
            sys.exit(f"{unit}: no functions or no metadata found")
        for what, x, y in (("functions", a, b), ("metadata entries", ma, mb)):
            differ = [n for n in x if n in y and x[n] != y[n]]
            missing = [n for n in x if n not in y]
            new = [n for n in y if n not in x]
            order = "" if what != "functions" else f" order {'the same' if oa == ob else 'differs'};"
            print(f"{label}: {len(x)} {what} before, {len(y)} after;{order} {len(differ)} differ, {len(missing)} missing, "
                  f"{len(new)} new")
            for kind, names in (("differs", differ), ("missing", missing), ("new", new)):
                for n in names:
                    print(f"  {kind}: {n}")
            bad += len(differ) + len(missing) + len(new)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
