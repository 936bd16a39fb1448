#!/usr/bin/env python3
"""Compare gfx950 assembly kernel by kernel (a refactor's check: same code).

  hipcc <the Makefile's flags> --cuda-device-only -S unit.hip -o unit.s
  python scripts/isa_diff.py --old old.s --new new_a.s new_b.s [--show]

Each side is one or more .s files (a unit that was split compares as the
union of its parts). A kernel is the text from its mangled-name label to its
.Lfunc_end; comments are stripped and the function-numbered local labels
(.LBB<n>_<m>, .Ltmp<n>) are normalised, since <n> only counts the functions
of the unit. Prints the kernels present on one side only, and each
kernel whose text differs with both sides' resource lines (.vgpr_count,
.sgpr_count, .agpr_count, .group_segment_fixed_size,
.private_segment_fixed_size from the metadata); --show adds a unified diff.
Exit status 0 when every kernel is identical, 1 otherwise.
"""
import argparse
import difflib
import re
import sys

RES = ("vgpr_count", "sgpr_count", "agpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(path):
    """{name: (normalised lines, {resource: value})} of one assembly file."""
    lines = open(path).read().splitlines()
    meta = {}
    cur = {}
    for ln in lines:  # amdhsa.kernels metadata: a block per kernel, keys sorted, .agpr_count first
        m = re.match(r"\s+(- )?\.(\w+):\s+(\S+)\s*$", ln)
        if not m:
            continue
        if m.group(1) and m.group(2) == "agpr_count":
            cur = {}
        if m.group(2) in RES:
            cur[m.group(2)] = m.group(3)
        elif m.group(2) == "name" and "agpr_count" in cur:
            meta[m.group(3)] = cur  # (the dict fills on: the counts follow the name)
    out = {}
    i = 0
    while i < len(lines):
        m = re.match(r"(_Z\w+):\s*(;.*)?$", lines[i])
        if not m or m.group(1) not in meta:
            i += 1
            continue
        name, body = m.group(1), []
        i += 1
        while i < len(lines) and not re.match(r"\.Lfunc_end\d+:", lines[i]):
            ln = re.sub(r"\s*;.*$", "", lines[i]).rstrip()
            ln = re.sub(r"\.LBB\d+_", ".LBB_", ln)
            ln = re.sub(r"\.Ltmp\d+", ".Ltmp", ln)
            if ln:
                body.append(ln)
            i += 1
        out[name] = (body, {k: meta[name].get(k, "?") for k in RES})
    return out


def side(paths):
    ks = {}
    for p in paths:
        for n, v in kernels(p).items():
            if n in ks:
                sys.exit(f"{n} is defined twice in {paths}")
            ks[n] = v
    return ks


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--show", action="store_true", help="print a unified diff of each kernel that differs")
    a = ap.parse_args()
    old, new = side(a.old), side(a.new)
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    differ = [n for n in sorted(set(old) & set(new)) if old[n][0] != new[n][0]]
    res_moved = [n for n in sorted(set(old) & set(new)) if old[n][1] != new[n][1]]
    print(f"kernels: old {len(old)}, new {len(new)}, identical {len(set(old) & set(new)) - len(differ)}, "
          f"differing {len(differ)}, only old {len(only_old)}, only new {len(only_new)}")
    for n in only_old:
        print(f"only old: {n}")
    for n in only_new:
        print(f"only new: {n}")
    for n in sorted(set(differ) | set(res_moved)):
        print(f"differs: {n}")
        print("  old " + " ".join(f".{k} {v}" for k, v in old[n][1].items()))
        print("  new " + " ".join(f".{k} {v}" for k, v in new[n][1].items()))
        if a.show:
            for ln in difflib.unified_diff(old[n][0], new[n][0], "old", "new", lineterm="", n=2):
                print("    " + ln)
    return 1 if (only_old or only_new or differ or res_moved) else 0


if __name__ == "__main__":
    sys.exit(main())
