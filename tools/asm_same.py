#!/usr/bin/env python3
"""Is it the same device code?   python tools/asm_same.py A.s B.s
A.s, B.s: two outputs of `python __graft_entry__.py --asm PATH` (say, of the parent's checkout and of this tree). Per kernel, demangled: the
instruction count, registers, scratch and LDS of the metadata, and whether the instruction text is the same once comments are stripped. Exit
status 1 if a kernel differs, in text or in a resource, or is in one file only. Text only: labels count, less the function's ordinal in
compiler-made ones (.LBB34_7 -> .LBB_7: it shifts when a kernel is added elsewhere); directives (.p2align, .section, ...) do not."""
import re
import subprocess
import sys

FIELDS = (("vgpr", "vgpr_count"), ("sgpr", "sgpr_count"), ("scratch", "private_segment_fixed_size"), ("lds", "group_segment_fixed_size"))
ROW = "%-64s %15s  %-11s %-11s %-9s %-13s %s"


def kernels(path):
    """{symbol: (instruction count, {resource: value}, normalised text)}"""
    s = open(path).read()
    out = {}
    for block in re.split(r"\n  - ", s[s.index("amdhsa.kernels:"):]):
        name = re.search(r"\.name: +(\S+)", block)
        if not name:
            continue
        sym = name.group(1)
        res = {k: int(re.search(r"\.%s: +(\d+)" % f, block).group(1)) for k, f in FIELDS}
        body = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end\d+:" % re.escape(sym), s, re.S | re.M).group(1)
        lines = [" ".join(line.split(";", 1)[0].split()) for line in body.split("\n")]
        lines = [re.sub(r"\.LBB\d+_", ".LBB_", l) for l in lines if l and (not l.startswith(".") or l.endswith(":"))]
        out[sym] = (sum(not l.endswith(":") for l in lines), res, "\n".join(lines))
    return out


def main(a_path, b_path):
    a, b = kernels(a_path), kernels(b_path)
    names = sorted(set(a) | set(b))
    try:
        dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    except (OSError, subprocess.CalledProcessError):
        dem = names
    dem = {n: re.sub(r"\((?:[^()]|\([^()]*\))*\)$", "", d) for n, d in zip(names, dem)}   # (the argument list says nothing a row needs)
    pair = lambda x, y: str(x) if x == y else "%s->%s" % (x, y)
    bad = 0
    print(ROW % ("kernel", "instructions", "vgpr", "sgpr", "scratch", "lds", "text"))
    for n in sorted(names, key=dem.get):
        if n not in a or n not in b:
            print("%-64s only in %s" % (dem[n][:64], b_path if n in b else a_path))
            bad += 1
            continue
        (ia, ra, ta), (ib, rb, tb) = a[n], b[n]
        bad += not (ta == tb and ra == rb)
        print(ROW % (dem[n][:64], pair(ia, ib), *(pair(ra[k], rb[k]) for k, _ in FIELDS), "identical" if ta == tb else "DIFFERS"))
    print("%d kernels, %d differ or are missing" % (len(names), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]) if len(sys.argv) == 3 else __doc__)
