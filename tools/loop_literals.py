#!/usr/bin/env python3
"""Static count of literal moves per loop of a kernel, from the device assembly (`python __graft_entry__.py --asm OUT.s`).

gfx950's VOP3 encoding takes no fp64 literal: every fp64 constant that is no inline constant is built by two 32-bit moves with a literal
operand (v_mov_b32 / s_mov_b32 ..., 0x...), at every use (the build runs without machine LICM). This tool counts them where they cost:
inside the loops. For the kernel whose (demangled or mangled) name contains NAME it prints, per outermost loop — LLVM's block comments
`Loop Header` / `in Loop: Header=BBn_m` delimit them; an inner loop is counted into the loop around it and listed under it ("of it") — the
number of instructions, the number of moves with a 32-bit literal operand, the distinct literals among them and the registers touched.

    python tools/loop_literals.py device.s 'k_step_duo<0, false, false>'     (name as c++filt prints it; or a mangled substring)
    python tools/loop_literals.py device.s --list                            (the kernels of the file)
"""
import re
import subprocess
import sys

LABEL = re.compile(r"^(\.LBB\d+_\d+|[A-Za-z_][\w$.]*):")
IN_LOOP = re.compile(r";\s+in Loop: Header=(BB\d+_\d+) Depth=(\d+)")
HEADER = re.compile(r";\s*=>\s*This (?:Inner )?Loop Header: Depth=(\d+)")
PARENT = re.compile(r";\s+Parent Loop (BB\d+_\d+) Depth=(\d+)")
LITERAL_MOVE = re.compile(r"^\s+([sv]_(?:mov|movk|cmov|cmovk)\w*)\s+.*[, ](0x[0-9a-fA-F]+)\s*(?:;.*)?$")
INSTR = re.compile(r"^\s+([a-z][a-z0-9_]+)\b")
REG = re.compile(r"\b([vs])(\d+)\b|\b([vs])\[(\d+):(\d+)\]")


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def kernels(lines):
    """{mangled name: (first line, last line)} of every .amdhsa kernel body: from its label to its s_endpgm-terminated .Lfunc_end"""
    starts = {}
    for k, l in enumerate(lines):
        m = re.match(r"^\s+\.type\s+([\w$.]+),@function", l)
        if m:
            starts[m.group(1)] = k
    spans = {}
    for name, k in starts.items():
        end = next((j for j in range(k, len(lines)) if lines[j].startswith(".Lfunc_end") or lines[j].lstrip().startswith(".end_amdhsa_kernel")), len(lines))
        spans[name] = (k, end)
    return spans


BLOCK = re.compile(r"^(?:\.L(BB\d+_\d+):|; %bb\.\d+:)")


def analyse(lines):
    """{loop header: counts} of one kernel body; an inner loop has its own record (`outer`: the depth-1 loop around it) and is
    counted into that outer loop's record as well"""
    def notes(k):   # a block's annotation: on its line and on the comment-only lines behind it
        j = k + 1
        while j < len(lines) and lines[j].startswith(" ") and lines[j].lstrip().startswith(";") and not lines[j].lstrip().startswith(";;"):
            j += 1
        return "\n".join(lines[k:j])
    outer_of = {}     # pass 1 (the layout may put a loop's blocks ahead of its header): inner loop header -> depth-1 header
    for k, l in enumerate(lines):
        m = BLOCK.match(l)
        if m and m.group(1):
            text = notes(k)
            if HEADER.search(text):
                top = [p for p, d in PARENT.findall(text) if d == "1"]
                outer_of[m.group(1)] = top[0] if top else m.group(1)
    new = lambda k, outer: dict(first=k + 1, insts=0, moves=0, lits=set(), v=set(), s=set(), outer=outer)
    loops, cur = {}, []
    for k, l in enumerate(lines):
        m = BLOCK.match(l)
        if m:
            text = notes(k)
            h = m.group(1) if (m.group(1) and HEADER.search(text)) else (IN_LOOP.search(text).group(1) if IN_LOOP.search(text) else None)
            cur = []
            if h is not None:
                top = outer_of.get(h, h)
                cur = [loops.setdefault(top, new(k, None))]
                if top != h:
                    cur.append(loops.setdefault(h, new(k, top)))
            continue
        if LABEL.match(l):   # any other label: outside every loop
            cur = []
        code = l.split(";")[0].rstrip()
        if not cur or not INSTR.match(code):
            continue
        mm = LITERAL_MOVE.match(code)
        for rec in cur:
            rec["insts"] += 1
            if mm:
                rec["moves"] += 1
                rec["lits"].add(mm.group(2).lower())
            for a, b, c, d, e in REG.findall(code):
                if a:
                    (rec["v"] if a == "v" else rec["s"]).add(int(b))
                else:
                    (rec["v"] if c == "v" else rec["s"]).update(range(int(d), int(e) + 1))
    return loops


def main(argv):
    if len(argv) < 2:
        print(__doc__); return 2
    lines = open(argv[0], errors="replace").read().split("\n")
    spans = kernels(lines)
    names = demangle(sorted(spans))
    if argv[1] == "--list":
        for n in sorted(spans):
            print(names[n])
        return 0
    want = argv[1]
    hits = [n for n in spans if want in n or want.replace(" ", "") in names[n].replace(" ", "")]
    # (a kernel's name also prefixes nothing else here; an exact demangled match wins over substring matches)
    exact = [n for n in hits if names[n].replace(" ", "").startswith("void" + want.replace(" ", "") + "(") or names[n].replace(" ", "").startswith(want.replace(" ", "") + "(")]
    hits = exact or hits
    if not hits:
        print("no kernel matches %r (try --list)" % want); return 1
    for n in hits:
        a, b = spans[n]
        loops = analyse(lines[a:b])
        print("%s   [lines %d-%d]" % (names[n], a + 1, b))
        print("  %-12s %8s %7s %14s %9s %6s %6s" % ("loop", "line", "insts", "literal moves", "distinct", "VGPRs", "SGPRs"))
        row = lambda h, r: print("  %-12s %8d %7d %14d %9d %6d %6d" % (h, a + r["first"], r["insts"], r["moves"], len(r["lits"]), len(r["v"]), len(r["s"])))
        for h, r in sorted(loops.items(), key=lambda kv: kv[1]["first"]):
            if r["outer"] is None:
                row(h, r)
                for hi, ri in sorted(loops.items(), key=lambda kv: kv[1]["first"]):
                    if ri["outer"] == h:
                        row("  of it " + hi[hi.index("_") + 1:], ri)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
