#!/usr/bin/env python3
"""Static instruction mix per loop of a kernel, from the device assembly (`python __graft_entry__.py --asm OUT.s`).

The wave-pair stepper is bound by what a SIMD can issue (docs/design/roofline.md "Round 5"): every instruction of either wave costs a
slot, whatever it does. tools/loop_literals.py counts one kind of overhead, the literal moves; this tool prints the whole mix, so that
"what is not arithmetic" has a number per class before and after a change. For the kernel whose (demangled or mangled) name contains
NAME it prints, per OUTERMOST loop (inner loops are counted into the loop around them; the loop finder is loop_literals.py's), the
instructions by opcode class:

    fp64 arithmetic | compare / select / min-max | literal moves | register-to-register moves (32- and 64-bit) | lane moves |
    s_nop behind a compare, other s_nop | s_waitcnt | LDS read / write | vector memory | scalar memory | branches | other SALU | other VALU

"s_nop behind a compare": the instruction in front of it (other s_nop skipped) is a v_cmp*. A report over opcode classes of a loop's
static body: a body is not a path (rare branches are counted like the common one), and it gates nothing.

    python tools/loop_mix.py device.s 'k_step_duo<0, false, false>'
    python tools/loop_mix.py device.s --list
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_literals as L  # noqa: E402

CLASSES = ["fp64 arithmetic", "compare / select / min-max", "literal moves", "reg-reg moves, 32-bit", "reg-reg moves, 64-bit", "lane moves",
           "s_nop behind a compare", "s_nop, other", "s_waitcnt", "LDS read", "LDS write", "vector memory", "scalar memory", "branches",
           "other SALU", "other VALU"]
FP64 = re.compile(r"^v_(fma|fmac|mul|add|rcp|rsq|sqrt|ldexp|frexp_mant|frexp_exp_i32|trig_preop|fract|floor|ceil|trunc|rndne|div_scale|div_fmas|div_fixup)_f64")
CMPSEL = re.compile(r"^v_(cmp|cmpx|cndmask|max|min|med3)")
REGREG = re.compile(r"^\s+[sv]_mov_b(32|64)(?:_e32|_e64)?\s+([sv](?:\d+|\[\d+:\d+\])|vcc|exec)\s*,\s*([sv](?:\d+|\[\d+:\d+\])|vcc|exec)\s*$")


def classify(op, code, prev_op):
    if L.LITERAL_MOVE.match(code):
        return "literal moves"
    m = REGREG.match(code)
    if m:
        return "reg-reg moves, %s-bit" % m.group(1)
    if op in ("v_readlane_b32", "v_writelane_b32", "v_readfirstlane_b32") or op.startswith("v_accvgpr") or op.startswith("ds_bpermute") or op.startswith("ds_permute"):
        return "lane moves"
    if op == "s_nop":
        return "s_nop behind a compare" if prev_op.startswith("v_cmp") else "s_nop, other"
    if op == "s_waitcnt":
        return "s_waitcnt"
    if op.startswith("ds_read") or op.startswith("ds_load"):
        return "LDS read"
    if op.startswith("ds_"):
        return "LDS write"
    if op.split("_")[0] in ("global", "flat", "buffer", "scratch"):
        return "vector memory"
    if re.match(r"^s_(load|buffer_load)", op):
        return "scalar memory"
    if op.startswith("s_cbranch") or op in ("s_branch", "s_setpc_b64", "s_swappc_b64", "s_endpgm"):
        return "branches"
    if FP64.match(op):
        return "fp64 arithmetic"
    if CMPSEL.match(op):
        return "compare / select / min-max"
    return "other SALU" if op.startswith("s_") else "other VALU"


def mix(lines):
    """{outermost loop header: (first line, {class: count})} of one kernel body"""
    def notes(k):
        j = k + 1
        while j < len(lines) and lines[j].startswith(" ") and lines[j].lstrip().startswith(";") and not lines[j].lstrip().startswith(";;"):
            j += 1
        return "\n".join(lines[k:j])
    outer_of = {}
    for k, l in enumerate(lines):
        m = L.BLOCK.match(l)
        if m and m.group(1):
            text = notes(k)
            if L.HEADER.search(text):
                top = [p for p, d in L.PARENT.findall(text) if d == "1"]
                outer_of[m.group(1)] = top[0] if top else m.group(1)
    loops, cur, prev_op = {}, None, ""
    for k, l in enumerate(lines):
        m = L.BLOCK.match(l)
        if m:
            text = notes(k)
            h = m.group(1) if (m.group(1) and L.HEADER.search(text)) else (L.IN_LOOP.search(text).group(1) if L.IN_LOOP.search(text) else None)
            cur = None
            if h is not None:
                cur = loops.setdefault(outer_of.get(h, h), (k + 1, dict.fromkeys(CLASSES, 0)))
            continue
        if L.LABEL.match(l):
            cur = None
        code = l.split(";")[0].rstrip()
        mm = L.INSTR.match(code)
        if not mm:
            continue
        op = mm.group(1)
        if cur is not None:
            cur[1][classify(op, code, prev_op)] += 1
        if op != "s_nop":   # (a run of s_nop behind a compare is one wait)
            prev_op = op
    return loops


def main(argv):
    if len(argv) < 2:
        print(__doc__); return 2
    lines = open(argv[0], errors="replace").read().split("\n")
    spans = L.kernels(lines)
    names = L.demangle(sorted(spans))
    if argv[1] == "--list":
        for n in sorted(spans):
            print(names[n])
        return 0
    want = argv[1].replace(" ", "")
    hits = [n for n in spans if argv[1] in n or want in names[n].replace(" ", "")]
    exact = [n for n in hits if names[n].replace(" ", "").startswith("void" + want + "(") or names[n].replace(" ", "").startswith(want + "(")]
    hits = exact or hits
    if not hits:
        print("no kernel matches %r (try --list)" % argv[1]); return 1
    for n in hits:
        a, b = spans[n]
        loops = sorted(mix(lines[a:b]).items(), key=lambda kv: kv[1][0])
        print("%s   [lines %d-%d]" % (names[n], a + 1, b))
        print("  %-28s" % "class" + "".join(" %10s" % h for h, _ in loops))
        for c in CLASSES:
            print("  %-28s" % c + "".join(" %10d" % r[1][c] for _, r in loops))
        print("  %-28s" % "all" + "".join(" %10d" % sum(r[1].values()) for _, r in loops))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
