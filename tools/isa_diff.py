"""Kernel-by-kernel comparison of the gfx950 assembly of two sets of csrc/*.hip files (or kept .s files).

For moving kernels between translation units: every .amdhsa_kernel symbol of the OLD inputs has to come out of the NEW
inputs exactly once with the same instructions.  A kernel's body is the text from its symbol's label to its .Lfunc_end,
without comments and directives, the .LBB block labels renumbered in order of appearance (their numbers count the
functions of a unit, so they move with the kernel's place in it).  Only text is compared.

usage: python tools/isa_diff.py OLD [OLD ...] -- NEW [NEW ...]
       each input a .hip file (compiled device-only with the Makefile's flags, tools/isa_counts.py) or a kept .s file
prints one line per symbol (SAME / DIFF with both lengths in instructions), the symbols on one side only, the symbols
defined more than once on a side and a final count; exit status 0 only if every symbol is once on each side and the same.
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_counts import assemble, demangle  # noqa: E402


def bodies(asm):
    """-> {kernel symbol: [its bodies, one per definition]} for the .amdhsa_kernel symbols of `asm`; a body is a list
    of lines (instructions and block labels)."""
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    res, cur, labels = {}, None, None
    for raw in asm.split("\n"):
        s = " ".join(raw.split(";")[0].split())
        if not s:
            continue
        m = re.fullmatch(r"(\S+):", s)
        if m and m.group(1) in kernels:
            cur, labels = [], {}
            res.setdefault(m.group(1), []).append(cur)
            continue
        if cur is None:
            continue
        if m and (s.startswith(".Lfunc_end") or not s.startswith(".")):  # the kernel's end, or another function
            cur = None
            continue
        if s.startswith(".") and not m:  # a directive
            continue
        cur.append(re.sub(r"\.LBB\d+_\d+", lambda b: labels.setdefault(b.group(0), ".LBB%d" % len(labels)), s))
    return res


def compare(old, new):
    """-> (lines to print, ok) for two {symbol: [bodies]} maps."""
    out, same, diff = [], 0, 0
    names = demangle(sorted(set(old) | set(new)))
    nice = {k: re.sub(r"^void |\(anonymous namespace\)::|\(.*\)$", "", v) for k, v in names.items()}
    both = sorted(set(old) & set(new), key=lambda k: nice[k])
    for sym in both:
        a, b = old[sym][0], new[sym][0]
        if a == b:
            same += 1
        else:
            diff += 1
        out.append(f"{'SAME' if a == b else 'DIFF'} {len(a):>6} {len(b):>6}  {nice[sym]}")
    only = [(side, sym) for side, here, there in (("old", old, new), ("new", new, old)) for sym in sorted(here) if sym not in there]
    out += [f"ONLY {side}  {nice[sym]}" for side, sym in only]
    twice = [(side, sym, len(m[sym])) for side, m in (("old", old), ("new", new)) for sym in sorted(m) if len(m[sym]) > 1]
    out += [f"TWICE {side} x{n}  {nice[sym]}" for side, sym, n in twice]
    out.append(f"{len(old)} old symbols, {len(new)} new: {same} same, {diff} differ, {len(only)} on one side only, "
               f"{len(twice)} defined more than once")
    return out, not (diff or only or twice)


def load(paths):
    res = {}
    for p in paths:
        asm = open(p).read() if p.endswith(".s") else assemble(p)
        for sym, defs in bodies(asm).items():
            res.setdefault(sym, []).extend(defs)
    return res


def main():
    args = sys.argv[1:]
    if "--" not in args or not args[:args.index("--")] or not args[args.index("--") + 1:]:
        print(__doc__)
        return 2
    i = args.index("--")
    lines, ok = compare(load(args[:i]), load(args[i + 1:]))
    print("\n".join(lines))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
