"""Is every function of one gfx950 assembly the same in another?

    python tools/isa_same.py --old OLD/*.s --new NEW/*.s [--rename OLD_SYMBOL=NEW_SYMBOL ...]

Both sides come from `make -C iterative_cleaner_amd/csrc asm` (of two trees);
either side may be any number of units, so code may move between files (a
kernel of the host file: `make ic_session.s`).  --rename compares a symbol of
the old side under another name (a kernel that left an anonymous namespace):
the name is replaced in its own text, nothing else about it is excused.
Each side is split by function symbol (kernels and non-inlined device
functions); comments and .loc / .file / .cfi lines are dropped and the function
index in .LBB<n>_ / .Ltmp<n> / .Lfunc_end<n> labels is normalised, since it
only counts the functions before this one in its file.  Per symbol the
instruction text and the .amdhsa_kernel descriptor block are compared.  One
line per symbol; exit status 1 if a symbol differs, is missing on a side or is
defined twice on a side."""
from __future__ import annotations

import argparse
import re
import sys

DROP = re.compile(r"^\.(loc|file|cfi_\w+)\b")
LABEL = re.compile(r"\.L(BB|tmp|func_end|func_begin)\d+")


def functions(paths):
    """{symbol: (text lines, descriptor lines)}, plus the symbols seen twice"""
    out, twice = {}, set()
    for path in paths:
        sym, part, body, desc = None, None, [], []
        for raw in open(path):
            s = raw.split(";")[0].strip()
            m = re.match(r"^\.type\s+(\S+),@function", s)
            if m:
                sym, part, body, desc = m.group(1), "text", [], []
                continue
            if sym is None or not s or DROP.match(s):
                continue
            if s.startswith(".amdhsa_kernel "):
                part = "desc"
            elif s.startswith(".Lfunc_end"):
                if sym in out:
                    twice.add(sym)
                out[sym] = (body, desc)
                sym = None
            elif s == ".end_amdhsa_kernel":
                part = None
            elif part == "text" and not s.startswith((".section", ".p2align", ".text")):
                body.append(LABEL.sub(lambda m: ".L" + m.group(1) + "#", s))
            elif part == "desc":
                desc.append(s)
    return out, twice


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    a = ap.parse_args()
    (old, otw), (new, ntw) = functions(a.old), functions(a.new)
    for was, now in (r.split("=", 1) for r in a.rename):
        if was not in old or now in old:
            sys.exit("--rename %s=%s: %s" % (was, now, "not on the old side" if was not in old else "new name taken"))
        body, desc = old.pop(was)
        old[now] = ([s.replace(was, now) for s in body], desc)
        if was in otw:
            otw.add(now)
    bad = 0
    for sym in sorted(set(old) | set(new)):
        kind = "kernel" if (old.get(sym) or new.get(sym))[1] else "function"
        if sym not in old or sym not in new:
            verdict = "missing in " + ("old" if sym not in old else "new")
        elif sym in otw or sym in ntw:
            verdict = "defined twice"
        elif old[sym][0] != new[sym][0]:
            verdict = "text differs (%d -> %d lines)" % (len(old[sym][0]), len(new[sym][0]))
        elif old[sym][1] != new[sym][1]:
            verdict = "descriptor differs: " + "; ".join(sorted(set(new[sym][1]) - set(old[sym][1])))
        else:
            verdict = "same"
        bad += verdict != "same"
        print("%-8s %-14s %s" % (kind, verdict, sym))
    nk = sum(1 for v in new.values() if v[1])
    print("%d kernels, %d functions, %d not the same" % (nk, len(new) - nk, bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
