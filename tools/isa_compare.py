#!/usr/bin/env python3
"""tools/isa_compare.py OLD NEW [--allow REGEX] — are two builds' gfx950 device functions the same, instruction for instruction?

OLD and NEW are libraries / object files (dumped with tools/isa_dump.py) or directories isa_dump.py already wrote.  Functions are paired by
name and compared with the pc-relative literals masked (the `s_add_u32` / `s_addc_u32` after an `s_getpc_b64`, into an SGPR pair or into
vcc: they move whenever the functions of a unit sit in another order or gain a neighbour, no instruction does) and the `s_nop` padding
after a function's last instruction dropped (it depends on what the unit places next).  Prints the functions that exist on one side only and those whose bodies
differ; exits 1 if any of them does not match --allow (a regular expression over the mangled name: the functions a change is MEANT to
touch, e.g. the ANIM kernel variants).  This is how "static scenes pay nothing" is shown at build time for a change to shared walk code:
build the parent commit, build the branch, compare.  Build-time analysis only; nothing is executed on a device.

compare(old_dir, new_dir) returns (only_old, only_new, differing) for callers that dumped the functions themselves."""
import argparse, os, re, sys, tempfile

import isa_dump

_LITERAL = re.compile(r"(s_add_u32|s_addc_u32) (s\d+|vcc_lo|vcc_hi), (s\d+|vcc_lo|vcc_hi), (0x[0-9a-f]+|-?\d+)")
# after a function's last instruction: alignment for whatever the unit places next (the disassembler prints a long run's tail as `...`)
_PADDING = re.compile(r"(\s*(s_nop \d+|\.\.\.))+\s*\Z")


def normalised(path):
    return _PADDING.sub("\n", _LITERAL.sub(r"\1 \2, \3, LIT", open(path).read()))


def compare(old_dir, new_dir):
    a, b = set(os.listdir(old_dir)), set(os.listdir(new_dir))
    differing = [f for f in sorted(a & b) if normalised(os.path.join(old_dir, f)) != normalised(os.path.join(new_dir, f))]
    strip = lambda names: [n[:-2] if n.endswith(".s") else n for n in names]
    return strip(sorted(a - b)), strip(sorted(b - a)), strip(differing)


def dumped(path, td, tag):
    if os.path.isdir(path):
        return path
    out = os.path.join(td, tag)
    isa_dump.main(path, out)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--allow", default=None, help="regular expression: functions that may differ or exist on one side only")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as td:
        only_old, only_new, differing = compare(dumped(a.old, td, "old"), dumped(a.new, td, "new"))
    ok = lambda n: a.allow is not None and re.search(a.allow, n) is not None
    bad = 0
    for title, names in (("only in OLD", only_old), ("only in NEW", only_new), ("bodies differ", differing)):
        print("%s: %d" % (title, len(names)))
        for n in names:
            print("  %s%s" % (n, "" if ok(n) else "   <-- not allowed"))
            bad += not ok(n)
    print("%d function(s) outside --allow" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
