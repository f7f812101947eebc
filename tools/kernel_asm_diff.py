#!/usr/bin/env python3
"""Compare two builds' device assembly kernel by kernel (dev tool, no GPU).

    hipcc ... --cuda-device-only -S x.hip -o x.s      (or `make asm`: build/asm/*.s)
    tools/kernel_asm_diff.py --old old/*.s --new new/*.s

Each side is any number of device .s files; a kernel may sit in a different
file on the two sides.  A kernel is what an `.amdhsa_kernel NAME` block names;
its code runs from the `NAME:` label to `.Lfunc_end`.  Comments are dropped
and local labels (.LBB<fn>_<n>, ...: numbered by the function's position in its
file) are renumbered in order of appearance, then the instruction lists and the
`.amdhsa_` resource lines (registers, LDS, scratch) are compared as text.
Prints the kernels on one side only, the kernels that differ, and totals; exit
status 1 when anything differs."""
import argparse
import re
import sys

LOCAL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")


def kernels(paths):
    """{name: (instructions, amdhsa lines)}, and the names seen more than once"""
    out, dup = {}, []
    for path in paths:
        lines = open(path).read().split("\n")
        names = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
        for name in names:
            body, meta, ids = [], [], {}
            i = next(n for n, l in enumerate(lines) if l.startswith(name + ":"))
            for l in lines[i + 1:]:
                l = l.split(";")[0].strip()
                if l.startswith(".Lfunc_end"):
                    break
                if l:
                    body.append(LOCAL.sub(lambda m: ids.setdefault(m.group(0), ".L%d" % len(ids)), l))
            j = next(n for n, l in enumerate(lines) if l.strip() == ".amdhsa_kernel " + name)
            while lines[j].strip() != ".end_amdhsa_kernel":
                j += 1
                meta.append(lines[j].strip())
            if name in out:
                dup.append(name)
            out[name] = (body, meta)
    return out, dup


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    args = ap.parse_args()
    (old, dup_o), (new, dup_n) = kernels(args.old), kernels(args.new)
    only_o, only_n = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    code = [k for k in sorted(set(old) & set(new)) if old[k][0] != new[k][0]]
    meta = [k for k in sorted(set(old) & set(new)) if old[k][1] != new[k][1]]
    for title, names in (("only in old", only_o), ("only in new", only_n),
                         ("more than once in old", dup_o), ("more than once in new", dup_n),
                         ("instructions differ", code), ("resource lines differ", meta)):
        for k in names:
            extra = " (%d -> %d lines)" % (len(old[k][0]), len(new[k][0])) if names is code else ""
            print("%s: %s%s" % (title, k, extra))
    # (the lists compared also hold the labels and directives between the instructions)
    n_i = lambda d: sum(not (l.startswith(".") or l.endswith(":")) for v in d.values() for l in v[0])
    print("kernels: old %d, new %d; instructions: old %d, new %d; only old %d, only new %d, "
          "repeated %d, code differs %d, resources differ %d"
          % (len(old), len(new), n_i(old), n_i(new), len(only_o), len(only_n),
             len(dup_o) + len(dup_n), len(code), len(meta)))
    return 1 if only_o or only_n or dup_o or dup_n or code or meta else 0


if __name__ == "__main__":
    sys.exit(main())
