#!/usr/bin/env python3
"""Compare the instruction streams of the kernels two builds have in common.

    make -C foo_dsp_resampler_amd/csrc OBJDIR=../_build_a EXTRA=-save-temps=obj OUT=../_build_a/lib.so      (build A)
    ... the same for build B from the other tree ...
    python tools/isa_compare.py A/fused_fast-hip-amdgcn-amd-amdhsa-gfx950.s B/fused_fast-hip-amdgcn-amd-amdhsa-gfx950.s [substring ...]

Every function of the two gfx950 assembly files (hipcc -save-temps) is cut out between its label and its .Lfunc_end,
comments and directives are dropped and basic-block labels are renumbered per function (their numbers carry the function's
index in the file, which moves when instances are added).  What is left is the instruction stream with every register,
immediate and kernel-argument offset in it, so "identical" here is stricter than "allowing for kernel-argument offsets".
Prints one line per kernel present in both files (optionally only those whose demangled-ish name contains a substring) and
the kernels that exist in only one; exit status 1 if any common kernel differs."""
import re
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and not line.startswith(".L") and name is None:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        s = line.split(";")[0].strip()
        if not s or (s.startswith(".") and not s.startswith(".LBB")):
            continue
        body.append(s)
    for body in out.values():
        ids = {}
        for i, s in enumerate(body):
            body[i] = re.sub(r"\.LBB\d+_(\d+)", lambda m: ".L%d" % ids.setdefault(m.group(1), len(ids)), s)
    return out


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    subs = sys.argv[3:]
    bad = 0
    for k in sorted(set(a) & set(b)):
        if subs and not any(s in k for s in subs):
            continue
        same = a[k] == b[k]
        bad += not same
        print("%s %6d %6d  %s" % ("same" if same else "DIFF", len(a[k]), len(b[k]), k))
    for k in sorted(set(a) ^ set(b)):
        if subs and not any(s in k for s in subs):
            continue
        print("only in %s: %s" % ("A" if k in a else "B", k))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
