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
the kernels that exist in only one; exit status 1 if any common kernel differs.

    python tools/isa_compare.py --prologue FILE.s substring

prints, for every kernel of one file whose name contains the substring, its register counts, scratch size and occupancy
(the file's metadata), and for every s_barrier that is followed by a matrix instruction before the next barrier -- the
start of a polyphase round -- what lies between the two: instructions, integer-division sequences (v_rcp_iflag), loads
issued, and every s_waitcnt.

    python tools/isa_compare.py --meta A.s B.s

prints one line per kernel of A with the register counts, ScratchSize and occupancy (waves per SIMD) of both files, and marks
(<<<<) the kernels whose scratch is not zero in B or whose occupancy changed.

    python tools/isa_compare.py --tile-loop FILE.s substring

prints, for every kernel whose name contains the substring, the skeleton of each polyphase round -- from the barrier in front of
the round's first matrix instruction to its last matrix instruction and the store behind it: labels, branches, every s_waitcnt,
vector-memory loads and stores, the count of matrix instructions in between -- and the number of s_waitcnt vmcnt(0) inside."""
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


def prologue(path, sub):
    text = open(path).read()
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_count:\s+(\d+)\n(?:.*\n)*?"
                         r"\s+\.vgpr_count:\s+(\d+)", text):
        meta[m.group(1)] = m.groups()[1:]
    for name, body in sorted(functions(path).items()):
        if sub not in name:
            continue
        scratch, sgpr, vgpr = meta.get(name, ("?", "?", "?"))
        m = re.search(re.escape(name) + r":.*?; Occupancy: (\d+)", text, re.S)
        print("%s\n  vgpr %s sgpr %s scratch %s occupancy (waves per SIMD) %s, %d instructions" %
              (name, vgpr, sgpr, scratch, m.group(1) if m else "?", len(body)))
        bars = [i for i, s in enumerate(body) if s.startswith("s_barrier")] + [len(body)]
        for b, nb in zip(bars, bars[1:]):
            first = next((i for i in range(b, nb) if body[i].startswith("v_mfma")), None)
            if first is None:
                continue
            part = body[b + 1:first]
            loads = [s.split()[0] for s in part if re.match(r"(s_load|s_buffer_load|global_load|buffer_load|flat_load)", s)]
            print("  barrier at %d -> first matrix instruction at %d: %d instructions, %d v_rcp_iflag, loads issued %s, waits %s" %
                  (b, first, len(part), sum(s.startswith("v_rcp_iflag") for s in part), loads or "none",
                   [s.replace("s_waitcnt ", "") for s in part if s.startswith("s_waitcnt")]))
    return 0


def meta(path):
    out, name = {}, None
    for line in open(path):
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and not line.startswith(".L"):
            name = m.group(1)
        m = re.match(r"^; (NumVgprs|TotalNumSgprs|ScratchSize|Occupancy): (\d+)", line)
        if m and name:
            out.setdefault(name, {})[m.group(1)] = int(m.group(2))
    return out


def meta_compare(pa, pb):
    a, b = meta(pa), meta(pb)
    bad = 0
    for k in sorted(a):
        x, y = a[k], b.get(k)
        if y is None:
            print("only in A: %s" % k)
            continue
        flag = "" if y["ScratchSize"] == 0 and y["Occupancy"] == x["Occupancy"] else "  <<<<"
        bad += bool(flag)
        print("%-78s vgpr %3d -> %3d  sgpr %3d -> %3d  scratch %d -> %d  occupancy %d -> %d%s" %
              (k, x["NumVgprs"], y["NumVgprs"], x["TotalNumSgprs"], y["TotalNumSgprs"], x["ScratchSize"], y["ScratchSize"],
               x["Occupancy"], y["Occupancy"], flag))
    print("%d kernels, %d with scratch in B or another occupancy" % (len(a), bad))
    return 1 if bad else 0


def tile_loop(path, sub):
    keep = re.compile(r"(\.L\d+:|s_waitcnt|s_cbranch|s_branch|buffer_store|global_load|global_store|buffer_load|s_barrier|v_mul_hi_u32|v_cvt_i32_f64)")
    for name, body in sorted(functions(path).items()):
        if sub not in name:
            continue
        print(name)
        bars = [i for i, s in enumerate(body) if s.startswith("s_barrier")] + [len(body)]
        rnd = 0
        for b, nb in zip(bars, bars[1:]):
            mf = [i for i in range(b, nb) if body[i].startswith("v_mfma")]
            if not mf:
                continue
            rnd += 1
            end = next((i for i in range(mf[-1], nb) if "store" in body[i]), mf[-1])
            print("  round %d: instructions %d .. %d, %d matrix instructions" % (rnd, b, end, len(mf)))
            n = 0
            for i in range(b, end + 1):
                if body[i].startswith("v_mfma"):
                    n += 1
                    continue
                if keep.match(body[i]):
                    if n:
                        print("      ... %d v_mfma ..." % n)
                        n = 0
                    print("    %5d  %s" % (i, body[i]))
            inside = [i for i in range(mf[0], mf[-1]) if body[i].startswith("s_waitcnt") and "vmcnt(0)" in body[i]]
            print("  round %d: s_waitcnt vmcnt(0) between the first and the last matrix instruction: %d" % (rnd, len(inside)))
    return 0


def main():
    if sys.argv[1] == "--prologue":
        return prologue(sys.argv[2], sys.argv[3])
    if sys.argv[1] == "--meta":
        return meta_compare(sys.argv[2], sys.argv[3])
    if sys.argv[1] == "--tile-loop":
        return tile_loop(sys.argv[2], sys.argv[3])
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
