"""The packed meter passes (RRX_tracks_true_peak_packed_device + RRX_tracks_loudness_packed_device: a library measured as it is
stored) against what the same scan costs through the row forms.

Workload: 64 ragged stereo tracks with the lengths of tools/perf_tracks.py (2 to 7 minutes at 44.1 kHz, from the printed LCG
seed), laid end to end in each of the four source formats -- float32, S16, packed S24, S32 -- with LCG noise for samples.  Timed,
per format:

  (a) packed   tracks_true_peak_packed_device + tracks_loudness_packed_device on the packed source
  (b) rows     tracks_true_peak_device + tracks_loudness_device on float32 rows [64, longest, 2] that hold the same tracks.  These
               are the row kernels as they were before the packed forms existed: their instruction streams did not move
               (profiles/scan_isa_compare.log)
  (c) build    the torch sequence that makes those rows from the source -- zeros, then per track rows[t, :n] = source[a:b] scaled
               to float32 -- which is what a caller without the packed calls does first

HIP events, `--warmup` calls and then `--steps` calls per candidate, `--rounds` rounds interleaved (a, b, c, a, b, c, ...), the
median of the rounds, as in tools/perf_true_peak.py.  The timed calls accumulate into the same result tensors, so from the second
call on no peak rises.  Peak memory is torch's max_memory_allocated over one (a) and over one (c) + (b), counted from the bytes
of the source (which both need).  The results of (a) and (b) are compared: equal bits for float32, S16 and S24, whose float32
rows are exact; S32 rows are rounded to float32, so there the difference is reported instead.

One JSON line per format, appended to --out (default profiles/scan_perf.jsonl) and printed:

  {"format", "seed", "tracks", "nch", "frames_total", "frames_longest", "source_bytes", "packed_ms", "packed_ms_rounds",
   "true_peak_ms", "loudness_ms": the two passes of (a) on their own, "rows_ms", "rows_ms_rounds", "build_rows_ms",
   "build_rows_ms_rounds", "ratio_to_rows": packed_ms / rows_ms, "speedup_vs_build_and_rows", "packed_peak_bytes",
   "rows_peak_bytes", "equal_bits", "max_rel_diff", "steps", "warmup"}; the s24 line also has "s24_form", the value of --s24-form: a
   label for the library that was measured ("dword": the product; "bytes": a build whose S24 loudness pass takes the generic kernel)

Exit status 1 if (a) is more than 10 % slower than (b) in a format.

  python tools/perf_scan.py [--formats f32,s16,s24,s32] [--seed 20240229] [--tracks 64] [--steps 5] [--warmup 2] [--rounds 3] [--s24-form dword] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import foo_dsp_resampler_amd as F  # noqa: E402
from perf_finish import timed  # noqa: E402
from perf_tracks import FS, NCH, lengths  # noqa: E402

BITS = {"s16": 15, "s24": 23, "s32": 31}


def make_source(fmt, total, seed):
    """LCG noise at about -12 dBFS as the format stores it, and a function that gives frames [a, b) as float32"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    if fmt == "f32":
        src = (torch.rand((total, NCH), generator=gen, device="cuda") - 0.5) * 0.5
        return src, lambda a, b: src[a:b]
    bits = BITS[fmt]
    ints = torch.randint(-(1 << (bits - 2)), 1 << (bits - 2), (total, NCH), generator=gen, device="cuda", dtype=torch.int32)
    if fmt == "s16":
        src = ints.to(torch.int16)
        return src, lambda a, b: src[a:b].float() * 2.0 ** -15
    if fmt == "s32":
        return ints, lambda a, b: ints[a:b].float() * 2.0 ** -31
    src = torch.stack([ints & 0xFF, (ints >> 8) & 0xFF, (ints >> 16) & 0xFF], dim=-1).to(torch.uint8).view(total, NCH * 3).contiguous()
    del ints

    def frames(a, b):
        p = src[a:b].view(b - a, NCH, 3).to(torch.int32)
        return (((p[..., 0] | (p[..., 1] << 8) | (p[..., 2] << 16)) << 8) >> 8).float() * 2.0 ** -23
    return src, frames


def one_format(fmt, lens, seed, steps, warmup, rounds):
    stream = torch.cuda.current_stream()
    rate, hop = FS, FS // 10
    plan = F.packed_plan(lens)
    table = plan.array()
    table[:, 4] = table[:, 1]  # the same entries describe rows that hold the tracks from frame 0 on
    tab = torch.from_numpy(table.view("int64")).cuda()
    n, longest, total = len(lens), max(lens), sum(lens)
    src, frames = make_source(fmt, total, seed)
    torch.cuda.synchronize()
    source_bytes = src.numel() * src.element_size()

    def build_rows():
        rows = torch.zeros((n, longest, NCH), dtype=torch.float32, device="cuda")
        for t, e in enumerate(table):
            rows[t, :int(e[1])] = frames(int(e[0]), int(e[0]) + int(e[1]))
        return rows

    stats = {k: [torch.zeros((n, NCH), dtype=torch.float64, device="cuda") for _ in range(2)] for k in "ab"}
    energy = {k: torch.zeros((n, NCH, longest // hop), dtype=torch.float64, device="cuda") for k in "ab"}
    work = torch.empty((n * NCH * (longest // hop) * 4,), dtype=torch.float64, device="cuda")
    hops = {}

    def packed_true_peak():
        F.tracks_true_peak_packed_device(src, tab, max_frames=longest, true_peak=stats["a"][0], peak=stats["a"][1], stream=stream)

    def packed_loudness():
        hops["a"] = F.tracks_loudness_packed_device(src, tab, rate=rate, max_frames=longest, energy=energy["a"], work=work, stream=stream)[1]

    def packed():
        packed_true_peak()
        packed_loudness()

    # peak memory: (a) alone, then (c) + (b); the rows stay for the timed rounds of (b)
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    packed()
    torch.cuda.synchronize()
    packed_peak = torch.cuda.max_memory_allocated() - base
    torch.cuda.reset_peak_memory_stats()
    rows = build_rows()

    def by_rows():
        F.tracks_true_peak_device(rows, tab, true_peak=stats["b"][0], peak=stats["b"][1], stream=stream)
        hops["b"] = F.tracks_loudness_device(rows, tab, rate=rate, energy=energy["b"], work=work, stream=stream)[1]

    by_rows()
    torch.cuda.synchronize()
    rows_peak = torch.cuda.max_memory_allocated() - base

    ams, tms, lms, bms, cms = [], [], [], [], []
    for _ in range(rounds):
        ams.append(timed(stream, packed, steps, warmup))
        bms.append(timed(stream, by_rows, steps, warmup))
        cms.append(timed(stream, build_rows, max(steps // 2, 1), 1))
        tms.append(timed(stream, packed_true_peak, steps, 1))
        lms.append(timed(stream, packed_loudness, steps, 1))
    torch.cuda.synchronize()
    equal = all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(stats["a"] + [energy["a"]], stats["b"] + [energy["b"]]))
    equal = equal and torch.equal(hops["a"], hops["b"])
    rel = max(float(((x - y).abs() / y.abs().clamp_min(1e-300)).max()) for x, y in zip(stats["a"] + [energy["a"]], stats["b"] + [energy["b"]]))
    a, b, c = statistics.median(ams), statistics.median(bms), statistics.median(cms)
    r4 = lambda v: [round(x, 4) for x in v]  # noqa: E731
    return {"format": fmt, "seed": seed, "tracks": n, "nch": NCH, "frames_total": total, "frames_longest": longest, "source_bytes": source_bytes,
            "packed_ms": round(a, 4), "packed_ms_rounds": r4(ams), "true_peak_ms": round(statistics.median(tms), 4),
            "loudness_ms": round(statistics.median(lms), 4), "rows_ms": round(b, 4), "rows_ms_rounds": r4(bms), "build_rows_ms": round(c, 4),
            "build_rows_ms_rounds": r4(cms), "ratio_to_rows": round(a / b, 4), "speedup_vs_build_and_rows": round((b + c) / a, 2),
            "packed_peak_bytes": packed_peak, "rows_peak_bytes": rows_peak, "equal_bits": bool(equal), "max_rel_diff": rel, "steps": steps,
            "warmup": warmup}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--formats", default="f32,s16,s24,s32")
    ap.add_argument("--seed", type=int, default=20240229)
    ap.add_argument("--tracks", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--s24-form", default="dword", help="recorded with the s24 line: which form of the S24 loudness pass the library under test has")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_perf.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_scan.py needs a GPU: there is nothing to time without one")
    lens = lengths(a.seed, a.tracks)
    slower = []
    for fmt in a.formats.split(","):
        line = one_format(fmt, lens, a.seed, a.steps, a.warmup, a.rounds)
        if fmt == "s24":
            line["s24_form"] = a.s24_form
        text = json.dumps(line)
        print(text, flush=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")
        if not line["packed_ms"] <= 1.10 * line["rows_ms"]:
            slower.append(fmt)
        torch.cuda.empty_cache()
    if slower:
        raise SystemExit("the packed passes are more than 10 %% slower than the row forms for %r" % (slower,))


if __name__ == "__main__":
    main()
