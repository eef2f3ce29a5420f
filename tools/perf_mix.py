"""Channel mixing on load (tracks_stage_mix_device, DESIGN.md 11, "Channel mixing") against what a caller with a 5.1 library in HBM
writes without it.

Workload: tools/perf_tracks.py's -- 64 tracks, 44.1 kHz -> 48 kHz, lengths between 2 and 7 minutes drawn with its LCG from --seed --
with SIX channels, as float32 and as packed S24, mixed to stereo by MIX_MATRICES["5.1_to_stereo"].  Every way is warmed up once,
then timed `--rounds` times (default 5, at least 5), the ways alternated within a round, between two HIP events on the current
stream, the second of which is synchronised on; medians and [min, max] are reported.  One JSON line per measurement, appended to
--out (default profiles/mix_perf.jsonl) and printed.

Measurement 1, per source format {"what": "stage_mix", "src_format"}: from the packed six-channel source to the stereo rows.
  (a) mix_stage        tracks_stage_mix_device: one pass, the source read once as stored;
  (b) torch_then_f32   what it replaces: torch builds the mixed float32 stereo packed source (S24: the bytes widened, shifted,
                       or-ed and scaled; then a float32 matmul with the matrix), then tracks_stage_device on it.
  "torch_mix_ms" is (b)'s torch part alone, "torch_peak_bytes" what (b) allocates at its peak beside the source and the rows, and
  "max_abs_diff" the largest difference of the two ways' rows ((b) has no stated bits: float32 products in torch's order).
  "mix_over_torch" = (a) / (b): the bar is that it is at most 1.
Measurement 2, in the same line: "plain_stage6_ms", the un-mixed tracks_stage_device of the same source into SIX-channel rows, and
  "mix_over_plain6" = (a) / that, beside "bytes_mix_over_plain6", the ratio of the bytes the two move (source + rows).
Measurement 3 {"what": "convert_mix"}: two whole conversions of the S24 tracks to stereo S16 with dither, each on a fresh handle.
  mix_on_load     convert_tracks_to_pcm_device(mix="5.1_to_stereo") on a stereo handle;
  mix_after       a six-channel handle, mix_device on its output rows, tracks_finish_device on the mixed rows.

  python tools/perf_mix.py [--seed 20240229] [--tracks 64] [--rounds 5] [--out FILE] [--skip-convert]
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
from perf_tracks import FO, FS, lengths, timed, to_s24  # noqa: E402

NSRC, NDST, MIX = 6, 2, "5.1_to_stereo"


def source(lens, fmt, seed):
    """packed six-channel tracks at a quarter of full scale, made in pieces: float32 [total, 6] or uint8 [total, 18]"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    total = sum(lens)
    out = torch.empty((total, NSRC) if fmt == F.RRX_FMT_FLOAT else (total, NSRC * 3), dtype=torch.float32 if fmt == F.RRX_FMT_FLOAT else torch.uint8,
                      device="cuda")
    for pos in range(0, total, 1 << 25):
        n = min(1 << 25, total - pos)
        if fmt == F.RRX_FMT_FLOAT:
            out[pos:pos + n] = (torch.rand((n, NSRC), generator=g, device="cuda") - 0.5) * 0.5
        else:
            out[pos:pos + n] = to_s24(torch.randint(-(1 << 21), 1 << 21, (n, NSRC), generator=g, device="cuda", dtype=torch.int32))
    return out


def torch_mix(packed, fmt, m32):
    """the mixed float32 stereo copy a caller makes with torch ops: unpack, scale, matmul"""
    if fmt == F.RRX_FMT_FLOAT:
        return torch.matmul(packed, m32)
    b = packed.view(packed.shape[0], -1, 3)
    v = b[..., 0].to(torch.int32) | (b[..., 1].to(torch.int32) << 8) | (b[..., 2].to(torch.int8).to(torch.int32) << 16)
    return torch.matmul(torch.mul(v, 2.0 ** -23), m32)


def spread(line, ms):
    for k, t in ms.items():
        line[k + "_ms"] = round(statistics.median(t), 3)
        line[k + "_ms_rounds"] = [round(x, 3) for x in t]
        line[k + "_range_ms"] = [round(min(t), 3), round(max(t), 3)]


def emit(a, line):
    text = json.dumps(line)
    print(text, flush=True)
    with open(a.out, "a") as f:
        f.write(text + "\n")


def stage_main(a, lens, name, fmt):
    plan = F.tracks_plan(FS, FO, lens)
    table, R, n = plan.to_device("cuda"), plan.row_frames, len(lens)
    M = F.mix_matrix(MIX)
    m32 = torch.from_numpy(M.T.copy()).to(torch.float32).cuda()              # [6, 2]
    packed = source(lens, fmt, a.seed)
    rows = torch.empty((n, R, NDST), dtype=torch.float32, device="cuda")
    rows6 = torch.empty((n, R, NSRC), dtype=torch.float32, device="cuda")
    mixed = [None]

    def mix_stage():
        F.tracks_stage_mix_device(packed, table, M, FS, FO, R, out=rows)

    def build():
        mixed[0] = None                                      # (the caching allocator hands the copy's memory back: no hipMalloc in a round)
        mixed[0] = torch_mix(packed, fmt, m32)

    def torch_then_f32():
        build()
        F.tracks_stage_device(mixed[0], table, FS, FO, R, out=rows)

    def plain_stage6():
        F.tracks_stage_device(packed, table, FS, FO, R, out=rows6)

    # warm-up, how far apart the two ways' rows are, and what (b) allocates
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    torch_then_f32()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    want = rows.clone()
    mix_stage()
    diff = 0.0
    for t in range(n):                                       # (track by track: no temporary of the rows' size)
        diff = max(diff, float((rows[t] - want[t]).abs().max()))
    del want
    plain_stage6()
    ways = {"mix_stage": mix_stage, "torch_then_f32": torch_then_f32, "torch_mix": build, "plain_stage6": plain_stage6}
    ms = {k: [] for k in ways}
    for _ in range(a.rounds):
        for k, fn in ways.items():
            ms[k].append(timed(fn)[0])
    src_bytes, row_bytes = packed.numel() * packed.element_size(), rows.numel() * 4
    line = {"what": "stage_mix", "src_format": name, "mix": MIX, "seed": a.seed, "tracks": n, "nch_src": NSRC, "nch": NDST, "in_rate": FS,
            "out_rate": FO, "frames_total": sum(lens), "row_frames": R, "source_bytes": src_bytes, "row_bytes": row_bytes,
            "row6_bytes": rows6.numel() * 4, "torch_peak_bytes": peak, "max_abs_diff": diff}
    spread(line, ms)
    line.update({"mix_over_torch": round(line["mix_stage_ms"] / line["torch_then_f32_ms"], 3),
                 "mix_over_plain6": round(line["mix_stage_ms"] / line["plain_stage6_ms"], 3),
                 "bytes_mix_over_plain6": round((src_bytes + row_bytes) / (src_bytes + rows6.numel() * 4), 3), "rounds": a.rounds})
    emit(a, line)


def convert_main(a, lens):
    plan = F.tracks_plan(FS, FO, lens)
    n = len(lens)
    packed = source(lens, F.RRX_FMT_S24_3, a.seed)
    offs = [0]
    for k in lens:
        offs.append(offs[-1] + k)
    tracks = [packed[offs[t]:offs[t + 1]] for t in range(n)]
    want = [int(e.out_frames) for e in plan.table]
    kw = dict(dither=True, seed=a.seed)

    def mix_on_load():
        r = F.Resampler(FS, FO, nch=NDST, nstreams=n)
        views, _, _ = r.convert_tracks_to_pcm_device(tracks, F.RRX_FMT_S16, mix=MIX, **kw)
        r.close()
        return [y.shape[0] for y in views]

    def mix_after():
        r = F.Resampler(FS, FO, nch=NSRC, nstreams=n)
        p, table, out = r._convert_tracks_rows(tracks)
        cur = torch.cuda.current_stream()
        stereo = F.mix_device(out, MIX, stream=cur)
        pcm, _, _ = F.tracks_finish_device(stereo, table, F.RRX_FMT_S16, p.dst_total, stream=cur, **kw)
        r.close()
        return [int(e.out_frames) for e in p.table]

    ways = {"mix_on_load": mix_on_load, "mix_after": mix_after}
    first = {k: round(timed(fn)[0], 2) for k, fn in ways.items()}
    ms = {k: [] for k in ways}
    for _ in range(a.rounds):
        for k, fn in ways.items():
            t, got = timed(fn)
            ms[k].append(t)
            assert got == want, k
    line = {"what": "convert_mix", "src_format": "s24_3", "dst_format": "s16", "mix": MIX, "seed": a.seed, "tracks": n, "nch_src": NSRC,
            "nch": NDST, "in_rate": FS, "out_rate": FO, "frames_total": sum(lens), "row_frames": plan.row_frames, "first_call_ms": first}
    spread(line, ms)
    line.update({"mix_on_load_over_mix_after": round(line["mix_on_load_ms"] / line["mix_after_ms"], 3), "rounds": a.rounds})
    emit(a, line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=20240229)
    ap.add_argument("--tracks", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix_perf.jsonl"))
    ap.add_argument("--skip-convert", action="store_true", help="measurements 1 and 2 only")
    a = ap.parse_args()
    if a.rounds < 5:
        raise SystemExit("at least five rounds: the spread is part of the result")
    if not torch.cuda.is_available():
        raise SystemExit("perf_mix.py needs a GPU: there is nothing to time without one")
    lens = lengths(a.seed, a.tracks)
    print("seed %d: %d tracks, %.1f to %.1f s, %.1f s in all" % (a.seed, len(lens), min(lens) / FS, max(lens) / FS, sum(lens) / FS), flush=True)
    for name, fmt in (("f32", F.RRX_FMT_FLOAT), ("s24_3", F.RRX_FMT_S24_3)):
        stage_main(a, lens, name, fmt)
        torch.cuda.empty_cache()
    if not a.skip_convert:
        convert_main(a, lens)


if __name__ == "__main__":
    main()
