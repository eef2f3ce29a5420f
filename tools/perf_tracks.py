"""A ragged batch of whole tracks (Resampler.convert_tracks_device) against the two things a caller with tracks of
unequal length in HBM can write without it.

Workload: 64 stereo tracks, 44.1 kHz -> 48 kHz, lengths between 2 and 7 minutes drawn with the LCG of tests/oracle_binding.py
(s = s * 1664525 + 1013904223 mod 2^32; length = 2 min + (s >> 8) / 2^24 * 5 min) from --seed, which is printed and recorded.
Three ways, each from float32 tracks in HBM to float32 tracks in HBM, each on a FRESH handle (a drained handle takes no second
track), so each time includes its RR_open / RRX_open_batch:

  ragged    one 64-stream handle, convert_tracks_device(tracks);
  loop      64 one-stream handles, convert_track_device(track[None]) one after the other: what a caller writes today;
  uniform   one 64-stream handle, convert_track_device of a [64, longest, 2] tensor: every row as long as the longest track,
            which is what the padding of the ragged batch costs, seen from above.

Each way is called once to warm up (code objects; torch's caching allocator, which afterwards reuses the 25 to 30 GB of rows a call
needs -- the first calls' times are kept as "first_call_ms") and then timed `--rounds` times (default 5), interleaved, between
two HIP events on the current stream (the events bracket the host work of the opens too: the stream idles while the host
plans); medians are reported.  One JSON line, appended to --out
(default profiles/tracks_perf.jsonl) and printed:

  {"seed", "tracks", "nch", "in_rate", "out_rate", "frames_total", "frames_longest", "row_frames", "padding_frames": the sum of
   row_frames - ext_i, "padding_share": padding_frames / (tracks * row_frames), "ragged_ms", "loop_ms", "uniform_ms", "*_rounds",
   "ragged_open_ms" / "loop_open_ms": host time of the opens inside those (time.perf_counter), "first_call_ms", "loop_over_ragged",
   "ragged_over_uniform", "rounds"}

  python tools/perf_tracks.py [--seed 20240229] [--tracks 64] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import foo_dsp_resampler_amd as F  # noqa: E402

FS, FO, NCH = 44100, 48000, 2


def lengths(seed, n):
    s, out = seed & 0xffffffff, []
    for _ in range(n):
        s = (s * 1664525 + 1013904223) & 0xffffffff
        out.append(2 * 60 * FS + (s >> 8) * (5 * 60 * FS) // (1 << 24))
    return out


def timed(fn):
    """(ms between two events around fn(), what fn returned)"""
    stream = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    r = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=20240229)
    ap.add_argument("--tracks", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracks_perf.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_tracks.py needs a GPU: there is nothing to time without one")
    lens = lengths(a.seed, a.tracks)
    print("seed %d: %d tracks, %.1f to %.1f s, %.1f s in all" % (a.seed, len(lens), min(lens) / FS, max(lens) / FS, sum(lens) / FS), flush=True)
    plan = F.tracks_plan(FS, FO, lens)
    padding = sum(plan.row_frames - int(e.frames + 2 * e.lead) for e in plan.table)
    torch.manual_seed(a.seed)
    tracks = [torch.rand((n, NCH), device="cuda") - 0.5 for n in lens]
    longest = max(lens)
    uniform_in = torch.zeros((len(lens), longest, NCH), device="cuda")
    for t, x in enumerate(tracks):
        uniform_in[t, :x.shape[0]] = x
    torch.cuda.synchronize()
    open_ms = {"ragged": [], "loop": []}

    def ragged():
        t0 = time.perf_counter()
        r = F.Resampler(FS, FO, nch=NCH, nstreams=len(tracks))
        open_ms["ragged"].append((time.perf_counter() - t0) * 1e3)
        ys = r.convert_tracks_device(tracks)
        r.close()
        return [y.shape[0] for y in ys]

    def loop():
        spent, got = 0.0, []
        for x in tracks:
            t0 = time.perf_counter()
            r = F.Resampler(FS, FO, nch=NCH)
            spent += time.perf_counter() - t0
            got.append(r.convert_track_device(x[None]).shape[1])
            r.close()
        open_ms["loop"].append(spent * 1e3)
        return got

    def uniform():
        r = F.Resampler(FS, FO, nch=NCH, nstreams=len(tracks))
        y = r.convert_track_device(uniform_in)
        r.close()
        return y.shape[1]

    ways = {"ragged": ragged, "loop": loop, "uniform": uniform}
    ms = {k: [] for k in ways}
    # one untimed-for-the-median call of each way first: code objects, and torch's caching allocator, which then hands every later
    # round its rows back without a hipMalloc (a first call allocates 25 to 30 GB afresh and is dominated by that)
    first = {k: round(timed(fn)[0], 2) for k, fn in ways.items()}
    for v in open_ms.values():
        v.clear()
    for _ in range(a.rounds):
        for k, fn in ways.items():
            t, got = timed(fn)
            ms[k].append(t)
            if k != "uniform":
                assert got == [int(e.out_frames) for e in plan.table], k
    med = {k: statistics.median(v) for k, v in ms.items()}
    line = {"seed": a.seed, "tracks": len(lens), "nch": NCH, "in_rate": FS, "out_rate": FO, "frames_total": sum(lens), "frames_longest": longest,
            "row_frames": plan.row_frames, "padding_frames": padding, "padding_share": round(padding / (len(lens) * plan.row_frames), 4)}
    for k in ways:
        line[k + "_ms"] = round(med[k], 2)
        line[k + "_ms_rounds"] = [round(t, 2) for t in ms[k]]
    for k in open_ms:
        line[k + "_open_ms"] = round(statistics.median(open_ms[k]), 2)
    line["first_call_ms"] = first
    line.update({"loop_over_ragged": round(med["loop"] / med["ragged"], 2), "ragged_over_uniform": round(med["ragged"] / med["uniform"], 3),
                 "rounds": a.rounds})
    text = json.dumps(line)
    print(text, flush=True)
    with open(a.out, "a") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
