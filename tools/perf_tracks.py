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

--pcm measures the integer sources of the stage pass instead ("Integer sources"), on the same workload, and appends
to profiles/tracks_pcm_perf.jsonl.  Stage only, per source format S16 / S24_3 / S32, from the packed integer tracks in HBM to the
float32 rows in HBM:

  (a) int_stage       tracks_stage_device on the integer source: one pass;
  (b) torch_then_f32  what a caller writes without it: a torch pass that converts the packed source to a float32 copy (S16 / S32:
                      ONE elementwise kernel, torch.mul(int tensor, 2^-bits); S24_3: the bytes widened, shifted, or-ed and scaled
                      by torch ops), then tracks_stage_device on that copy.

The rows of (a) and (b) are compared once, bit for bit, before anything is timed ("rows_equal").  Then convert_tracks_to_pcm_device
end to end, S16 tracks to S16 against float32 tracks to S16, each on a fresh handle as above.  One warm-up, `--rounds` rounds
interleaved, HIP events, medians.  One JSON line per format {"what": "stage", "src_format", "int_stage_ms", "torch_then_f32_ms",
"torch_convert_ms": the conversion alone, "*_rounds", "int_over_torch": (a) / (b), "source_bytes", "row_bytes", "rows_equal"} and one
{"what": "end_to_end", "s16_tracks_ms", "f32_tracks_ms", "s16_over_f32"}.

  python tools/perf_tracks.py --pcm [--seed 20240229] [--tracks 64] [--rounds 5] [--out FILE]

--streamed measures the window form ("Windows") on the same workload, S16 tracks in, packed S24 out with dither, and
appends to profiles/tracks_window_perf.jsonl:

  whole_rows   convert_tracks_to_pcm_device: every row staged, pushed, pulled and finished whole;
  streamed     convert_tracks_to_pcm_streamed(window=--window, default isamp_max): two windows and no rows.

Each on a fresh handle.  The two results are compared once, byte for byte and statistic for statistic, before anything is timed
("equal").  One warm-up, `--rounds` rounds interleaved, HIP events, medians and ranges; torch.cuda.max_memory_allocated of each form
is taken over a call of its own after the warm-up, with the tracks themselves (which both forms are handed) subtracted.  One JSON
line {"what": "streamed", "window", "isamp_max", "whole_rows_ms", "streamed_ms", "*_rounds", "*_range_ms": [min, max],
"streamed_over_whole_rows", "whole_rows_peak_bytes", "streamed_peak_bytes", "tracks_bytes", "first_call_ms", "equal", "parts_ms": the passes of the two forms each on its own (streamed_parts)}.

  python tools/perf_tracks.py --streamed [--window FRAMES] [--seed 20240229] [--tracks 64] [--rounds 5] [--out FILE]

--streamed --shaped measures noise-shaped dither in the window form on the same batch, S16 tracks in, packed S16 out, `wannamaker9`,
at segments 4096, 16384 and 65536, and appends one line per segment to profiles/tracks_window_shaped_perf.jsonl.  Three ways in one
process, each on a fresh handle:

  streamed_shaped     convert_tracks_to_pcm_streamed_shaped(window=--window): two windows, two states and no rows;
  whole_rows_shaped   convert_tracks_to_pcm_device(shaping=): every row whole, all segments of a track side by side;
  streamed            convert_tracks_to_pcm_streamed, dither without shaping: what the windows cost without the serial chain.

The two shaped results are compared first ("equal"); warm-up, rounds, medians, ranges and peak memory as above.  One JSON line
{"what": "streamed_shaped", "segment", "shaping", "window", "win_out", "windows_out", "<way>_ms", "<way>_ms_rounds", "<way>_range_ms",
"<way>_peak_bytes", "streamed_shaped_over_whole_rows_shaped", "streamed_shaped_over_streamed", "chain_frames_streamed": windows_out *
min(segment, win_out), "chain_frames_whole_rows": min(segment, longest output), "equal"} -- the chain lengths DESIGN.md 11 predicts
the cost from.

  python tools/perf_tracks.py --streamed --shaped [--window FRAMES] [--seed 20240229] [--tracks 64] [--rounds 5] [--out FILE]

--streamed --normalized measures the streamed loudness-normalised conversion ("Windows with true peak and loudness")
on the same batch, S16 tracks in, packed S24 out with dither, at the two windows measured above (isamp_max and 65536; --window: that
one only), and appends one line per window to profiles/tracks_window_measure_perf.jsonl.  Four ways in one process, each on a fresh
handle:

  pass_a                  the measuring pass alone: the streamed loop with the two measuring window calls in place of the output stage;
  streamed_normalized     convert_tracks_to_pcm_streamed_loudness_normalized: pass A, the gain, a reset, the streamed conversion;
  streamed                convert_tracks_to_pcm_streamed: what one pass over the windows costs;
  whole_rows_normalized   convert_tracks_to_pcm_loudness_normalized: every row whole, converted once.

The two normalised results are compared first, every element of their tuples ("equal"); warm-up, rounds, medians, ranges and peak
memory as above.  One JSON line {"what": "streamed_normalized", "window", "win_out", "windows_out", "hop", "<way>_ms", "<way>_ms_rounds",
"<way>_range_ms", "<way>_peak_bytes", "pass_a_over_streamed", "streamed_normalized_over_whole_rows_normalized", "measuring_ms": pass_a -
streamed, "predicted_loudness_ms": windows_out * 2 * hop * 230 cycles at 2.4 GHz, the cost DESIGN.md 11 predicts, "equal"}.

  python tools/perf_tracks.py --streamed --normalized [--window FRAMES] [--seed 20240229] [--tracks 64] [--rounds 5] [--out FILE]

--library measures a library on ONE handle ("Libraries"): the same LCG lengths, 256 tracks (--tracks) on a handle of 64
streams (--streams), S16 tracks in, packed S24 out with dither and per-track gains, at phase 50 and at phase 25, and appends to
profiles/tracks_library_perf.jsonl:

  (a) one_handle     convert_library_to_pcm on one handle, opened once before anything is timed: sorted batches, a reset between
                     them, rows reused;
  (b) fresh_sorted   the same sorted batches, each through convert_tracks_to_pcm_device on a fresh handle that is opened and
                     closed: what a caller writes without RRX_reset;
  (c) fresh_given    the same tracks cut into batches in their given order, on fresh handles.

(a) and (b) are compared first, byte for byte and statistic for statistic ("equal"); (c) puts a track on another dither channel, so
it is compared with the two in a pass without dither ("equal_without_dither").  One warm-up, `--rounds` rounds interleaved, HIP
events, medians and ranges.  Host times (time.perf_counter, the handle waited for): one reset against RR_close + RRX_open_batch on
the used handle, and the first open of the config on an empty plan cache against the second.  One JSON line per phase {"what":
"library", "phase", "tracks", "streams", "batches", "padding_sorted", "padding_given", "one_handle_ms", "fresh_sorted_ms",
"fresh_given_ms", "*_rounds", "*_range_ms", "one_handle_over_fresh_sorted", "reset_ms", "close_open_ms", "first_open_ms",
"second_open_ms", "plan_cache", "first_call_ms", "equal", "equal_without_dither"}.

  python tools/perf_tracks.py --library [--seed 20240229] [--tracks 256] [--streams 64] [--rounds 5] [--out FILE]
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


PCM = (("s16", F.RRX_FMT_S16, 15), ("s24_3", F.RRX_FMT_S24_3, 23), ("s32", F.RRX_FMT_S32, 31))


def pcm_source(lens, bits, seed):
    """packed integer tracks [frames_total, nch] at half of full scale (int64 would not fit beside the rows: made in pieces)"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    total = sum(lens)
    dt = torch.int16 if bits == 15 else torch.int32
    out = torch.empty((total, NCH), dtype=dt, device="cuda")
    half = 1 << (bits - 1)
    for pos in range(0, total, 1 << 26):
        n = min(1 << 26, total - pos)
        out[pos:pos + n] = torch.randint(-half, half, (n, NCH), generator=g, device="cuda", dtype=torch.int32).to(dt)
    return out


def to_s24(v):
    """int32 [frames, nch] in [-2^23, 2^23) -> packed bytes [frames, nch * 3]"""
    out = torch.empty(v.shape + (3,), dtype=torch.uint8, device=v.device)
    for k in range(3):
        out[..., k] = (v >> (8 * k)) & 0xff
    return out.view(v.shape[0], -1)


def torch_convert(packed, fmt, bits):
    """the float32 copy a caller makes with torch ops"""
    if fmt != F.RRX_FMT_S24_3:
        return torch.mul(packed, 2.0 ** -bits)               # one kernel: integer in, float32 out
    b = packed.view(packed.shape[0], -1, 3)
    v = b[..., 0].to(torch.int32) | (b[..., 1].to(torch.int32) << 8) | (b[..., 2].to(torch.int8).to(torch.int32) << 16)
    return torch.mul(v, 2.0 ** -bits)


def pcm_main(a, lens):
    plan = F.tracks_plan(FS, FO, lens)
    table = plan.to_device("cuda")
    R = plan.row_frames
    rows = torch.empty((len(lens), R, NCH), dtype=torch.float32, device="cuda")
    lines = []
    for name, fmt, bits in PCM:
        v = pcm_source(lens, 23 if bits == 23 else bits, a.seed)
        packed = to_s24(v) if bits == 23 else v
        del v
        f32 = [None]

        def int_stage():
            F.tracks_stage_device(packed, table, FS, FO, R, out=rows)

        def convert():
            f32[0] = None                                    # (the caching allocator hands the copy's memory back: no hipMalloc in a round)
            f32[0] = torch_convert(packed, fmt, bits)

        def torch_then_f32():
            convert()
            F.tracks_stage_device(f32[0], table, FS, FO, R, out=rows)

        # warm-up, and the check that the two ways give the same rows
        torch_then_f32()
        want = rows.clone()
        int_stage()
        equal = bool(torch.equal(rows.view(torch.int32), want.view(torch.int32)))
        del want
        convert()
        ways = {"int_stage": int_stage, "torch_then_f32": torch_then_f32, "torch_convert": convert}
        ms = {k: [] for k in ways}
        for _ in range(a.rounds):
            for k, fn in ways.items():
                ms[k].append(timed(fn)[0])
        med = {k: statistics.median(t) for k, t in ms.items()}
        line = {"what": "stage", "src_format": name, "seed": a.seed, "tracks": len(lens), "nch": NCH, "in_rate": FS, "out_rate": FO,
                "frames_total": sum(lens), "row_frames": R, "source_bytes": packed.numel() * packed.element_size(),
                "row_bytes": rows.numel() * 4, "rows_equal": equal}
        for k in ways:
            line[k + "_ms"] = round(med[k], 3)
            line[k + "_ms_rounds"] = [round(t, 3) for t in ms[k]]
        line.update({"int_over_torch": round(med["int_stage"] / med["torch_then_f32"], 3), "rounds": a.rounds})
        lines.append(line)
        print(json.dumps(line), flush=True)
        f32[0] = packed = None
        torch.cuda.empty_cache()
    del rows
    torch.cuda.empty_cache()
    # end to end: S16 tracks -> S16 against float32 tracks -> S16
    v = pcm_source(lens, 15, a.seed)
    offs = [0]
    for n in lens:
        offs.append(offs[-1] + n)
    i16 = [v[offs[t]:offs[t + 1]] for t in range(len(lens))]
    f32t = [torch.mul(x, 2.0 ** -15) for x in i16]

    def end_to_end(tracks):
        def run():
            r = F.Resampler(FS, FO, nch=NCH, nstreams=len(tracks))
            views, _, _ = r.convert_tracks_to_pcm_device(tracks, F.RRX_FMT_S16, dither=True, seed=a.seed)
            r.close()
            return [y.shape[0] for y in views]
        return run

    ways = {"s16_tracks": end_to_end(i16), "f32_tracks": end_to_end(f32t)}
    first = {k: round(timed(fn)[0], 2) for k, fn in ways.items()}
    ms = {k: [] for k in ways}
    for _ in range(a.rounds):
        for k, fn in ways.items():
            t, got = timed(fn)
            ms[k].append(t)
            assert got == [int(e.out_frames) for e in plan.table], k
    med = {k: statistics.median(t) for k, t in ms.items()}
    line = {"what": "end_to_end", "dst_format": "s16", "seed": a.seed, "tracks": len(lens), "nch": NCH, "in_rate": FS, "out_rate": FO,
            "frames_total": sum(lens), "row_frames": R}
    for k in ways:
        line[k + "_ms"] = round(med[k], 2)
        line[k + "_ms_rounds"] = [round(t, 2) for t in ms[k]]
    line.update({"first_call_ms": first, "s16_over_f32": round(med["s16_tracks"] / med["f32_tracks"], 3), "rounds": a.rounds})
    lines.append(line)
    print(json.dumps(line), flush=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


def streamed_parts(a, lens, plan, packed, window):
    """Where the time of the two forms goes: the three passes of the streamed loop each on its own -- every window staged, a fresh
    handle pushed window by window and pulled (zeros in: the resampler's time does not depend on the samples), every output window
    finished -- against the whole-row stage and finish calls.  Medians of `--rounds` rounds, HIP events; the whole-row resampling is
    what is left of that form's time."""
    n, table = len(lens), plan.to_device("cuda")
    total = plan.row_frames + -(-2 * FS // FO) + 1
    cap = total * FO // FS + 2
    win_out = -(-window * FO // FS)
    win = torch.zeros((n, window, NCH), dtype=torch.float32, device="cuda")
    wout = torch.zeros((n, win_out, NCH), dtype=torch.float32, device="cuda")
    kw = dict(dither=True, seed=a.seed)
    _, peak, clipped = F.tracks_finish_window_device(wout, table, cap, 0, 0, None, plan.dst_total)
    dst = torch.empty((plan.dst_total, NCH * 3), dtype=torch.uint8, device="cuda")

    def stage_windows():
        for pos in range(0, total, window):
            F.tracks_stage_window_device(packed, table, FS, FO, total, pos, min(window, total - pos), out=win)

    def finish_windows():
        for pos in range(0, cap, win_out):
            F.tracks_finish_window_device(wout, table, cap, pos, min(win_out, cap - pos), F.RRX_FMT_S24_3, plan.dst_total, out=dst, peak=peak,
                                          clipped=clipped, **kw)

    def resample_windows():
        r = F.Resampler(FS, FO, nch=NCH, nstreams=n)
        r.set_stream(torch.cuda.current_stream().cuda_stream)

        def pull():
            while r.available:
                r.pull_device(wout, win_out, stride=win_out)

        for pos in range(0, total, window):
            r.push_device(win, min(window, total - pos), stride=window)
            pull()
        r.drain()
        pull()
        r.close()

    rows = torch.empty((n, plan.row_frames, NCH), dtype=torch.float32, device="cuda")
    orows = torch.zeros((n, plan.out_row_cap, NCH), dtype=torch.float32, device="cuda")
    ways = {"stage_windows": stage_windows, "resample_windows": resample_windows, "finish_windows": finish_windows,
            "stage_whole": lambda: F.tracks_stage_device(packed, table, FS, FO, plan.row_frames, out=rows),
            "finish_whole": lambda: F.tracks_finish_device(orows, table, F.RRX_FMT_S24_3, plan.dst_total, out=dst, peak=peak, clipped=clipped, **kw)}
    for fn in ways.values():
        fn()
    ms = {k: [] for k in ways}
    for _ in range(a.rounds):
        for k, fn in ways.items():
            ms[k].append(timed(fn)[0])
    out = {k: round(statistics.median(t), 2) for k, t in ms.items()}
    out["windows_in"], out["windows_out"] = -(-total // window), -(-cap // win_out)
    return out


def compare_ways(a, plan, ways, one, other):
    """what the --streamed runs share: every way of `ways` ({name: run(keep=False)}) warmed up once, `one` and `other` compared byte
    for byte and statistic for statistic, the peak allocation of each over a call of its own, then `a.rounds` rounds interleaved.
    (first call ms, equal, peak bytes, ms per round, medians)"""
    first = {k: round(timed(fn)[0], 2) for k, fn in ways.items()}        # warm-up: code objects, the caching allocator
    a_res, b_res = ways[one](keep=True), ways[other](keep=True)
    equal = bool(torch.equal(a_res[0][0]._base, b_res[0][0]._base) and torch.equal(a_res[1].view(torch.int64), b_res[1].view(torch.int64))
                 and torch.equal(a_res[2], b_res[2]))
    del a_res, b_res
    peak = {}
    for k, fn in ways.items():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated() - before
    for fn in ways.values():                                             # (the cache was emptied: fill it again before timing)
        fn()
    ms = {k: [] for k in ways}
    for _ in range(a.rounds):
        for k, fn in ways.items():
            t, got = timed(fn)
            ms[k].append(t)
            assert got == [int(e.out_frames) for e in plan.table], k
    return first, equal, peak, ms, {k: statistics.median(t) for k, t in ms.items()}


def ways_into(line, ways, peak, ms, med):
    for k in ways:
        line[k + "_ms"] = round(med[k], 2)
        line[k + "_ms_rounds"] = [round(t, 2) for t in ms[k]]
        line[k + "_range_ms"] = [round(min(ms[k]), 2), round(max(ms[k]), 2)]
        line[k + "_peak_bytes"] = peak[k]


SHAPED_SEGMENTS = (4096, 16384, 65536)


def streamed_shaped_main(a, lens):
    plan = F.tracks_plan(FS, FO, lens)
    v = pcm_source(lens, 15, a.seed)
    offs = [0]
    for n in lens:
        offs.append(offs[-1] + n)
    tracks = [v[offs[t]:offs[t + 1]] for t in range(len(lens))]
    kw = dict(dither=True, seed=a.seed)
    shaping, fmt = "wannamaker9", F.RRX_FMT_S16
    isamp_max = [0]
    for segment in SHAPED_SEGMENTS:
        def form(which):
            def run(keep=False):
                r = F.Resampler(FS, FO, nch=NCH, nstreams=len(tracks))
                isamp_max[0] = r.isamp_max
                if which == "streamed_shaped":
                    res = r.convert_tracks_to_pcm_streamed_shaped(tracks, fmt, shaping, segment, window=a.window, **kw)
                elif which == "whole_rows_shaped":
                    res = r.convert_tracks_to_pcm_device(tracks, fmt, shaping=shaping, segment=segment, **kw)
                else:
                    res = r.convert_tracks_to_pcm_streamed(tracks, fmt, window=a.window, **kw)
                r.close()
                return res if keep else [y.shape[0] for y in res[0]]
            return run

        ways = {k: form(k) for k in ("streamed_shaped", "whole_rows_shaped", "streamed")}
        first, equal, peak, ms, med = compare_ways(a, plan, ways, "whole_rows_shaped", "streamed_shaped")
        window = a.window if a.window is not None else isamp_max[0]
        total = plan.row_frames + -(-2 * FS // FO) + 1                   # the virtual rows of the streamed forms (ratelib.py)
        cap, win_out = total * FO // FS + 2, -(-window * FO // FS)
        windows_out = -(-cap // min(win_out, cap))
        line = {"what": "streamed_shaped", "segment": segment, "shaping": shaping, "src_format": "s16", "dst_format": "s16", "seed": a.seed,
                "tracks": len(lens), "nch": NCH, "in_rate": FS, "out_rate": FO, "frames_total": sum(lens), "row_frames": plan.row_frames,
                "out_row_cap": plan.out_row_cap, "window": window, "isamp_max": isamp_max[0], "win_out": win_out, "windows_out": windows_out}
        ways_into(line, ways, peak, ms, med)
        line.update({"streamed_shaped_over_whole_rows_shaped": round(med["streamed_shaped"] / med["whole_rows_shaped"], 3),
                     "streamed_shaped_over_streamed": round(med["streamed_shaped"] / med["streamed"], 3),
                     "chain_frames_streamed": windows_out * min(segment, win_out),
                     "chain_frames_whole_rows": min(segment, max(int(e.out_frames) for e in plan.table)),
                     "tracks_bytes": v.numel() * v.element_size(), "first_call_ms": first, "equal": equal, "rounds": a.rounds})
        text = json.dumps(line)
        print(text, flush=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")


def streamed_normalized_main(a, lens):
    plan = F.tracks_plan(FS, FO, lens)
    v = pcm_source(lens, 15, a.seed)
    offs = [0]
    for n in lens:
        offs.append(offs[-1] + n)
    tracks = [v[offs[t]:offs[t + 1]] for t in range(len(lens))]
    kw = dict(dither=True, seed=a.seed)
    fmt = F.RRX_FMT_S24_3
    isamp_max = [0]
    want = [int(e.out_frames) for e in plan.table]
    for window in (None, 65536) if a.window is None else (a.window,):
        def form(which):
            def run(keep=False):
                r = F.Resampler(FS, FO, nch=NCH, nstreams=len(tracks))
                isamp_max[0] = r.isamp_max
                if which == "pass_a":                            # the measuring pass of the streamed loudness-normalised form, alone
                    import functools
                    res = r._convert_tracks_streamed(list(tracks), fmt, window, None, None, {}, "pass_a",
                                                     measure=functools.partial(F.ratelib._WindowMeter, FO, NCH))
                    r.close()
                    return res if keep else want
                if which == "streamed_normalized":
                    res = r.convert_tracks_to_pcm_streamed_loudness_normalized(tracks, fmt, window=window, **kw)
                elif which == "whole_rows_normalized":
                    res = r.convert_tracks_to_pcm_loudness_normalized(tracks, fmt, **kw)
                else:
                    res = r.convert_tracks_to_pcm_streamed(tracks, fmt, window=window, **kw)
                r.close()
                return res if keep else [y.shape[0] for y in res[0]]
            return run

        ways = {k: form(k) for k in ("pass_a", "streamed_normalized", "streamed", "whole_rows_normalized")}
        first = {k: round(timed(fn)[0], 2) for k, fn in ways.items()}        # warm-up: code objects, the caching allocator
        x, y = ways["whole_rows_normalized"](keep=True), ways["streamed_normalized"](keep=True)
        equal = bool(torch.equal(x[0][0]._base, y[0][0]._base) and all(torch.equal(p.contiguous().view(torch.int64), q.contiguous().view(torch.int64))
                                                                       for p, q in zip(x[1:], y[1:])))
        del x, y
        peak = {}
        for k, fn in ways.items():
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            peak[k] = torch.cuda.max_memory_allocated() - before
        for fn in ways.values():                                             # (the cache was emptied: fill it again before timing)
            fn()
        ms = {k: [] for k in ways}
        for _ in range(a.rounds):
            for k, fn in ways.items():
                t, got = timed(fn)
                ms[k].append(t)
                assert got == want, k
        med = {k: statistics.median(t) for k, t in ms.items()}
        win = window if window is not None else isamp_max[0]
        total = plan.row_frames + -(-2 * FS // FO) + 1                       # the virtual rows of the streamed forms (ratelib.py)
        cap, win_out = total * FO // FS + 2, -(-win * FO // FS)
        windows_out = -(-cap // min(win_out, cap))
        hop = FO // 10
        line = {"what": "streamed_normalized", "src_format": "s16", "dst_format": "s24_3", "seed": a.seed, "tracks": len(lens), "nch": NCH,
                "in_rate": FS, "out_rate": FO, "frames_total": sum(lens), "row_frames": plan.row_frames, "out_row_cap": plan.out_row_cap,
                "window": win, "isamp_max": isamp_max[0], "win_out": win_out, "windows_out": windows_out, "hop": hop}
        ways_into(line, ways, peak, ms, med)
        line.update({"pass_a_over_streamed": round(med["pass_a"] / med["streamed"], 3),
                     "streamed_normalized_over_whole_rows_normalized": round(med["streamed_normalized"] / med["whole_rows_normalized"], 3),
                     "measuring_ms": round(med["pass_a"] - med["streamed"], 2),     # pass A has no output stage: a lower bound of the measuring
                     "predicted_loudness_ms": round(windows_out * 2 * hop * 230 / 2.4e6, 1),   # windows x 2 x one hop's chain, 230 cycles a frame at 2.4 GHz
                     "tracks_bytes": v.numel() * v.element_size(), "first_call_ms": first, "equal": equal, "rounds": a.rounds})
        text = json.dumps(line)
        print(text, flush=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")


def streamed_main(a, lens):
    plan = F.tracks_plan(FS, FO, lens)
    v = pcm_source(lens, 15, a.seed)
    offs = [0]
    for n in lens:
        offs.append(offs[-1] + n)
    tracks = [v[offs[t]:offs[t + 1]] for t in range(len(lens))]
    kw = dict(dither=True, seed=a.seed)
    isamp_max = [0]

    def form(streamed):
        def run(keep=False):
            r = F.Resampler(FS, FO, nch=NCH, nstreams=len(tracks))
            isamp_max[0] = r.isamp_max
            if streamed:
                res = r.convert_tracks_to_pcm_streamed(tracks, F.RRX_FMT_S24_3, window=a.window, **kw)
            else:
                res = r.convert_tracks_to_pcm_device(tracks, F.RRX_FMT_S24_3, **kw)
            r.close()
            return res if keep else [y.shape[0] for y in res[0]]
        return run

    ways = {"whole_rows": form(False), "streamed": form(True)}
    first, equal, peak, ms, med = compare_ways(a, plan, ways, "whole_rows", "streamed")
    line = {"what": "streamed", "src_format": "s16", "dst_format": "s24_3", "seed": a.seed, "tracks": len(lens), "nch": NCH, "in_rate": FS,
            "out_rate": FO, "frames_total": sum(lens), "row_frames": plan.row_frames, "out_row_cap": plan.out_row_cap,
            "window": a.window if a.window is not None else isamp_max[0], "isamp_max": isamp_max[0]}
    ways_into(line, ways, peak, ms, med)
    line.update({"streamed_over_whole_rows": round(med["streamed"] / med["whole_rows"], 3), "tracks_bytes": v.numel() * v.element_size(),
                 "first_call_ms": first, "equal": equal, "rounds": a.rounds, "parts_ms": streamed_parts(a, lens, plan, v, line["window"])})
    text = json.dumps(line)
    print(text, flush=True)
    with open(a.out, "a") as f:
        f.write(text + "\n")


def library_main(a, lens):
    S, n = a.streams, len(lens)
    v = pcm_source(lens, 15, a.seed)
    offs = [0]
    for k in lens:
        offs.append(offs[-1] + k)
    tracks = [v[offs[t]:offs[t + 1]] for t in range(n)]
    gains = [0.5 + (t % 7) * 0.125 for t in range(n)]
    gain_dev = torch.tensor(gains, dtype=torch.float64, device="cuda")
    K = 0xBF58476D1CE4E5B9
    given = [list(range(k, min(k + S, n))) for k in range(0, n, S)]
    for phase in (50.0, 25.0):
        tb = F.tracks_batches(FS, FO, lens, S, phase=phase)
        given_rows = [F.tracks_plan(FS, FO, [lens[i] for i in idx], phase=phase).row_frames for idx in given]
        padding_given = 1.0 - tb.useful / (S * sum(given_rows))
        # host times of the opens, before anything else warms the plan cache for this config
        F.plan_cache_clear()
        t0 = time.perf_counter()
        r = F.Resampler(FS, FO, nch=NCH, nstreams=S, phase=phase)
        first_open = (time.perf_counter() - t0) * 1e3
        r.close()
        t0 = time.perf_counter()
        r = F.Resampler(FS, FO, nch=NCH, nstreams=S, phase=phase)
        second_open = (time.perf_counter() - t0) * 1e3
        one = [r]                                            # the one handle of (a); replaced by the close + open measurement below

        def one_handle(dither=True, keep=False):
            res = one[0].convert_library_to_pcm(tracks, F.RRX_FMT_S24_3, gain=gain_dev, dither=dither, seed=a.seed)
            return res if keep else [y.shape[0] for y in res[0]]

        def fresh(batches):
            def run(dither=True, keep=False):
                views, peak, clipped = [None] * n, [None] * n, [None] * n
                for b, idx in enumerate(batches):
                    h = F.Resampler(FS, FO, nch=NCH, nstreams=S, phase=phase)
                    w, p, c = h.convert_tracks_to_pcm_device([tracks[i] for i in idx], F.RRX_FMT_S24_3, gain=gain_dev[idx].contiguous(),
                                                             dither=dither, seed=(a.seed + b * S * NCH * K) % (1 << 64))
                    h.close()
                    for k, i in enumerate(idx):
                        views[i], peak[i], clipped[i] = w[k], p[k], c[k]
                return (views, torch.stack(peak), torch.stack(clipped)) if keep else [y.shape[0] for y in views]
            return run

        def same(x, y):
            return bool(all(torch.equal(p, q) for p, q in zip(x[0], y[0])) and torch.equal(x[1].view(torch.int64), y[1].view(torch.int64))
                        and torch.equal(x[2], y[2]))

        ways = {"one_handle": one_handle, "fresh_sorted": fresh(tb.batches), "fresh_given": fresh(given)}
        first = {k: round(timed(fn)[0], 2) for k, fn in ways.items()}        # warm-up: code objects, the caching allocator
        x = one_handle(keep=True)
        y = ways["fresh_sorted"](keep=True)
        equal = same(x, y)
        del x, y
        x = one_handle(dither=False, keep=True)
        equal_plain = True
        for k in ("fresh_sorted", "fresh_given"):
            y = ways[k](dither=False, keep=True)
            equal_plain = equal_plain and same(x, y)
            del y
        del x
        want = [F.track_geometry(FS, FO, k, phase=phase)[3] for k in lens]
        ms = {k: [] for k in ways}
        for _ in range(a.rounds):
            for k, fn in ways.items():
                t, got = timed(fn)
                ms[k].append(t)
                assert got == want, k
        med = {k: statistics.median(t) for k, t in ms.items()}
        # one reset against close + open, on the handle the library has just used
        reset_ms, close_open_ms = [], []
        for _ in range(a.rounds):
            one_handle()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            one[0].reset()
            one[0].sync()
            reset_ms.append((time.perf_counter() - t0) * 1e3)
            one_handle()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            one[0].close()
            one[0] = F.Resampler(FS, FO, nch=NCH, nstreams=S, phase=phase)
            one[0].sync()
            close_open_ms.append((time.perf_counter() - t0) * 1e3)
        one[0].close()
        line = {"what": "library", "phase": phase, "src_format": "s16", "dst_format": "s24_3", "seed": a.seed, "tracks": n, "streams": S,
                "nch": NCH, "in_rate": FS, "out_rate": FO, "frames_total": sum(lens), "batches": len(tb), "row_frames": tb.row_frames,
                "padding_sorted": round(tb.padding, 4), "padding_given": round(padding_given, 4)}
        for k in ways:
            line[k + "_ms"] = round(med[k], 2)
            line[k + "_ms_rounds"] = [round(t, 2) for t in ms[k]]
            line[k + "_range_ms"] = [round(min(ms[k]), 2), round(max(ms[k]), 2)]
        hits, misses, entries = F.plan_cache_stats()
        line.update({"one_handle_over_fresh_sorted": round(med["one_handle"] / med["fresh_sorted"], 3),
                     "reset_ms": round(statistics.median(reset_ms), 3), "reset_ms_rounds": [round(t, 3) for t in reset_ms],
                     "close_open_ms": round(statistics.median(close_open_ms), 3), "close_open_ms_rounds": [round(t, 3) for t in close_open_ms],
                     "first_open_ms": round(first_open, 2), "second_open_ms": round(second_open, 2),
                     "plan_cache": {"hits": hits, "misses": misses, "entries": entries},
                     "first_call_ms": first, "equal": equal, "equal_without_dither": equal_plain, "rounds": a.rounds})
        text = json.dumps(line)
        print(text, flush=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=20240229)
    ap.add_argument("--tracks", type=int, default=None, help="default 64; --library: 256")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pcm", action="store_true", help="integer sources of the stage pass instead (see above)")
    ap.add_argument("--streamed", action="store_true", help="the window form against the whole-row form instead (see above)")
    ap.add_argument("--window", type=int, default=None, help="--streamed: frames of the input window (default: isamp_max)")
    ap.add_argument("--shaped", action="store_true", help="--streamed: noise-shaped dither in the window form instead (see above)")
    ap.add_argument("--normalized", action="store_true", help="--streamed: the streamed loudness-normalised conversion instead (see above)")
    ap.add_argument("--library", action="store_true", help="a library on one handle against fresh handles per batch instead (see above)")
    ap.add_argument("--streams", type=int, default=64, help="--library: streams of the handle")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.tracks is None:
        a.tracks = 256 if a.library else 64
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "tracks_library_perf.jsonl" if a.library else "tracks_window_shaped_perf.jsonl" if a.streamed and a.shaped else
                             "tracks_window_measure_perf.jsonl" if a.streamed and a.normalized else
                             "tracks_window_perf.jsonl" if a.streamed else
                             "tracks_pcm_perf.jsonl" if a.pcm else "tracks_perf.jsonl")
    if not torch.cuda.is_available():
        raise SystemExit("perf_tracks.py needs a GPU: there is nothing to time without one")
    lens = lengths(a.seed, a.tracks)
    print("seed %d: %d tracks, %.1f to %.1f s, %.1f s in all" % (a.seed, len(lens), min(lens) / FS, max(lens) / FS, sum(lens) / FS), flush=True)
    if a.library:
        return library_main(a, lens)
    if a.shaped and not a.streamed:
        raise SystemExit("--shaped goes with --streamed")
    if a.normalized and not a.streamed:
        raise SystemExit("--normalized goes with --streamed")
    if a.streamed and a.normalized:
        return streamed_normalized_main(a, lens)
    if a.streamed:
        return streamed_shaped_main(a, lens) if a.shaped else streamed_main(a, lens)
    if a.pcm:
        return pcm_main(a, lens)
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
