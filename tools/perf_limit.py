"""The limiter (RRX_limit_device: detector, window minimum, box smoothing and product, three launches) against the true-peak pass
and the measure-only output stage on the same rows, and the true-peak overshoot it leaves.

Timing.  Input: the output tensor of one bench.py step of BASELINE configs 1 (256 streams x 2 channels) and 3 (16 streams x 32
channels), float32, as tools/perf_true_peak.py takes it.  The limiter runs out of place into a float32 tensor through the C ABI,
with its work buffer and results allocated once, at a ceiling of half the rows' sample peak (so that it has work to do), at
(lookahead, hold) = (72, 0) and (1024, 4096).  Everything runs on the same tensor in the same process, `--rounds` rounds
interleaved: in every round each candidate is warmed up `--warmup` times and then timed over `--steps` calls between two HIP
events on the stream.  The call reads the rows twice, writes them once and moves 32 bytes of work per frame.

Residuals.  Noise (sigma 0.25) and an fs/4 tone whose amplitude is modulated between 0.2 and 1.0, 48000 frames x 2 channels each,
under gains that push their true peak 3, 6 and 12 dB over a ceiling of 10 ** (-1 / 20), limited at lookahead 1, 72 and 256 (hold
0) into float64; the residual is max(true peak, sample peak) of the result over the ceiling, minus one.

One JSON line per shape and per residual table, appended to --out (default profiles/limit_perf.jsonl) and printed:

  {"config", "streams", "nch", "frames", "lookahead", "hold", "ms": median of the rounds, "ms_rounds", "gsamples_per_s",
   "true_peak_ms", "ratio_to_true_peak", "measure_only_ms", "ratio_to_measure_only", "limited_share", "steps", "warmup"}
  {"residuals": {signal: {"+3dB" ...: {lookahead: overshoot}}}}

  python tools/perf_limit.py [--configs 1,3] [--steps 20] [--warmup 3] [--rounds 3] [--out FILE] [--no-residuals]

Windows.  `--window W` times the window form instead (RRX_tracks_limit_window_device, DESIGN.md 11 "Windows with the limiter"): the
float32 output tensor of config 1 as whole-row tracks, limited in windows of W frames -- every window from the frames of the rows
within its reach, into one window buffer -- against RRX_tracks_limit_device on the same rows in the same run, interleaved as above.
A window evaluates the detector on back + ahead frames more than it emits, so the expectation is the whole-row time plus the
detector's time * (back + ahead) / W plus three launches a window; the true-peak pass on the same rows stands in for the detector,
which runs the same filter.  One line per (lookahead, hold), appended to profiles/limit_window_perf.jsonl:

  {"config", "streams", "nch", "frames", "window", "windows", "lookahead", "hold", "back", "ahead", "whole_ms", "window_ms", "ms_rounds",
   "whole_ms_rounds", "ratio", "true_peak_ms", "expected_ms": whole_ms + true_peak_ms * (back + ahead) / window, "excess_ms",
   "excess_us_per_window", "steps", "warmup"}

  python tools/perf_limit.py --window 4354 [--steps 20] [--warmup 3] [--rounds 3] [--out FILE]

Release.  `--release` times RRX_tracks_limit_release_device ("Limiter: release") against RRX_tracks_limit_device at
the same lookahead and hold, on the first 64 streams of config 1's float32 output tensor as 64 whole-row stereo tracks, both out
of place into one float32 tensor -- same rows, same run, interleaved as above -- under the pole of a 100 ms release
at 48 kHz, in blocks of `--block` entries (default 1024).  By bytes the three launches of the release add two reads and one write
of m, 24 bytes a frame, to the 56 bytes a stereo float32 frame costs the limiter: about 1.4 times.  One line per (lookahead,
hold), appended to profiles/limit_release_perf.jsonl:

  {"config", "tracks", "nch", "frames", "lookahead", "hold", "release", "block", "blocks_per_track", "limit_ms", "release_ms",
   "limit_ms_rounds", "release_ms_rounds", "ratio", "extra_ms", "extra_gbytes_per_s": 24 bytes a frame over extra_ms, "steps", "warmup"}

  python tools/perf_limit.py --release [--block 1024] [--steps 20] [--warmup 3] [--rounds 3] [--out FILE]

Release by windows.  `--window W --release` times RRX_tracks_limit_release_window_device ("Windows with the limiter's
release") on the 64-track shape above, over ascending windows of W frames, every window given the state of the one before and
read from the rows within its reach as under `--window`, against two baselines in the same run, interleaved as above:
RRX_tracks_limit_window_device over the same windows, and the whole-row RRX_tracks_limit_release_device.  One line per
(lookahead, hold), appended to profiles/limit_release_window_perf.jsonl:

  {"config", "tracks", "nch", "frames", "window", "windows", "lookahead", "hold", "release", "block", "release_window_ms",
   "window_ms", "whole_release_ms", the three "..._rounds", "ratio_to_window", "ratio_to_whole_release",
   "extra_us_per_window": (release_window_ms - window_ms) / windows, "steps", "warmup"}

  python tools/perf_limit.py --window 4096 --release [--block 1024] [--steps 20] [--warmup 3] [--rounds 3] [--out FILE]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import foo_dsp_resampler_amd as F  # noqa: E402
from perf_finish import step_tensor, timed  # noqa: E402

PAIRS = ((72, 0), (1024, 4096))


def one_config(k, steps, warmup, rounds):
    stream = torch.cuda.Stream()
    x, _ = step_tensor(k, stream)
    S, frames, nch = x.shape
    phases, taps, coefs = F.TRUE_PEAK_FILTERS["bs1770"]
    co = (C.c_double * len(coefs))(*coefs)
    with torch.cuda.stream(stream):
        tp = torch.zeros((S, nch), dtype=torch.float64, device="cuda")
        pk = torch.zeros((S, nch), dtype=torch.float64, device="cuda")
        pk2 = torch.zeros((S, nch), dtype=torch.float64, device="cuda")
        cl = torch.zeros((S, nch), dtype=torch.int64, device="cuda")
        out = torch.empty_like(x)
        red = torch.ones((S,), dtype=torch.float64, device="cuda")
        lim = torch.zeros((S,), dtype=torch.int64, device="cuda")
        work = torch.empty((F.limit_work_doubles(S, frames, taps, 1024),), dtype=torch.float64, device="cuda")
        ceiling = 0.5 * float(x.abs().max())
    stream.synchronize()

    def limiter(L, H):
        def call():
            F.ratelib._check(F.lib().RRX_limit_device(-1, C.c_void_p(stream.cuda_stream), F.RRX_FMT_FLOAT, C.c_void_p(x.data_ptr()), frames,
                                                      F.RRX_FMT_FLOAT, C.c_void_p(out.data_ptr()), frames, S, frames, nch, None, ceiling,
                                                      C.cast(co, C.c_void_p), phases, taps, L, H, C.c_void_p(red.data_ptr()),
                                                      C.c_void_p(lim.data_ptr()), C.c_void_p(work.data_ptr()), work.numel()), "RRX_limit_device")
        return call

    def true_peak():
        return F.true_peak_device(x, true_peak=tp, peak=pk, stream=stream)

    def measure_only():
        return F.finish_device(x, None, peak=pk2, clipped=cl, stream=stream)

    calls = [limiter(L, H) for L, H in PAIRS]
    ms, tms, mms = [[] for _ in PAIRS], [], []
    for _ in range(rounds):
        for i, call in enumerate(calls):
            ms[i].append(timed(stream, call, steps, warmup))
        tms.append(timed(stream, true_peak, steps, warmup))
        mms.append(timed(stream, measure_only, steps, warmup))
    t, mo = statistics.median(tms), statistics.median(mms)
    lines = []
    for i, (L, H) in enumerate(PAIRS):
        with torch.cuda.stream(stream):
            lim.zero_()
            calls[i]()
            share = float(lim.sum()) / (S * frames)
        stream.synchronize()
        m = statistics.median(ms[i])
        lines.append({"config": k, "streams": S, "nch": nch, "frames": frames, "lookahead": L, "hold": H, "ms": round(m, 4),
                      "ms_rounds": [round(v, 4) for v in ms[i]], "gsamples_per_s": round(S * frames * nch / m / 1e6, 2),
                      "true_peak_ms": round(t, 4), "ratio_to_true_peak": round(m / t, 2), "measure_only_ms": round(mo, 4),
                      "ratio_to_measure_only": round(m / mo, 2), "limited_share": round(share, 4), "steps": steps, "warmup": warmup})
    return lines


def window_config(k, W, steps, warmup, rounds):
    stream = torch.cuda.Stream()
    x, _ = step_tensor(k, stream)
    S, frames, nch = x.shape
    phases, taps, coefs = F.TRUE_PEAK_FILTERS["bs1770"]
    co = (C.c_double * len(coefs))(*coefs)
    table = np.zeros((S, 6), np.uint64)  # only the output slices are looked at: every track is its whole row
    table[:, 4] = frames
    with torch.cuda.stream(stream):
        # the rows with one row of slack behind them: a window's buffer begins buf_first frames into the rows, at the rows' own pitch
        mem = torch.zeros((S * frames * nch + frames * nch,), dtype=torch.float32, device="cuda")
        rows = mem[:S * frames * nch].view(S, frames, nch)
        rows.copy_(x)
        d_table = torch.from_numpy(table.view(np.int64)).cuda()
        out = torch.empty_like(x)
        wout = torch.empty((S, W, nch), dtype=torch.float32, device="cuda")
        tp = torch.zeros((S, nch), dtype=torch.float64, device="cuda")
        pk = torch.zeros((S, nch), dtype=torch.float64, device="cuda")
        red = torch.ones((S,), dtype=torch.float64, device="cuda")
        lim = torch.zeros((S,), dtype=torch.int64, device="cuda")
        work = torch.empty((max(F.limit_work_doubles(S, frames, taps, 1024), F.tracks_limit_window_work_doubles(S, W, taps, 1024, 4096)),),
                           dtype=torch.float64, device="cuda")
        ceiling = 0.5 * float(x.abs().max())
    stream.synchronize()
    windows = [(first, min(W, frames - first)) for first in range(0, frames, W)]

    def whole(L, H):
        def call():
            F.ratelib._check(F.lib().RRX_tracks_limit_device(-1, C.c_void_p(stream.cuda_stream), C.c_void_p(d_table.data_ptr()), S, nch, F.RRX_FMT_FLOAT,
                                                             C.c_void_p(rows.data_ptr()), F.RRX_FMT_FLOAT, C.c_void_p(out.data_ptr()), frames, None,
                                                             ceiling, C.cast(co, C.c_void_p), phases, taps, L, H, C.c_void_p(red.data_ptr()),
                                                             C.c_void_p(lim.data_ptr()), C.c_void_p(work.data_ptr()), work.numel()),
                             "RRX_tracks_limit_device")
        return call

    def by_windows(L, H):
        back, ahead = F.limit_window_reach(L, H)

        def call():
            for first, n in windows:
                b0, b1 = max(0, first - back), min(frames, first + n + ahead)
                F.ratelib._check(F.lib().RRX_tracks_limit_window_device(
                    -1, C.c_void_p(stream.cuda_stream), C.c_void_p(d_table.data_ptr()), S, nch, F.RRX_FMT_FLOAT,
                    C.c_void_p(rows.data_ptr() + b0 * nch * 4), frames, b0, b1 - b0, frames, first, n, F.RRX_FMT_FLOAT, C.c_void_p(wout.data_ptr()),
                    W, None, ceiling, C.cast(co, C.c_void_p), phases, taps, L, H, C.c_void_p(red.data_ptr()), C.c_void_p(lim.data_ptr()),
                    C.c_void_p(work.data_ptr()), work.numel()), "RRX_tracks_limit_window_device")
        return call

    def true_peak():
        return F.true_peak_device(rows, true_peak=tp, peak=pk, stream=stream)

    lines = []
    for L, H in PAIRS:
        back, ahead = F.limit_window_reach(L, H)
        a, b, wms, wins, tms = whole(L, H), by_windows(L, H), [], [], []
        for _ in range(rounds):
            wms.append(timed(stream, a, steps, warmup))
            wins.append(timed(stream, b, steps, warmup))
            tms.append(timed(stream, true_peak, steps, warmup))
        m, v, t = statistics.median(wms), statistics.median(wins), statistics.median(tms)
        expected = m + t * (back + ahead) / W
        lines.append({"config": k, "streams": S, "nch": nch, "frames": frames, "window": W, "windows": len(windows), "lookahead": L, "hold": H,
                      "back": back, "ahead": ahead, "whole_ms": round(m, 4), "window_ms": round(v, 4), "ms_rounds": [round(u, 4) for u in wins],
                      "whole_ms_rounds": [round(u, 4) for u in wms], "ratio": round(v / m, 3), "true_peak_ms": round(t, 4),
                      "expected_ms": round(expected, 4), "excess_ms": round(v - expected, 4),
                      "excess_us_per_window": round((v - expected) * 1000.0 / len(windows), 2), "steps": steps, "warmup": warmup})
    return lines


def release_config(k, tracks, block, steps, warmup, rounds):
    stream = torch.cuda.Stream()
    x, _ = step_tensor(k, stream)
    with torch.cuda.stream(stream):
        rows = x[:tracks].contiguous()
    del x
    S, frames, nch = rows.shape
    phases, taps, coefs = F.TRUE_PEAK_FILTERS["bs1770"]
    co = (C.c_double * len(coefs))(*coefs)
    table = np.zeros((S, 6), np.uint64)  # only the output slices are looked at: every track is its whole row
    table[:, 4] = frames
    pole = F.limit_release_coef(100.0, 48000)
    with torch.cuda.stream(stream):
        d_table = torch.from_numpy(table.view(np.int64)).cuda()
        out = torch.empty_like(rows)
        red = torch.ones((S,), dtype=torch.float64, device="cuda")
        lim = torch.zeros((S,), dtype=torch.int64, device="cuda")
        work = torch.empty((F.limit_release_work_doubles(S, frames, taps, 1024, block),), dtype=torch.float64, device="cuda")
        ceiling = 0.5 * float(rows.abs().max())
    stream.synchronize()

    def plain(L, H):
        def call():
            F.ratelib._check(F.lib().RRX_tracks_limit_device(-1, C.c_void_p(stream.cuda_stream), C.c_void_p(d_table.data_ptr()), S, nch, F.RRX_FMT_FLOAT,
                                                             C.c_void_p(rows.data_ptr()), F.RRX_FMT_FLOAT, C.c_void_p(out.data_ptr()), frames, None,
                                                             ceiling, C.cast(co, C.c_void_p), phases, taps, L, H, C.c_void_p(red.data_ptr()),
                                                             C.c_void_p(lim.data_ptr()), C.c_void_p(work.data_ptr()), work.numel()),
                             "RRX_tracks_limit_device")
        return call

    def released(L, H):
        def call():
            F.ratelib._check(F.lib().RRX_tracks_limit_release_device(
                -1, C.c_void_p(stream.cuda_stream), C.c_void_p(d_table.data_ptr()), S, nch, F.RRX_FMT_FLOAT, C.c_void_p(rows.data_ptr()),
                F.RRX_FMT_FLOAT, C.c_void_p(out.data_ptr()), frames, None, ceiling, C.cast(co, C.c_void_p), phases, taps, L, H, pole, block,
                C.c_void_p(red.data_ptr()), C.c_void_p(lim.data_ptr()), C.c_void_p(work.data_ptr()), work.numel()), "RRX_tracks_limit_release_device")
        return call

    lines = []
    for L, H in PAIRS:
        a, b, pms, rms = plain(L, H), released(L, H), [], []
        for _ in range(rounds):
            pms.append(timed(stream, a, steps, warmup))
            rms.append(timed(stream, b, steps, warmup))
        p, r = statistics.median(pms), statistics.median(rms)
        lines.append({"config": k, "tracks": S, "nch": nch, "frames": frames, "lookahead": L, "hold": H, "release": pole, "block": block,
                      "blocks_per_track": -(-(frames + L - 1) // block), "limit_ms": round(p, 4), "release_ms": round(r, 4),
                      "limit_ms_rounds": [round(v, 4) for v in pms], "release_ms_rounds": [round(v, 4) for v in rms], "ratio": round(r / p, 3),
                      "extra_ms": round(r - p, 4), "extra_gbytes_per_s": round(24.0 * S * frames / (r - p) / 1e6, 1) if r > p else None,
                      "steps": steps, "warmup": warmup})
    return lines


def release_window_config(k, tracks, W, block, steps, warmup, rounds):
    stream = torch.cuda.Stream()
    x, _ = step_tensor(k, stream)
    S, frames, nch = tracks, x.shape[1], x.shape[2]
    phases, taps, coefs = F.TRUE_PEAK_FILTERS["bs1770"]
    co = (C.c_double * len(coefs))(*coefs)
    table = np.zeros((S, 6), np.uint64)  # only the output slices are looked at: every track is its whole row
    table[:, 4] = frames
    pole = F.limit_release_coef(100.0, 48000)
    with torch.cuda.stream(stream):
        # the rows with one row of slack behind them: a window's buffer begins buf_first frames into the rows, at the rows' own pitch
        mem = torch.zeros((S * frames * nch + frames * nch,), dtype=torch.float32, device="cuda")
        rows = mem[:S * frames * nch].view(S, frames, nch)
        rows.copy_(x[:S])
        ceiling = 0.5 * float(rows.abs().max())
        del x
        d_table = torch.from_numpy(table.view(np.int64)).cuda()
        out = torch.empty_like(rows)
        wout = torch.empty((S, W, nch), dtype=torch.float32, device="cuda")
        red = torch.ones((S,), dtype=torch.float64, device="cuda")
        lim = torch.zeros((S,), dtype=torch.int64, device="cuda")
        states = [torch.zeros((S, F.RRX_LIMIT_RELEASE_WIN_STATE), dtype=torch.float64, device="cuda") for _ in range(2)]
        work = torch.empty((max(F.limit_release_work_doubles(S, frames, taps, 1024, block),
                                F.tracks_limit_release_window_work_doubles(S, W, taps, 1024, 4096, block)),), dtype=torch.float64, device="cuda")
    stream.synchronize()
    windows = [(first, min(W, frames - first)) for first in range(0, frames, W)]
    sp = C.c_void_p(stream.cuda_stream)

    def by_windows(L, H, release):
        back, ahead = F.limit_window_reach(L, H)

        def call():
            for i, (first, n) in enumerate(windows):
                b0, b1 = max(0, first - back), min(frames, first + n + ahead)
                head = (-1, sp, C.c_void_p(d_table.data_ptr()), S, nch, F.RRX_FMT_FLOAT, C.c_void_p(rows.data_ptr() + b0 * nch * 4), frames, b0,
                        b1 - b0, frames, first, n, F.RRX_FMT_FLOAT, C.c_void_p(wout.data_ptr()), W, None, ceiling, C.cast(co, C.c_void_p), phases,
                        taps, L, H)
                tail = (C.c_void_p(red.data_ptr()), C.c_void_p(lim.data_ptr()), C.c_void_p(work.data_ptr()), work.numel())
                if release:
                    state = (pole, block, C.c_void_p(states[i % 2].data_ptr()) if i else None, C.c_void_p(states[1 - i % 2].data_ptr()))
                    F.ratelib._check(F.lib().RRX_tracks_limit_release_window_device(*(head + state + tail)), "RRX_tracks_limit_release_window_device")
                else:
                    F.ratelib._check(F.lib().RRX_tracks_limit_window_device(*(head + tail)), "RRX_tracks_limit_window_device")
        return call

    def whole(L, H):
        def call():
            F.ratelib._check(F.lib().RRX_tracks_limit_release_device(
                -1, sp, C.c_void_p(d_table.data_ptr()), S, nch, F.RRX_FMT_FLOAT, C.c_void_p(rows.data_ptr()), F.RRX_FMT_FLOAT,
                C.c_void_p(out.data_ptr()), frames, None, ceiling, C.cast(co, C.c_void_p), phases, taps, L, H, pole, block,
                C.c_void_p(red.data_ptr()), C.c_void_p(lim.data_ptr()), C.c_void_p(work.data_ptr()), work.numel()), "RRX_tracks_limit_release_device")
        return call

    lines = []
    for L, H in PAIRS:
        a, b, c, rw, pw, wr = by_windows(L, H, True), by_windows(L, H, False), whole(L, H), [], [], []
        for _ in range(rounds):
            rw.append(timed(stream, a, steps, warmup))
            pw.append(timed(stream, b, steps, warmup))
            wr.append(timed(stream, c, steps, warmup))
        r, p, w = statistics.median(rw), statistics.median(pw), statistics.median(wr)
        lines.append({"config": k, "tracks": S, "nch": nch, "frames": frames, "window": W, "windows": len(windows), "lookahead": L, "hold": H,
                      "release": pole, "block": block, "release_window_ms": round(r, 4), "window_ms": round(p, 4), "whole_release_ms": round(w, 4),
                      "release_window_ms_rounds": [round(v, 4) for v in rw], "window_ms_rounds": [round(v, 4) for v in pw],
                      "whole_release_ms_rounds": [round(v, 4) for v in wr], "ratio_to_window": round(r / p, 3),
                      "ratio_to_whole_release": round(r / w, 3), "extra_us_per_window": round((r - p) * 1000.0 / len(windows), 2),
                      "steps": steps, "warmup": warmup})
    return lines


def residuals():
    ceiling = 10.0 ** (-1.0 / 20.0)
    gen = torch.Generator(device="cuda").manual_seed(7)
    n = torch.arange(48000, device="cuda", dtype=torch.float64)
    tone = torch.sin(2 * math.pi * n / 4 + math.pi / 4) * (0.6 + 0.4 * torch.sin(2 * math.pi * n / 1531.0))
    signals = {"noise": torch.randn((48000, 2), generator=gen, device="cuda", dtype=torch.float64) * 0.25,
               "modulated_fs4_tone": torch.stack([tone, tone.roll(1)], dim=1).contiguous()}
    table = {}
    for name, x in signals.items():
        level = float(torch.maximum(*F.true_peak_device(x)[:2]).max())
        table[name] = {}
        for db in (3, 6, 12):
            gain = ceiling * 10.0 ** (db / 20.0) / level
            row = {}
            for L in (1, 72, 256):
                y, _, _ = F.limit_device(x, ceiling, gain=gain, lookahead=L, hold=0)
                row[str(L)] = float(torch.maximum(*F.true_peak_device(y)[:2]).max()) / ceiling - 1.0
            table[name]["+%ddB" % db] = row
    return {"residuals": table, "ceiling": ceiling, "frames": 48000, "nch": 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="1,3")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-residuals", action="store_true")
    ap.add_argument("--window", type=int, default=0, help="time the window form in windows of this many frames (config 1) instead")
    ap.add_argument("--release", action="store_true", help="time the limiter with a release against the limiter, on 64 stereo tracks")
    ap.add_argument("--block", type=int, default=1024, help="entries of a block of the release's scan")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_limit.py needs a GPU: there is nothing to time without one")
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "limit_release_window_perf.jsonl" if a.release and a.window else
                             "limit_release_perf.jsonl" if a.release else "limit_window_perf.jsonl" if a.window else "limit_perf.jsonl")
    lines = []
    if a.release and a.window:
        if a.window < 1:
            raise SystemExit("--window is a positive frame count")
        lines += release_window_config(1, 64, a.window, a.block, a.steps, a.warmup, a.rounds)
    elif a.release:
        lines += release_config(1, 64, a.block, a.steps, a.warmup, a.rounds)
    elif a.window:
        if a.window < 1:
            raise SystemExit("--window is a positive frame count")
        lines += window_config(1, a.window, a.steps, a.warmup, a.rounds)
    else:
        for k in [int(v) for v in a.configs.split(",") if v]:
            lines += one_config(k, a.steps, a.warmup, a.rounds)
        if not a.no_residuals:
            lines.append(residuals())
    for line in lines:
        text = json.dumps(line)
        print(text, flush=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
