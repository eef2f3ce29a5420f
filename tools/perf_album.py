"""The gapless stage pass (tracks_stage_album_device, DESIGN.md 11, "Gapless albums") against the stage pass it stands beside.

Workload: tools/perf_tracks.py's -- 64 stereo tracks, 44.1 kHz -> 48 kHz, lengths between 2 and 7 minutes drawn with its LCG from
--seed -- as 8 albums of 8 consecutive tracks, as float32 and as packed S24.  Every way is warmed up once, then timed `--rounds`
times (default 5, at least 5), the ways alternated within a round, between two HIP events on the current stream, the second of
which is synchronised on; medians and [min, max] are reported.  One JSON line per measurement, appended to --out (default
profiles/album_perf.jsonl) and printed.

Measurement 1, per source format {"what": "stage_album", "src_format"}: from the packed source to the rows.
  (a) linked     tracks_stage_album_device on the album plan: 8 x 7 joins copied from the neighbours, 16 album edges extrapolated;
  (b) unlinked   tracks_stage_device on tracks_plan of the same lengths: 128 edges extrapolated.  That call is not touched by
                 this feature, so it is the build before it.
  The linked pass does strictly less LPC work and writes the same bytes but for the rows' few extra frames (lead grows by the
  track's phase on the album's grid, under r1 = 147 frames).  The bar: median(a) <= median(b) + (max(b) - min(b)); "within_bar"
  says so.
Measurement 2 {"what": "convert_album"}, reported only: two whole conversions of the S24 tracks to S16 with dither on a fresh
  handle each, convert_tracks_to_pcm_device with and without gapless=.

  python tools/perf_album.py [--seed 20240229] [--tracks 64] [--albums 8] [--rounds 5] [--out FILE] [--skip-convert]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import foo_dsp_resampler_amd as F  # noqa: E402
from perf_mix import emit, spread  # noqa: E402
from perf_tracks import FO, FS, lengths, timed, to_s24  # noqa: E402

NCH = 2


def source(lens, fmt, seed):
    """packed stereo tracks at a quarter of full scale, made in pieces: float32 [total, 2] or uint8 [total, 6]"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    total = sum(lens)
    f32 = fmt == F.RRX_FMT_FLOAT
    out = torch.empty((total, NCH) if f32 else (total, NCH * 3), dtype=torch.float32 if f32 else torch.uint8, device="cuda")
    for pos in range(0, total, 1 << 25):
        n = min(1 << 25, total - pos)
        if f32:
            out[pos:pos + n] = (torch.rand((n, NCH), generator=g, device="cuda") - 0.5) * 0.5
        else:
            out[pos:pos + n] = to_s24(torch.randint(-(1 << 21), 1 << 21, (n, NCH), generator=g, device="cuda", dtype=torch.int32))
    return out


def groups_of(n, albums):
    per = -(-n // albums)
    return [t // per for t in range(n)]


def stage_main(a, lens, groups, name, fmt):
    plain = F.tracks_plan(FS, FO, lens)
    album = F.tracks_plan_album(FS, FO, lens, groups)
    n = len(lens)
    packed = source(lens, fmt, a.seed)
    ptab, atab, links = plain.to_device("cuda"), album.to_device("cuda"), album.links_to_device("cuda")
    prow = torch.empty((n, plain.row_frames, NCH), dtype=torch.float32, device="cuda")
    arow = torch.empty((n, album.row_frames, NCH), dtype=torch.float32, device="cuda")

    def linked():
        F.tracks_stage_album_device(packed, atab, links, FS, FO, album.row_frames, out=arow)

    def unlinked():
        F.tracks_stage_device(packed, ptab, FS, FO, plain.row_frames, out=prow)

    ways = {"linked": linked, "unlinked": unlinked}
    for fn in ways.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in ways}
    for _ in range(a.rounds):
        for k, fn in ways.items():
            ms[k].append(timed(fn)[0])
    none = F.RRX_LINK_NONE
    line = {"what": "stage_album", "src_format": name, "seed": a.seed, "tracks": n, "albums": len(set(groups)), "nch": NCH, "in_rate": FS,
            "out_rate": FO, "frames_total": sum(lens), "row_frames_linked": album.row_frames, "row_frames_unlinked": plain.row_frames,
            "source_bytes": packed.numel() * packed.element_size(), "row_bytes_linked": arow.numel() * 4, "row_bytes_unlinked": prow.numel() * 4,
            "edges_extrapolated_linked": int((album.links_array() == none).sum()), "edges_extrapolated_unlinked": 2 * n}
    spread(line, ms)
    lo, hi = line["unlinked_range_ms"]
    line.update({"linked_over_unlinked": round(line["linked_ms"] / line["unlinked_ms"], 3), "bar_ms": round(line["unlinked_ms"] + hi - lo, 3),
                 "within_bar": bool(line["linked_ms"] <= line["unlinked_ms"] + hi - lo), "rounds": a.rounds})
    emit(a, line)


def convert_main(a, lens, groups):
    n = len(lens)
    packed = source(lens, F.RRX_FMT_S24_3, a.seed)
    offs = [0]
    for k in lens:
        offs.append(offs[-1] + k)
    tracks = [packed[offs[t]:offs[t + 1]] for t in range(n)]
    kw = dict(dither=True, seed=a.seed)

    def convert(gapless):
        def run():
            r = F.Resampler(FS, FO, nch=NCH, nstreams=n)
            views, _, _ = r.convert_tracks_to_pcm_device(tracks, F.RRX_FMT_S16, gapless=gapless, **kw)
            r.close()
            return sum(y.shape[0] for y in views)
        return run

    ways = {"gapless": convert(groups), "islands": convert(None)}
    first = {k: round(timed(fn)[0], 2) for k, fn in ways.items()}
    ms = {k: [] for k in ways}
    frames = {}
    for _ in range(a.rounds):
        for k, fn in ways.items():
            t, frames[k] = timed(fn)
            ms[k].append(t)
    line = {"what": "convert_album", "src_format": "s24_3", "dst_format": "s16", "seed": a.seed, "tracks": n, "albums": len(set(groups)), "nch": NCH,
            "in_rate": FS, "out_rate": FO, "frames_total": sum(lens), "frames_out": frames, "first_call_ms": first}
    spread(line, ms)
    line.update({"gapless_over_islands": round(line["gapless_ms"] / line["islands_ms"], 3), "rounds": a.rounds})
    emit(a, line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=20240229)
    ap.add_argument("--tracks", type=int, default=64)
    ap.add_argument("--albums", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "album_perf.jsonl"))
    ap.add_argument("--skip-convert", action="store_true", help="measurement 1 only")
    a = ap.parse_args()
    if a.rounds < 5:
        raise SystemExit("at least five rounds: the spread is part of the result")
    if not torch.cuda.is_available():
        raise SystemExit("perf_album.py needs a GPU: there is nothing to time without one")
    lens = lengths(a.seed, a.tracks)
    groups = groups_of(len(lens), a.albums)
    print("seed %d: %d tracks in %d albums, %.1f to %.1f s, %.1f s in all" % (a.seed, len(lens), len(set(groups)), min(lens) / FS, max(lens) / FS,
                                                                          sum(lens) / FS), flush=True)
    for name, fmt in (("f32", F.RRX_FMT_FLOAT), ("s24_3", F.RRX_FMT_S24_3)):
        stage_main(a, lens, groups, name, fmt)
        torch.cuda.empty_cache()
    if not a.skip_convert:
        convert_main(a, lens, groups)


if __name__ == "__main__":
    main()
