"""Ragged track batches by windows on the device (csrc/tracks.hip; DESIGN.md 11, "Windows"): tracks_stage_window_device,
tracks_finish_window_device and Resampler.convert_tracks_to_pcm_streamed.

The bar throughout is EQUALITY of bits with the whole-row calls, which tests/test_gpu_tracks.py and tests/test_gpu_tracks_pcm.py
hold to today's per-track calls: a set of windows that covers the rows gives the rows of tracks_stage_device, the bytes, peaks
and clip counts of tracks_finish_device, and the streamed conversion gives convert_tracks_to_pcm_device's result -- in memory
that does not grow with the longest track, which the last test measures.  The wrong tables are a clamp at work, not a fault
provoked: sentinels and guard bytes around every buffer are looked at."""
import ctypes as C
import functools

import numpy as np
import pytest

import foo_dsp_resampler_amd as F
from test_gpu_tracks import (GUARD, NB, R_OUT, SEED, SENTINEL, SLICES, bits, finish_rows, finish_table, ragged_finish, same_bits)
from test_gpu_tracks_pcm import BITS, to_raw
from test_plugin_layer import music_like

pytestmark = pytest.mark.gpu

FS, FO = 44100, 48000
LENGTHS = (0, 40, 64, 65, 100, 1500, 2206, 5000)
R = 5000 + 2 * 2205                                           # row_frames of LENGTHS at 44.1k -> 48k
LEAD = 2205
# cuts of the irregular partition: next to the row's ends, around the lead, and around the end of the track and of the forward
# extension of the 1500- and the 5000-frame track (whose extension ends with the row)
CUTS = sorted({c for c in [1, 2204, 2205, 2206, R - 1] + [LEAD + n + d for n in (1500, 5000) for d in (-1, 0)] +
               [LEAD + n + LEAD + d for n in (1500, 5000) for d in (-1, 0, 1)] if 0 < c < R})
SRC = {"f32": None, "s16": F.RRX_FMT_S16, "s24": F.RRX_FMT_S24_3, "s32": F.RRX_FMT_S32}


def even(step, n=R):
    return [(a, min(step, n - a)) for a in range(0, n, step)]


def irregular(cuts=CUTS, n=R):
    edges = [0] + list(cuts) + [n]
    return [(a, b - a) for a, b in zip(edges, edges[1:])]


PARTITIONS = {"one": even(R), "257": even(257), "2205": even(2205), "4099": even(4099), "irregular": irregular()}


def test_the_partitions_are_what_they_are_meant_to_be():
    plan = F.tracks_plan(FS, FO, LENGTHS)
    assert plan.row_frames == R and int(plan.table[5].lead) == LEAD
    for name, part in PARTITIONS.items():
        assert part[0][0] == 0 and sum(n for _, n in part) == R and all(a + n == b for (a, n), (b, _) in zip(part, part[1:])), name
    firsts = {a % 4 for part in PARTITIONS.values() for a, _ in part}
    assert firsts == {0, 1, 2, 3}
    assert {LEAD + 1500 - 1, LEAD + 1500, 2 * LEAD + 1500 - 1, 2 * LEAD + 1500, 2 * LEAD + 1500 + 1, LEAD + 5000, R - 1} <= set(CUTS)


@functools.lru_cache(maxsize=None)
def source(kind, nch, lengths=LENGTHS):
    """the packed source as the numpy array the call takes (float32, int16, int32 [frames, nch], or uint8 [frames, nch * 3]); read-only"""
    xs = [music_like(n, nch, FS, 50 + i) if n else np.zeros((0, nch), np.float32) for i, n in enumerate(lengths)]
    x = np.concatenate(xs)
    if SRC[kind] is not None:
        x = to_raw(np.rint(x.astype(np.float64) * 0.5 * 2.0 ** BITS[SRC[kind]]).astype(np.int64), SRC[kind])
    x.setflags(write=False)
    return x


def whole_rows(packed, tab, rows):
    """tracks_stage_device, the reference: numpy [ntracks, rows, nch]"""
    return F.tracks_stage_device(packed, tab, FS, FO, rows).cpu().numpy()


def stage_windows(packed, tab, rows, part, stream=None):
    """tracks_stage_window_device for every window of `part`, each into its own slot of one buffer: 16 sentinel frames, the window
    rows at a pitch of win_frames + 3, 16 sentinel frames.  The sentinels and the 3 gap frames of every row must be untouched;
    returns {(win_first, win_frames): numpy [ntracks, win_frames, nch]}."""
    import torch
    n = tab.shape[0]
    nch = packed.shape[1] // 3 if packed.dtype == torch.uint8 else packed.shape[1]
    size = [16 + n * (wn + 3) + 16 for _, wn in part]
    at = np.concatenate([[0], np.cumsum(size)])
    buf = torch.full((int(at[-1]), nch), SENTINEL, dtype=torch.float32, device="cuda")
    keep = packed.clone()
    for (wf, wn), o in zip(part, at):
        win = buf[o + 16:o + 16 + n * (wn + 3)].view(n, wn + 3, nch)
        got = F.tracks_stage_window_device(packed, tab, FS, FO, rows, wf, wn, out=win, stream=stream)
        assert got is win
    if stream is not None:
        stream.synchronize()
    assert torch.equal(packed.view(torch.uint8), keep.view(torch.uint8)), "the packed source was written"
    host = buf.cpu().numpy()
    out = {}
    for (wf, wn), o, sz in zip(part, at, size):
        slot = host[o:o + sz]
        assert (slot[:16] == SENTINEL).all() and (slot[-16:] == SENTINEL).all(), ("frames outside the window buffer were written", wf, wn)
        win = slot[16:-16].reshape(n, wn + 3, nch)
        assert (win[:, wn:] == SENTINEL).all(), ("frames between win_frames and win_stride were written", wf, wn)
        out[(wf, wn)] = win[:, :wn]
    return out


def assemble(wins, n, rows, nch):
    got = np.full((n, rows, nch), SENTINEL, np.float32)
    for (wf, wn), w in wins.items():
        got[:, wf:wf + wn] = w
    return got


@pytest.mark.parametrize("nch", [1, 2, 3])
@pytest.mark.parametrize("kind", list(SRC))
def test_stage_windows_are_the_rows_bit_for_bit(kind, nch):
    import torch
    packed = torch.from_numpy(np.array(source(kind, nch))).cuda()
    tab = F.tracks_plan(FS, FO, LENGTHS).to_device("cuda")
    want = whole_rows(packed, tab, R)
    assert not (want == SENTINEL).any()
    for name, part in PARTITIONS.items():
        got = assemble(stage_windows(packed, tab, R, part), len(LENGTHS), R, nch)
        diff = bits(got) != bits(want)
        print(kind, nch, name, "differing samples:", int(diff.sum()), "of", diff.size)
        assert not diff.any(), (kind, nch, name, np.argwhere(diff)[:4])


def test_single_frame_windows_at_every_cut():
    import torch
    packed = torch.from_numpy(np.array(source("s24", 3))).cuda()
    tab = F.tracks_plan(FS, FO, LENGTHS).to_device("cuda")
    want = whole_rows(packed, tab, R)
    points = sorted({0, R - 1} | {c + d for c in CUTS for d in (-1, 0) if 0 <= c + d < R})
    wins = stage_windows(packed, tab, R, [(c, 1) for c in points])
    for (wf, wn), w in wins.items():
        assert np.array_equal(bits(w), bits(want[:, wf:wf + 1])), wf


def test_stage_windows_with_a_nan_in_one_channel():
    import torch
    lengths = [100, 1500, 5000]
    tracks = [music_like(n, 2, FS, 60 + i) for i, n in enumerate(lengths)]
    tracks[1][1500 - 1 - 16, 0] = np.nan                     # inside the last 32 frames, and (prime == frames) inside the backward base too
    packed = torch.from_numpy(np.concatenate(tracks)).cuda()
    tab = F.tracks_plan(FS, FO, lengths).to_device("cuda")
    want = whole_rows(packed, tab, R)
    assert np.isnan(want[1, :LEAD, 0]).all() and np.isnan(want[1, LEAD + 1500:2 * LEAD + 1500, 0]).all() and np.isfinite(want[1, :, 1]).all()
    for part in (even(2205), irregular()):
        got = assemble(stage_windows(packed, tab, R, part), 3, R, 2)
        assert same_bits(got, want)
        assert np.array_equal(np.isnan(got), np.isnan(want))


def test_stage_windows_on_a_side_stream():
    import torch
    packed = torch.from_numpy(np.array(source("s16", 2))).cuda()
    tab = F.tracks_plan(FS, FO, LENGTHS).to_device("cuda")
    want = whole_rows(packed, tab, R)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    dev = torch.cuda.current_device()
    with torch.cuda.stream(side):                            # the buffers are filled on the side stream
        wins = stage_windows(packed, tab, R, even(2205), stream=side)
    assert torch.cuda.current_device() == dev
    assert np.array_equal(bits(assemble(wins, len(LENGTHS), R, 2)), bits(want))


def test_stage_windows_under_a_wrong_table_are_the_rows_under_it():
    import torch
    lengths = [300, 200, 400]
    packed = torch.from_numpy(np.concatenate([music_like(n, 2, FS, 80 + i) for i, n in enumerate(lengths)])).cuda()
    plan = F.tracks_plan(FS, FO, lengths)
    rows = plan.row_frames
    tables = []
    for bad in ((2 ** 40, 200, 2205, 0, 0, 0), (300, 2 ** 40, 2205, 0, 0, 0), (300, 200, 2 ** 62, 0, 0, 0),
                (2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1, 0, 0, 0), (850, 200, 0, 0, 0, 0), (300, 20, 2205, 0, 0, 0)):
        tab = plan.array()
        tab[1] = bad
        tables.append(tab)
    tables.append(np.ascontiguousarray(plan.array()[::-1]))
    for tab in tables:
        dtab = torch.from_numpy(tab.view(np.int64)).cuda()
        want = whole_rows(packed, dtab, rows)
        for part in (even(257, rows), irregular([1, 199, 200, 201, 2204, 2205, 2206, 2405, 2406, rows - 1], rows)):
            got = assemble(stage_windows(packed, dtab, rows, part), 3, rows, 2)
            assert np.array_equal(bits(got), bits(want)), tab[1]


def test_an_empty_window_is_ok_and_writes_nothing():
    import torch
    plan = F.tracks_plan(FS, FO, [100, 300])
    table = plan.to_device("cuda")
    packed = torch.zeros((400, 2), dtype=torch.float32, device="cuda")
    win = torch.full((2, 8, 2), SENTINEL, dtype=torch.float32, device="cuda")
    dst = torch.full((plan.dst_total, 2), 0x5a5a, dtype=torch.int16, device="cuda")
    stats = torch.zeros((2, 2), dtype=torch.int64, device="cuda")
    F.tracks_stage_window_device(packed, table, FS, FO, plan.row_frames, 0, 1, out=win)     # (initialises the library)
    win.fill_(SENTINEL)
    vp, L = C.c_void_p, F.lib()
    for first in (0, 17, plan.row_frames):
        assert L.RRX_tracks_stage_window_device(-1, None, FS, FO, vp(table.data_ptr()), 2, 2, F.RRX_FMT_FLOAT, vp(packed.data_ptr()), 400,
                                                plan.row_frames, first, 0, vp(win.data_ptr()), 8) == 0
        assert L.RRX_tracks_finish_window_device(-1, None, vp(table.data_ptr()), 2, 2, F.RRX_FMT_FLOAT, vp(win.data_ptr()), 8, plan.out_row_cap,
                                                 first, 0, F.RRX_FMT_S16, vp(dst.data_ptr()), plan.dst_total, None, 0, 0, vp(stats.data_ptr()),
                                                 vp(stats.data_ptr())) == 0
    ndev = torch.cuda.device_count()
    assert L.RRX_tracks_stage_window_device(ndev, None, FS, FO, vp(table.data_ptr()), 2, 2, F.RRX_FMT_FLOAT, vp(packed.data_ptr()), 400,
                                            plan.row_frames, 0, 8, vp(win.data_ptr()), 8) == 6           # a device the process does not have
    torch.cuda.synchronize()
    assert (win == SENTINEL).all() and (dst == 0x5a5a).all() and not stats.any()


# ------------------------------------------------------------------------------------------------------------- ragged finish

def fin_even(step):
    return even(step, R_OUT)


FIN_PARTITIONS = {"one": fin_even(R_OUT), "7": fin_even(7), "333": fin_even(333),
                  "16 singles": [(a, 1) for a in range(16)] + [(16, R_OUT - 16)], "333 reversed": fin_even(333)[::-1]}
POISON = 1e30                                                 # in the frames between win_frames and win_stride: never read


def finish_windows(x, tab, dst_total, fmt, gain, dith, part, pre=64, post=64):
    """tracks_finish_window_device for every window of `part`, accumulating into one destination `pre` bytes into a guarded byte
    buffer and one pair of statistics; returns what ragged_finish (tests/test_gpu_tracks.py) returns for the whole-row call"""
    import torch
    n, rows_n, nch = x.shape
    rows = torch.from_numpy(np.array(x)).cuda()
    table = torch.from_numpy(tab.view(np.int64)).cuda()
    g = None if gain is None else torch.from_numpy(np.ascontiguousarray(gain, dtype=np.float64)).cuda()
    out = buf = None
    if fmt is not None:
        nbytes = dst_total * nch * NB[fmt]
        buf = torch.full((pre + nbytes + post,), GUARD, dtype=torch.uint8, device="cuda")
        out = buf[pre:pre + nbytes]
        out = out.view(dst_total, nch * 3) if fmt == F.RRX_FMT_S24_3 else out.view(torch.int16 if fmt == F.RRX_FMT_S16 else torch.int32).view(dst_total, nch)
    pk = cl = None
    for wf, wn in part:
        win = torch.full((n, wn + 2, nch), POISON, dtype=rows.dtype, device="cuda")
        win[:, :wn] = rows[:, wf:wf + wn]
        o, p, c = F.tracks_finish_window_device(win, table, rows_n, wf, wn, fmt, dst_total, gain=g, dither=dith, seed=SEED, out=out, peak=pk, clipped=cl)
        assert o is out and (pk is None or (p is pk and c is cl))
        pk, cl = p, c
    raw = None
    if buf is not None:
        host = buf.cpu().numpy()
        assert (host[:pre] == GUARD).all() and (host[pre + nbytes:] == GUARD).all(), "bytes around the destination were written"
        raw = host[pre:pre + nbytes]
    return raw, pk.cpu().numpy().view(np.uint64), cl.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("nch", [1, 2, 3])
@pytest.mark.parametrize("double", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("fmt", [F.RRX_FMT_S16, F.RRX_FMT_S24_3, F.RRX_FMT_S32], ids=["s16", "s24", "s32"])
def test_finish_windows_are_the_whole_row_call(fmt, double, nch):
    x = finish_rows(nch, fmt, double)
    tab, dst_total = finish_table()
    gains = 0.5 + 0.4 * np.arange(len(SLICES))
    pre = 65 if fmt == F.RRX_FMT_S24_3 else 66 if fmt == F.RRX_FMT_S16 else 64    # the odd byte offsets even frames never give
    want = ragged_finish(x, tab, dst_total, fmt, gains, True, pre=pre)
    assert want[2].sum() > 0 and not (want[0] == GUARD).all()
    for name, part in FIN_PARTITIONS.items():
        assert sorted(part)[0][0] == 0 and sum(n for _, n in part) == R_OUT
        got = finish_windows(x, tab, dst_total, fmt, gains, True, part, pre=pre)
        assert np.array_equal(got[0], want[0]), (fmt, double, nch, name, int((got[0] != want[0]).sum()))
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (fmt, double, nch, name)


def test_finish_windows_measure_only():
    x = finish_rows(3, F.RRX_FMT_S32, False)
    tab, dst_total = finish_table()
    gains = 0.5 + 0.4 * np.arange(len(SLICES))
    want = ragged_finish(x, tab, dst_total, None, gains, True)
    for part in (fin_even(7), fin_even(333)[::-1]):
        got = finish_windows(x, tab, dst_total, None, gains, True, part)
        assert got[0] is None and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert want[2].sum() > 0


def test_finish_windows_under_a_wrong_table_are_the_whole_row_call_under_it():
    x = finish_rows(2, F.RRX_FMT_S24_3, False)
    tab, dst_total = finish_table()
    last = len(SLICES) - 1
    for bad in ((0, 0, 0, 5, 2 ** 40, int(tab[last, 5])), (0, 0, 0, 5, 130, 2 ** 50), (0, 0, 0, 2 ** 63, 130, int(tab[last, 5])),
                (0, 0, 0, 2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1)):
        t2 = tab.copy()
        t2[last] = bad
        want = ragged_finish(x, t2, dst_total, F.RRX_FMT_S24_3, None, False)
        for part in (fin_even(7), FIN_PARTITIONS["16 singles"]):
            got = finish_windows(x, t2, dst_total, F.RRX_FMT_S24_3, None, False, part)
            for g, w in zip(got, want):
                assert np.array_equal(g, w), bad


# ---------------------------------------------------------------------------------------------------------------- end to end

def e2e_tracks(fs, lengths, int16):
    import torch
    xs = [music_like(n, 2, fs, 70 + i) for i, n in enumerate(lengths)]
    if int16:
        xs = [np.rint(x.astype(np.float64) * 0.5 * 2.0 ** 15).astype(np.int16) for x in xs]
    return [torch.from_numpy(x).cuda() for x in xs]


def both_forms(fs, fo, lengths, nstreams, int16, window, fmt, **kw):
    tracks = e2e_tracks(fs, lengths, int16)
    out = []
    for streamed in (False, True):
        r = F.Resampler(fs, fo, nch=2, nstreams=nstreams)    # a fresh handle each
        if streamed:
            out.append(r.convert_tracks_to_pcm_streamed(tracks, fmt, window=window, **dict(kw)))
        else:
            out.append(r.convert_tracks_to_pcm_device(tracks, fmt, **dict(kw)))
        assert r.available == 0
        r.close()
    return out


@pytest.mark.parametrize("fs,fo,lengths,nstreams,int16,window,fmt,kw", [
    (44100, 48000, (40, 65, 1500, 7000, 30000), 5, False, 4099, F.RRX_FMT_S16, {}),                                  # A: several pushes, windows through extensions
    (96000, 44100, (70, 3000, 50000), 4, True, 10007, F.RRX_FMT_S24_3, dict(gain=1.9, dither=True, seed=SEED)),       # B
    (44100, 48000, (40, 65, 1500, 7000, 30000), 5, False, None, F.RRX_FMT_S24_3, dict(dither=True, seed=SEED)),       # C: window = isamp_max
], ids=["A", "B", "C"])
def test_streamed_conversion_equals_the_whole_row_form(fs, fo, lengths, nstreams, int16, window, fmt, kw):
    import torch
    plan = F.tracks_plan(fs, fo, lengths)
    if window is not None:
        assert plan.row_frames > 3 * window                  # several pushes
        assert any(int(e.lead) % window and (int(e.lead) + int(e.frames)) % window for e in plan.table)
    (views, peak, clipped), (sviews, speak, sclipped) = both_forms(fs, fo, lengths, nstreams, int16, window, fmt, **kw)
    assert len(views) == len(sviews) == len(lengths)
    for t, (v, s) in enumerate(zip(views, sviews)):
        assert v.shape == s.shape and v.dtype == s.dtype and v.shape[0] == int(plan.table[t].out_frames)
        assert torch.equal(v, s), (t, int((v != s).sum()))
    assert sviews[0]._base is sviews[-1]._base                # one packed buffer
    assert torch.equal(peak.view(torch.int64), speak.view(torch.int64)) and torch.equal(clipped, sclipped)
    assert float(peak.max()) > 0.1


def test_streamed_refusals():
    import torch
    r = F.Resampler(FS, FO, nch=2, nstreams=2)
    x = [torch.zeros((100, 2), device="cuda")]
    with pytest.raises(ValueError):
        r.convert_tracks_to_pcm_streamed(x, F.RRX_FMT_S16, window=r.isamp_max + 1)
    with pytest.raises(ValueError):
        r.convert_tracks_to_pcm_streamed(x, F.RRX_FMT_S16, window=0)
    with pytest.raises(ValueError):
        r.convert_tracks_to_pcm_streamed(x, F.RRX_FMT_S16, peak=torch.zeros((2, 2), dtype=torch.float64, device="cuda"))
    views, peak, clipped = r.convert_tracks_to_pcm_streamed([torch.zeros((0, 2), device="cuda")], F.RRX_FMT_S16)   # nothing but an empty track
    assert tuple(views[0].shape) == (0, 2) and not peak.any() and not clipped.any()
    r.close()


def test_streamed_memory_is_bounded_by_the_windows():
    """The rise of torch's peak allocation over the call: at most the packed source, the destination, the two windows, the table
    and the statistics, plus 1 MiB (the allocator rounds each of about ten blocks up to 512 bytes) -- and the whole-row form on
    the same input is above that bound, so the bound says something."""
    import torch
    fs, fo, lengths, nstreams, window = 44100, 48000, (40, 65, 1500, 7000, 30000), 5, 4099
    tracks = e2e_tracks(fs, lengths, False)
    plan = F.tracks_plan(fs, fo, lengths)
    win_out = -(-window * fo // fs)                           # the output window convert_tracks_to_pcm_streamed documents
    bound = (plan.src_total * 2 * 4 + plan.dst_total * 2 * 2 + nstreams * window * 2 * 4 + nstreams * win_out * 2 * 4 +
             nstreams * 48 + 2 * nstreams * 2 * 8 + (1 << 20))
    rise = []
    for streamed in (True, False):
        r = F.Resampler(fs, fo, nch=2, nstreams=nstreams)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        if streamed:
            res = r.convert_tracks_to_pcm_streamed(tracks, F.RRX_FMT_S16, window=window)
        else:
            res = r.convert_tracks_to_pcm_device(tracks, F.RRX_FMT_S16)
        torch.cuda.synchronize()
        rise.append(torch.cuda.max_memory_allocated() - before)
        del res
        r.close()
    print("bound", bound, "streamed", rise[0], "whole rows", rise[1])
    assert rise[0] <= bound, (rise, bound)
    assert rise[1] > bound, (rise, bound)
