"""Gapless albums, host side (include/ratelib_amd_album.h; DESIGN.md 11, "Gapless albums"): the symbols, the planner against the
model's formulas, the stage pass's host twin against the model's rows, every refusal that needs no device, and the point of it
all on the CPU oracle -- an album's rows, staged by the twin, resampled one by one on fresh handles and cut by their entries, are
the album resampled as one stream.  CPU only."""
import ctypes as C
import inspect
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import album_cases as AC
import album_model as AM
import foo_dsp_resampler_amd as F
import parity
from oracle_binding import Oracle

ROOT = AC.ROOT
RR_OK, RR_INVPARAM, RR_EXTUNINIT = 0, 6, 5
NONE = F.RRX_LINK_NONE


def cfg(fs, fo):
    return F.RRConfig(fs, fo, 50.0, 95.0, 0, F.RR_BEST)


def test_symbols_are_exported_and_listed():
    declared, streamed = AC.header_functions()
    assert declared == sorted(F.ALBUM_SYMBOLS) and F.album.available_symbols() == F.ALBUM_SYMBOLS
    assert "typedef struct RRX_track_link" in AC.header_text() and C.sizeof(F.RRXTrackLink) == 16
    for name in ("tracks_plan_album", "tracks_stage_album_device", "tracks_stage_album_window_device", "TracksAlbumPlan", "RRX_LINK_NONE"):
        assert hasattr(F, name) and name in F.__all__
    for m in ("convert_tracks_device", "convert_tracks_to_pcm_device", "convert_library_to_pcm"):
        p = inspect.signature(getattr(F.Resampler, m)).parameters
        assert "gapless" in p and p["gapless"].default is None, m
    # (convert_tracks_to_pcm_streamed takes it as a keyword beside those of the output stage, as it takes `mix=`: its signature is pinned)
    assert "gapless" in inspect.getsource(F.Resampler.convert_tracks_to_pcm_streamed)
    makefile = open(os.path.join(ROOT, "foo_dsp_resampler_amd", "csrc", "Makefile")).read()
    assert "tracks_album.hip" in makefile and "FP_tracks_album  := -ffp-contract=off" in makefile


def test_every_stream_taking_entry_point_has_a_gated_case():
    """what tests/test_stream_order_table.py holds ratelib_amd.h to, for this header: every function whose parameter list names
    hip_stream, and every public wrapper that takes `stream=`, is run behind gates by tests/test_gpu_tracks_album_stream.py"""
    _, streamed = AC.header_functions()
    assert streamed == sorted(AC.STREAM_WRAPPER_OF)
    takes = sorted(n for n, f in vars(F.album).items()
                   if inspect.isfunction(f) and not n.startswith("_") and "stream" in inspect.signature(f).parameters)
    assert takes == sorted(AC.STREAM_WRAPPER_OF.values())
    extra = AC.header_text() + "\nint RRX_new_album_device(int device, void *hip_stream,\n    int n);\n"
    assert "RRX_new_album_device" in AC.header_functions(extra)[1]


# --------------------------------------------------------------------------------------------------------------------- planner

def albums_of(lengths, groups):
    """[(first track, one past the last)] of every run of one non-negative id"""
    out, t0 = [], 0
    while t0 < len(lengths):
        t1 = t0 + 1
        while groups[t0] >= 0 and t1 < len(lengths) and groups[t1] == groups[t0]:
            t1 += 1
        if groups[t0] >= 0:
            out.append((t0, t1))
        t0 = t1
    return out


@pytest.mark.parametrize("fs,fo", AC.RATES)
def test_the_plan_is_the_model(fs, fo):
    for name, (lengths, groups) in AC.PLANS.items():
        plan = F.tracks_plan_album(fs, fo, lengths, groups)
        table, links, row, cap, src, dst = AM.plan_model(fs, fo, lengths, groups)
        assert [tuple(int(v) for v in e) for e in plan.array()] == table, name
        assert [tuple(int(v) for v in e) for e in plan.links_array()] == links, name
        assert (plan.row_frames, plan.out_row_cap, plan.src_total, plan.dst_total) == (row, cap, src, dst), name
        g = np.gcd(fs, fo)
        r1 = fs // g
        for t0, t1 in albums_of(lengths, groups):
            A = sum(lengths[t0:t1])
            if A <= 64:
                continue
            # the tiling identity: the album's slices add up to the album as one track, and every row starts on the album's grid
            assert sum(int(e.out_frames) for e in plan.table[t0:t1]) == F.track_geometry(fs, fo, A)[3], (name, t0)
            S = 0
            for e in plan.table[t0:t1]:
                assert (S - int(e.lead)) % r1 == 0, (name, t0)
                S += int(e.frames)
    n_add = F.edge_geometry(fs, fo)[0]
    assert AC.PLANS["first-shorter-than-n_add"][0][0] < n_add


def test_singles_are_tracks_plan_entry_for_entry():
    for fs, fo in AC.RATES[:3]:
        lengths = [100, 0, 1500, 64, 65, 30000, 1500, 40]
        plain = F.tracks_plan(fs, fo, lengths)
        for groups in ([-1] * 8, [-1, -2, -1, -1, -7, -1, -1, -1]):
            plan = F.tracks_plan_album(fs, fo, lengths, groups)
            assert (plan.array() == plain.array()).all() and (plan.links_array() == NONE).all()
            assert (plan.row_frames, plan.out_row_cap, plan.src_total, plan.dst_total) == (plain.row_frames, plain.out_row_cap, plain.src_total,
                                                                                          plain.dst_total)
        # an album of at most 64 frames in all is planned as singles, and an album of one track is that track
        lengths, groups = AC.PLANS["tiny-album"]
        assert (F.tracks_plan_album(fs, fo, lengths, groups).array() == F.tracks_plan(fs, fo, lengths).array()).all()
        lengths, groups = AC.PLANS["album-of-one"]
        plan = F.tracks_plan_album(fs, fo, lengths, groups)
        assert (plan.array() == F.tracks_plan(fs, fo, lengths).array()).all() and (plan.links_array() == NONE).all()


def test_plan_refusals():
    good = cfg(44100, 48000)
    assert AM.plan_raw(good, [100, 200], [0, 0])[0] == RR_OK
    for k in ("config", "frames", "group", "table", "links", "row", "cap", "src", "dst"):
        code, _, _, v = AM.plan_raw(good, [100, 200], [0, 0], null=(k,))
        assert code == RR_INVPARAM and all(x == 0xdead for x in v), k   # a refused call writes none of the four
    assert AM.plan_raw(good, [100], [0], ntracks=0)[0] == RR_INVPARAM
    assert AM.plan_raw(good, [100], [0], ntracks=-1)[0] == RR_INVPARAM
    assert AM.plan_raw(cfg(1, 100000), [100], [0])[0] == RR_INVPARAM
    assert AM.plan_raw(cfg(0, 48000), [100], [0])[0] == RR_INVPARAM
    assert AM.plan_raw(good, [2 ** 64 - 1], [0])[0] == RR_INVPARAM
    assert AM.plan_raw(good, [2 ** 63, 2 ** 63], [0, 0])[0] == RR_INVPARAM
    assert AM.plan_raw(good, [100, 2 ** 36 + 1], [-1, -1])[0] == RR_INVPARAM
    assert AM.plan_raw(good, [2 ** 35 + 1, 2 ** 35 + 1], [0, 0])[0] == RR_INVPARAM   # the album is walked as one track
    # an id that comes back behind another one
    code, _, _, v = AM.plan_raw(good, [100, 200, 300], [0, 1, 0])
    assert code == RR_INVPARAM and all(x == 0xdead for x in v)
    assert AM.plan_raw(good, [100, 200, 300, 50], [0, -1, 0, 5])[0] == RR_INVPARAM
    assert AM.plan_raw(good, [100, 200, 300, 50], [-1, 0, -1, -1])[0] == RR_OK      # singles may repeat their negative ids
    with pytest.raises(ValueError):
        F.tracks_plan_album(44100, 48000, [], [])
    with pytest.raises(ValueError):
        F.tracks_plan_album(44100, 48000, [10, -1], [0, 0])
    with pytest.raises(ValueError):
        F.tracks_plan_album(44100, 48000, [10, 20], [0])
    with pytest.raises(F.RRError):
        F.tracks_plan_album(44100, 48000, [10, 20, 30], [0, 1, 0])


# ------------------------------------------------------------------------------------------------------------ twin against model

STAGE_LENGTHS, STAGE_GROUPS = [700, 3000, 100, 2500, 70, 40, 2300], [1, 1, 1, 1, -1, -1, 2]


def check_rows(got, rows, written, label):
    assert got.shape == rows.shape, label
    w = np.broadcast_to(written[..., None], rows.shape)
    assert (got.view(np.uint32)[w] == rows.view(np.uint32)[w]).all(), label
    assert (got[~w] == AM.UNTOUCHED).all(), (label, "the frames of an edge without a link were written")


@pytest.mark.parametrize("fmt", AC.FORMATS)
def test_the_twin_is_the_model_bit_for_bit(fmt):
    fs, fo = 44100, 48000
    plan = F.tracks_plan_album(fs, fo, STAGE_LENGTHS, STAGE_GROUPS)
    table, links, R, S = plan.array(), plan.links_array(), plan.row_frames, plan.src_total
    assert int(table[0][2]) > STAGE_LENGTHS[0]                       # the album begins inside track 1's backward extension
    for nch in (1, 2, 3):
        packed, x = AC.source(fmt, S, nch)
        rows, written = AM.stage_model(table, links, x, R)
        assert not written.all() and written[1].all() and written[2].all()   # album edges and singles extrapolate; inner rows do not
        check_rows(AM.twin(fs, fo, table, links, packed, fmt, nch, S, R), rows, written, (fmt, nch))
        for wf, wn in ((0, 1), (2204, 63), (2205 + 690, 40), (R - 500, 500), (R - 1, 1), (1000, 0)):
            got = AM.twin(fs, fo, table, links, packed, fmt, nch, S, R, win=(wf, wn), stride=wn + 3)
            check_rows(got[:, :wn], rows[:, wf:wf + wn], written[:, wf:wf + wn], (fmt, nch, wf, wn))
            assert (got[:, wn:] == AM.UNTOUCHED).all()
        # without links every edge is extrapolated: the track and the zeros behind it, as RRX_tracks_stage_device_samples copies them
        none = np.full_like(links, NONE)
        rows0, written0 = AM.stage_model(table, none, x, R)
        check_rows(AM.twin(fs, fo, table, None, packed, fmt, nch, S, R), rows0, written0, (fmt, nch, "no links"))
        plain = F.tracks_plan(fs, fo, STAGE_LENGTHS)
        rows1, written1 = AM.stage_model(plain.array(), none, x, plain.row_frames)
        check_rows(AM.twin(fs, fo, plain.array(), None, packed, fmt, nch, S, plain.row_frames), rows1, written1, (fmt, nch, "plain plan"))


def test_any_subset_of_the_entries_is_a_batch_table():
    fs, fo, fmt, nch = 44100, 48000, F.RRX_FMT_S24_3, 2
    plan = F.tracks_plan_album(fs, fo, STAGE_LENGTHS, STAGE_GROUPS)
    packed, x = AC.source(fmt, plan.src_total, nch)
    rows, written = AM.stage_model(plan.array(), plan.links_array(), x, plan.row_frames)
    r = random.Random(5)
    for _ in range(12):
        idx = r.sample(range(len(plan)), r.randrange(1, len(plan) + 1))
        sub = plan.subset(idx, pad=r.randrange(3))
        assert sub.row_frames == max(int(plan.table[i].frames + 2 * plan.table[i].lead) for i in idx)
        assert (sub.src_total, sub.dst_total, sub.out_row_cap) == (plan.src_total, plan.dst_total, sub.row_frames * fo // fs + 2)
        got = AM.twin(fs, fo, sub.array(), sub.links_array(), packed, fmt, nch, plan.src_total, sub.row_frames)
        R = sub.row_frames
        check_rows(got[:len(idx)], rows[idx][:, :R], written[idx][:, :R], idx)
        assert (rows[idx][:, R:] == 0).all()                         # (what the shorter rows leave out is the longer ones' zeros)
        assert (got[len(idx):] == 0).all()                           # the idle streams: zero-length entries, rows of zeros


def test_hostile_tables_and_links_read_inside_the_source():
    fs, fo, nch = 44100, 48000, 2
    S, R = 900, 5000
    big = 2 ** 64 - 1
    entries = [(300, 200, 2205, 0, 0, 0), (2 ** 40, 200, 2205, 0, 0, 0), (850, 200, 2205, 0, 0, 0), (300, 2 ** 40, 2205, 0, 0, 0),
               (300, 200, 2 ** 62, 0, 0, 0), (big, big, big, 0, 0, 0), (0, 900, 100, 0, 0, 0), (900, 0, 300, 0, 0, 0), (100, 0, 2205, 0, 0, 0)]
    link_sets = [(0, 0), (5, 7), (2 ** 40, 2 ** 40), (big - 1, big - 1), (NONE, 2 ** 50), (2 ** 50, NONE), (299, 401), (300, 400), (301, 399)]
    for fmt in AC.FORMATS:
        packed, x = AC.source(fmt, S, nch, 9)
        for ln in link_sets:
            links = [ln] * len(entries)
            rows, written = AM.stage_model(entries, links, x, R)
            check_rows(AM.twin(fs, fo, entries, links, packed, fmt, nch, S, R), rows, written, (fmt, ln))
    # the twin ran on an array of exactly S frames: a read outside it is what the sanitised build of the suite looks for; here the
    # values say the same, since every frame the model takes from the source lies in [0, S)
    r = random.Random(11)
    for _ in range(300):
        e = tuple(r.choice([0, 1, r.randrange(2 ** 12), r.randrange(2 ** 40), 2 ** 63, big - r.randrange(3)]) for _ in range(3)) + (0, 0, 0)
        ln = tuple(r.choice([0, 1, r.randrange(2 ** 12), 2 ** 63, big - 1, NONE]) for _ in range(2))
        R2 = r.choice([1, 2, r.randrange(1, 6000)])
        packed, x = AC.source(F.RRX_FMT_S16, S, 1, 3)
        rows, written = AM.stage_model([e], [ln], x, R2)
        check_rows(AM.twin(fs, fo, [e], [ln], packed, F.RRX_FMT_S16, 1, S, R2), rows, written, (e, ln, R2))


# ------------------------------------------------------------------------------------------------------------------ refusals

CHILD = r"""
import sys, ctypes as C
sys.path.insert(0, %r)
import foo_dsp_resampler_amd as F
L = F.album.lib()
p = 0x10000  # never dereferenced: every call below is answered from its arguments, or from the library's state, alone
base = dict(device=-1, stream=None, fs=44100, fo=48000, table=p, links=p, ntracks=3, nch=2, fmt=16, packed=p, src_total=1000, row_frames=4096,
            first=100, frames=500, win=p, stride=512)
def rows(**kw):
    a = dict(base, **kw)
    return L.RRX_tracks_stage_album_device(a["device"], a["stream"], a["fs"], a["fo"], a["table"], a["links"], a["ntracks"], a["nch"], a["fmt"],
                                           a["packed"], a["src_total"], a["win"], a["row_frames"])
def window(**kw):
    a = dict(base, **kw)
    return L.RRX_tracks_stage_album_window_device(a["device"], a["stream"], a["fs"], a["fo"], a["table"], a["links"], a["ntracks"], a["nch"],
                                                  a["fmt"], a["packed"], a["src_total"], a["row_frames"], a["first"], a["frames"], a["win"],
                                                  a["stride"])
def twin(**kw):
    a = dict(base, **kw)
    return L.RRX_debug_tracks_stage_album_host(a["fs"], a["fo"], a["table"], a["links"], a["ntracks"], a["nch"], a["fmt"], a["packed"],
                                               a["src_total"], a["row_frames"], a["first"], a["frames"], a["win"], a["stride"])
shared = [("fmt8", dict(fmt=8)), ("double", dict(fmt=1)), ("table", dict(table=None)), ("packed", dict(packed=None)), ("win", dict(win=None)),
          ("ntracks0", dict(ntracks=0)), ("ntracks-1", dict(ntracks=-1)), ("nch0", dict(nch=0)), ("fs0", dict(fs=0)), ("fo0", dict(fo=0)),
          ("channels2^30", dict(ntracks=2**29, nch=2)), ("src2^60", dict(src_total=2**59)), ("rows2^60", dict(row_frames=2**58))]
win_only = [("past-the-row", dict(first=3597)), ("sum-wraps", dict(first=2**64 - 1, frames=2)), ("stride", dict(stride=499)),
            ("stride0", dict(stride=0)), ("window2^60", dict(stride=2**58)), ("row_frames0", dict(row_frames=0, first=0, frames=0))]
for links in (p, None):                      # with links, and without them (the un-linked calls' own refusals)
    for name, kw in shared + [("device-2", dict(device=-2)), ("row_frames0", dict(row_frames=0))]:
        print("inv rows", name, rows(links=links, **kw))
    for name, kw in shared + win_only + [("device-2", dict(device=-2))]:
        print("inv window", name, window(links=links, **kw))
    for name, kw in [("good", dict()), ("float", dict(fmt=0)), ("s24", dict(fmt=24)), ("s32", dict(fmt=32))]:
        print("ok rows", name, rows(links=links, **kw))
    for name, kw in [("good", dict()), ("s24", dict(fmt=24)), ("whole-row", dict(first=0, frames=4096, stride=4096)), ("last-frame", dict(first=4095, frames=1)),
                     ("win_frames0", dict(frames=0))]:
        print("ok window", name, window(links=links, **kw))
for name, kw in shared + win_only:
    print("inv twin", name, twin(**kw))
"""


def test_device_calls_refuse_from_their_arguments_alone():
    """RR_INVPARAM comes before RR_EXTUNINIT: in a process that never called init_ratelib (and sees no device) every refusal is
    answered from the arguments, and a call with nothing to refuse gets as far as RR_EXTUNINIT and no further"""
    out = subprocess.run([sys.executable, "-c", CHILD % ROOT], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", RSMP_TEST_HOOKS="1"))
    assert out.returncode == 0, out.stderr
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.split() and ln.split()[0] in ("inv", "ok")]
    for what, n_inv, n_ok in (("rows", 2 * 15, 2 * 4), ("window", 2 * 20, 2 * 5), ("twin", 19, 0)):
        inv = [ln for ln in lines if ln[:2] == ["inv", what]]
        assert len(inv) == n_inv and all(int(ln[3]) == RR_INVPARAM for ln in inv), inv
        ok = [ln for ln in lines if ln[:2] == ["ok", what]]
        assert len(ok) == n_ok and all(int(ln[3]) == RR_EXTUNINIT for ln in ok), ok


def test_the_twin_is_inert_without_test_hooks():
    code = ("import sys; sys.path.insert(0, %r)\nimport foo_dsp_resampler_amd as F\n"
            "print(F.album.lib().RRX_debug_tracks_stage_album_host(0, 0, None, None, 0, 0, 0, None, 0, 0, 0, 0, None, 0))\n" % ROOT)
    env = {k: v for k, v in os.environ.items() if k != "RSMP_TEST_HOOKS"}
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-1] == "-1"


def test_python_refusals_need_no_device():
    class Fake:                                              # enough of a tensor to reach the checks that come first
        def __init__(self, dtype, shape):
            self.dtype, self.shape, self.is_cuda = dtype, shape, False

        def dim(self):
            return len(self.shape)

        def is_contiguous(self):
            return True

    with pytest.raises(TypeError):
        F.tracks_stage_album_device(Fake("torch.float32", (10, 2)), None, None, 44100, 48000, 100)
    with pytest.raises(TypeError):
        F.tracks_stage_album_window_device(Fake("torch.float32", (10, 2)), None, None, 44100, 48000, 100, 0, 10)
    with pytest.raises(ValueError):
        F.album._gapless_checked([0, 0], 3)


# -------------------------------------------------------------------------------------------------------- continuity on the oracle

def one_stream(fs, fo, row):
    return Oracle(fs, fo, nch=1).process(row)


@pytest.mark.parametrize("fs,fo", [(44100, 48000), (48000, 44100)])
@pytest.mark.parametrize("lengths", [[20011, 9000, 15013], [7001, 64, 12000, 1, 9999]], ids=["three", "five"])
def test_an_album_s_rows_are_the_album_as_one_stream(fs, fo, lengths):
    """Every row staged by the twin -- the neighbours' frames inside, zeros for the album's outer extension on both sides -- then
    resampled by a fresh oracle handle and cut by its entry, against the album between zeros resampled as one stream and cut as one
    track.  The frame counts are equal.  The bar is 0.01 "ulp" of tests/parity.py: ten times the 0.001 measured on tones when the
    geometry was derived (fp64 rounding across differently aligned FFT blocks; noise was bit-equal), a hundredth of the 1.0 bar of
    the GPU tests that this property feeds.  Default passband only: a steeper one has filters longer than n_add, which truncates
    the context in the per-track path as well, and nobody has measured that."""
    n_add, n_drop, _, _ = F.edge_geometry(fs, fo)
    A = sum(lengths)
    plan = F.tracks_plan_album(fs, fo, lengths, [0] * len(lengths))
    whole = F.tracks_plan(fs, fo, [A])
    assert plan.dst_total == whole.dst_total
    for name, x in AC.signals(A, fs).items():
        ref_row = np.zeros((A + 2 * n_add, 1), np.float32)
        ref_row[n_add:n_add + A] = x
        ref = one_stream(fs, fo, ref_row)[n_drop:n_drop + whole.dst_total]
        assert ref.shape[0] == whole.dst_total
        rows = AM.twin(fs, fo, plan.array(), plan.links_array(), x, F.RRX_FMT_FLOAT, 1, A, plan.row_frames)
        rows[rows == AM.UNTOUCHED] = 0.0                       # the album's outer edges: zeros, as the reference has them
        parts = []
        for t, e in enumerate(plan.table):
            y = one_stream(fs, fo, rows[t, :int(e.frames + 2 * e.lead)])
            assert y.shape[0] >= int(e.out_first + e.out_frames), (name, t)
            parts.append(y[int(e.out_first):int(e.out_first + e.out_frames)])
        got = np.concatenate(parts)
        assert got.shape == ref.shape
        rep = parity.compare_f32(got, ref)
        print("album continuity", fs, fo, name, len(lengths), rep)
        assert rep["max_ulp"] <= 0.01, (name, rep)
