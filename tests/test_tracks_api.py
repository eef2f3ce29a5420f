"""Ragged track batches, host side (RRX_track_geometry / RRX_tracks_plan): the geometry of a track on a handle of
its own against the plugin harness over the CPU resampler, the table of a batch against that geometry, and every refusal that
needs no device.  CPU only."""
import ctypes as C
import functools
import os

import pytest

import foo_dsp_resampler_amd as F
from oracle_binding import OracleDsp
from test_plugin_layer import music_like, run_track

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RR_OK, RR_INVPARAM = 0, 6
RATES = [(44100, 48000), (96000, 44100), (44100, 48001)]
# both sides of the 64-frame branch, of prime_len (2205 at 44.1 kHz) and of one second of input (the counters' wrap)
LENGTHS = [1, 40, 64, 65, 100, 1500, 2205, 2206, 30000, 100000]
NEW = ("RRX_track_geometry", "RRX_tracks_plan", "RRX_tracks_stage_device", "RRX_tracks_finish_device")


def cfg(fs, fo):
    return F.RRConfig(fs, fo, 50.0, 95.0, 0, F.RR_BEST)


def test_symbols_are_exported_and_listed():
    header = open(os.path.join(ROOT, "include", "ratelib_amd.h")).read()
    for name in NEW:
        assert name in F.EXPECTED_SYMBOLS and name in F.available_symbols()
        assert name in header
    assert "typedef struct RRX_track" in header and C.sizeof(F.RRXTrack) == 48
    for name in ("track_geometry", "tracks_plan", "tracks_stage_device", "tracks_finish_device"):
        assert callable(getattr(F, name))
    assert hasattr(F.Resampler, "convert_tracks_device") and hasattr(F.Resampler, "convert_tracks_to_pcm_device")


@functools.lru_cache(maxsize=None)
def harness_total(fs, fo, frames):
    """frames the plugin harness emits for one track over the CPU resampler"""
    outs, _ = run_track(OracleDsp(fo), music_like(frames, 2, fs, 7), fs, [4096])
    return sum(c.shape[0] for c, _ in outs)


@pytest.mark.parametrize("fs,fo", RATES)
def test_track_geometry_is_the_plugin_harness_track(fs, fo):
    n_add, n_drop, _, _ = F.edge_geometry(fs, fo)
    for frames in LENGTHS:
        lead, ext, out_first, out_frames = F.track_geometry(fs, fo, frames)
        want = (n_add, frames + 2 * n_add, n_drop) if frames > 64 else (0, frames, 0)
        total = harness_total(fs, fo, frames)
        print(fs, fo, frames, (lead, ext, out_first, out_frames), "harness", total)
        assert (lead, ext, out_first) == want
        assert out_frames == total
    assert F.track_geometry(fs, fo, 0) == (0, 0, 0, 0)          # legal, and owns no output


def test_the_longest_length_is_past_the_counter_wrap():
    # (what makes 100000 frames a case of its own: more than one second of input AND of output before the drain)
    for fs, fo in RATES:
        _, ext, _, out_frames = F.track_geometry(fs, fo, LENGTHS[-1])
        assert ext > fs and out_frames > fo


def plan_raw(c, lengths, ntracks=None, null=()):
    n = len(lengths)
    fr = (C.c_size_t * max(n, 1))(*lengths)
    table = (F.RRXTrack * max(n, 1))()
    v = [C.c_size_t(0xdead) for _ in range(4)]
    args = dict(config=C.byref(c) if c is not None else None, frames=fr, table=table, row=C.byref(v[0]), cap=C.byref(v[1]), src=C.byref(v[2]),
                dst=C.byref(v[3]))
    for k in null:
        args[k] = None
    rc = F.lib().RRX_tracks_plan(args["config"], args["frames"], n if ntracks is None else ntracks, args["table"], args["row"], args["cap"],
                                 args["src"], args["dst"])
    return rc, table, [x.value for x in v]


def test_tracks_plan_is_geometry_per_entry_with_running_sums():
    fs, fo = 44100, 48000
    lengths = [100, 0, 1500, 64, 65, 0, 0, 30000, 1500, 40]
    plan = F.tracks_plan(fs, fo, lengths)
    assert len(plan) == len(lengths)
    src = dst = row = 0
    for e, frames in zip(plan.table, lengths):
        lead, ext, out_first, out_frames = F.track_geometry(fs, fo, frames)
        assert (e.src_first, e.frames, e.lead, e.out_first, e.out_frames, e.dst_first) == (src, frames, lead, out_first, out_frames, dst)
        src, dst, row = src + frames, dst + out_frames, max(row, ext)
    assert (plan.row_frames, plan.src_total, plan.dst_total) == (row, src, dst)
    assert plan.out_row_cap == row * fo // fs + 2               # convert_track_device's capacity for a row
    assert plan.array().shape == (len(lengths), 6) and plan.array()[7, 1] == 30000
    only_empty = F.tracks_plan(fs, fo, [0, 0])
    assert (only_empty.row_frames, only_empty.src_total, only_empty.dst_total, only_empty.out_row_cap) == (0, 0, 0, 2)
    assert all(e.out_frames == 0 and e.lead == 0 for e in only_empty.table)
    down = F.tracks_plan(96000, 44100, [70, 3000])
    assert down.out_row_cap == down.row_frames * 44100 // 96000 + 2


def test_refusals_need_no_device():
    good = cfg(44100, 48000)
    assert plan_raw(good, [100, 200])[0] == RR_OK
    for k in ("config", "frames", "table", "row", "cap", "src", "dst"):
        rc, _, v = plan_raw(good, [100, 200], null=(k,))
        assert rc == RR_INVPARAM, k
        assert all(x == 0xdead for x in v), k                   # a refused call writes nothing
    assert plan_raw(good, [100], ntracks=0)[0] == RR_INVPARAM
    assert plan_raw(good, [100], ntracks=-1)[0] == RR_INVPARAM
    assert plan_raw(cfg(1, 100000), [100])[0] == RR_INVPARAM    # a ratio the planner refuses (rate_base.h:528)
    assert plan_raw(cfg(0, 48000), [100])[0] == RR_INVPARAM
    big = 2 ** 64 - 1
    assert plan_raw(good, [big])[0] == RR_INVPARAM              # frames + 2 * n_add would wrap
    assert plan_raw(good, [2 ** 63, 2 ** 63])[0] == RR_INVPARAM  # the running sum would
    assert plan_raw(good, [100, 2 ** 36 + 1])[0] == RR_INVPARAM  # above what the call walks
    v = [C.c_size_t(0xdead) for _ in range(4)]
    p = [C.byref(x) for x in v]
    fn = F.lib().RRX_track_geometry
    assert fn(C.byref(good), 100, *p) == RR_OK and v[0].value == 2205
    assert fn(None, 100, *p) == RR_INVPARAM
    for i in range(4):
        q = list(p)
        q[i] = None
        assert fn(C.byref(good), 100, *q) == RR_INVPARAM, i
    assert fn(C.byref(cfg(1, 100000)), 100, *p) == RR_INVPARAM
    assert fn(C.byref(good), big, *p) == RR_INVPARAM
    with pytest.raises(ValueError):
        F.tracks_plan(44100, 48000, [])
    with pytest.raises(ValueError):
        F.tracks_plan(44100, 48000, [10, -1])


def test_device_calls_refuse_from_their_arguments_alone():
    """Everything below is answered before any device (or init_ratelib) is looked at; the pointers are never dereferenced."""
    L, p = F.lib(), 0x10000
    stage = dict(device=-1, stream=None, fs=44100, fo=48000, table=p, ntracks=3, nch=2, packed=p, src_total=1000, rows=p, row_frames=4096)

    def call_stage(**kw):
        a = dict(stage, **kw)
        return L.RRX_tracks_stage_device(a["device"], a["stream"], a["fs"], a["fo"], a["table"], a["ntracks"], a["nch"], a["packed"],
                                         a["src_total"], a["rows"], a["row_frames"])

    for kw in (dict(table=None), dict(packed=None), dict(rows=None), dict(ntracks=0), dict(ntracks=-1), dict(nch=0), dict(nch=-2),
               dict(fs=0), dict(fo=0), dict(row_frames=0), dict(device=-2), dict(ntracks=2 ** 29, nch=2), dict(src_total=2 ** 59),
               dict(row_frames=2 ** 58)):
        assert call_stage(**kw) == RR_INVPARAM, kw
    fin = dict(device=-1, stream=None, table=p, ntracks=3, nch=2, sf=0, rows=p, row_frames=4096, df=16, dst=p, dst_total=9000, gain=None,
               dither=1, seed=7, peak=p, clipped=p)

    def call_fin(**kw):
        a = dict(fin, **kw)
        return L.RRX_tracks_finish_device(a["device"], a["stream"], a["table"], a["ntracks"], a["nch"], a["sf"], a["rows"], a["row_frames"],
                                          a["df"], a["dst"], a["dst_total"], a["gain"], a["dither"], a["seed"], a["peak"], a["clipped"])

    for kw in (dict(table=None), dict(rows=None), dict(ntracks=0), dict(ntracks=-1), dict(nch=0), dict(sf=16), dict(sf=7), dict(df=0),
               dict(df=1), dict(df=8), dict(dst=None, peak=None, clipped=None), dict(device=-2), dict(row_frames=2 ** 58),
               dict(dst_total=2 ** 59)):
        assert call_fin(**kw) == RR_INVPARAM, kw
