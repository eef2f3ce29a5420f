"""The shaped output stage on the device (RRX_finish_shaped_device / RRX_tracks_finish_shaped_device, finish_shaped.hip) against the
numpy restatement of its arithmetic in shaped_model.py: output bytes, peak bit patterns, clip counts and the state, through
strides, guard bytes, unaligned rows and every shape of the lane grid; chunks with a ping-ponged state; the tracks form; and the
Python wrappers end to end.  The wrong tables of the tracks form are clamps at work, not faults provoked."""
import ctypes as C

import numpy as np
import pytest
import torch

import foo_dsp_resampler_amd as F
import shaped_model as SM

pytestmark = pytest.mark.gpu
SEED = 0x1234567887654321
MIX = 0xBF58476D1CE4E5B9
S16, S24, S32 = F.RRX_FMT_S16, F.RRX_FMT_S24_3, F.RRX_FMT_S32

# the CPU matrix thinned to one pass per axis: every value of an axis beside this base case
BASE = dict(target=(S16, True), double=False, gain=1.7, dith=True, order=9, segment=64, shape=(3, 3), frames=4099, first=3)
AXES = dict(target=[(S24, True), (S32, True), (S16, False)], double=[True], gain=[None, 0.5], dith=[False], order=[1, 5, 16],
            segment=[0, 1, 7, 5000], shape=[(1, 1), (1, 2), (2, 8)], frames=[1, 5], first=[0, 2 ** 32 + 5])


def check(case, **dev_kw):
    (fmt, write), (nstreams, nch) = case["target"], case["shape"]
    x = SM.make_input(nstreams, case["frames"], nch, fmt, case["double"])
    g = None if case["gain"] is None else case["gain"] * (1 + 0.25 * np.arange(nstreams))
    coefs = SM.coefs_of(case["order"])
    st = None if SM.restarts(case["first"], case["segment"]) else SM.random_state(nstreams, nch, case["order"])
    want = SM.model(x, fmt, coefs, case["segment"], g, case["dith"], SEED, case["first"], st, write=write)
    got = SM.device(x, fmt, coefs, case["segment"], g, case["dith"], SEED, case["first"], st, write=write, **dev_kw)
    SM.same(got, want, x, tuple(sorted(case.items(), key=str)))


@pytest.mark.parametrize("axis", ["base"] + sorted(AXES))
def test_kernel_equals_the_model_one_axis_at_a_time(axis):
    for value in [None] if axis == "base" else AXES[axis]:
        check(dict(BASE, **({} if axis == "base" else {axis: value})))


@pytest.mark.parametrize("fmt", SM.FORMATS, ids=["s16", "s24", "s32"])
def test_rows_at_strides_and_every_destination_phase(fmt):
    """rows one frame apart with guard bytes around them, the destination 1, 2 and 3 samples off an aligned address (and the
    source with it): every sample is stored with stores of its own width, so the phase cannot matter"""
    x = SM.make_input(2, 1201, 3, fmt, False)
    g = np.array([0.5, 1.7])
    want = SM.model(x, fmt, SM.W9, 64, g, True, SEED, 77, SM.random_state(2, 3, 9))
    for off in (0, 1, 2, 3):
        SM.same(SM.device(x, fmt, SM.W9, 64, g, True, SEED, 77, SM.random_state(2, 3, 9), pad=1, src_off=off, dst_off=off), want, x, (fmt, off))


@pytest.mark.parametrize("nch", [1, 2, 3, 8, 257])
def test_channel_counts(nch):
    """257 channels: a workgroup of 64 lanes lies inside one segment, and a segment's lanes span several workgroups"""
    x = SM.make_input(2, 300, nch, S24, False)
    for segment, first in ((64, 5), (0, 0)):
        st = None if SM.restarts(first, segment) else SM.random_state(2, nch, 5)
        SM.same(SM.device(x, S24, SM.L5, segment, None, True, SEED, first, st), SM.model(x, S24, SM.L5, segment, None, True, SEED, first, st), x,
                (nch, segment))


def test_a_segment_longer_than_the_call_and_a_segment_of_one():
    x = SM.make_input(2, 4099, 2, S16, True)
    for segment, first in ((10 ** 6, 0), (10 ** 6, 123456), (2 ** 63, 7), (1, 0), (1, 2 ** 40 + 1)):
        st = None if SM.restarts(first, segment) else SM.random_state(2, 2, 9)
        SM.same(SM.device(x, S16, SM.W9, segment, None, True, SEED, first, st), SM.model(x, S16, SM.W9, segment, None, True, SEED, first, st), x,
                (segment, first))


def test_many_workgroups_per_stream_and_a_last_partial_segment():
    """3 x 3 x 70 001 frames at segment 16: 4376 segments a stream, 13 128 lanes, 206 workgroups, the last segment of one frame --
    with a first frame that makes the first segment partial too"""
    x = SM.make_input(3, 70001, 3, S24, False)
    g = np.array([0.5, 1.0, 1.7])
    for first in (0, 2 ** 32 + 5):
        st = None if SM.restarts(first, 16) else SM.random_state(3, 3, 9)
        SM.same(SM.device(x, S24, SM.W9, 16, g, True, SEED, first, st, pad=1, src_off=1, dst_off=1), SM.model(x, S24, SM.W9, 16, g, True, SEED, first, st),
                x, (first,))


def test_never_restarting_is_one_lane_per_channel():
    x = SM.make_input(2, 4099, 2, S32, False)
    SM.same(SM.device(x, S32, SM.W9, 0, None, True, SEED), SM.model(x, S32, SM.W9, 0, None, True, SEED), x, ("segment 0",))


CUTS = (1, 63, 64, 65, 4000)


@pytest.mark.parametrize("segment", [64, 0])
def test_chunked_calls_with_a_ping_ponged_state_on_a_side_stream(segment):
    """through the Python call, which hands every call a new state tensor: the bytes, statistics and final state of one call"""
    x = SM.make_input(2, 4099, 3, S24, False)
    g = np.array([0.5, 1.7])
    want = SM.model(x, S24, SM.W9, segment, g, True, SEED)
    t = torch.from_numpy(x.copy()).cuda()
    gt = torch.from_numpy(g).cuda()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    out = torch.empty((2, 4099, 9), dtype=torch.uint8, device="cuda")
    peak = clipped = state = None
    with torch.cuda.stream(side):
        for lo, hi in zip((0,) + CUTS, CUTS + (4099,)):
            part = t[:, lo:hi].contiguous()
            o, peak, clipped, new = F.finish_shaped_device(part, S24, "wannamaker9", segment, gain=gt, seed=SEED, first_frame=lo, state=state, peak=peak,
                                                           clipped=clipped, stream=side)
            assert state is None or new.data_ptr() != state.data_ptr()
            out[:, lo:hi] = o
            state = new
    side.synchronize()
    got = (out.cpu().numpy(), peak.cpu().numpy().view(np.uint64), clipped.cpu().numpy().view(np.uint64), state.cpu().numpy())
    SM.same(got, want, x, ("chunks", segment))
    whole = F.finish_shaped_device(t, S24, "wannamaker9", segment, gain=gt, seed=SEED)
    torch.cuda.synchronize()
    assert torch.equal(whole[0], out) and torch.equal(whole[2], clipped) and torch.equal(whole[3], state)
    # measure only sees the clip count of the write, and a call without frames hands the state on
    m = F.finish_shaped_device(t, S24, "wannamaker9", segment, gain=gt, seed=SEED, out=False)
    assert m[0] is None and torch.equal(m[2], clipped)
    e = F.finish_shaped_device(t[:, :0].contiguous(), S24, "wannamaker9", segment, gain=gt, seed=SEED, first_frame=4099, state=state)
    assert torch.equal(e[3], state) and e[3].data_ptr() != state.data_ptr() and not e[2].any()
    assert np.array_equal(t.cpu().numpy().view(np.uint8), x.view(np.uint8)), "the source was written"


# ---------------------------------------------------------------------------------------------------------------- the tracks form

LENGTHS = [0, 1, 64, 65, 3000, 2047]          # output frames of the tracks
ROW = 3100                                    # pitch of the rows
GUARD = 0xA5


def tracks_case(nch, double):
    """rows of seeded noise with finish_model's planted values, every track's slice at an out_first of its own, packed end to end"""
    rows = np.array(SM.make_input(len(LENGTHS), ROW, nch, S24, double))
    tab = np.zeros((len(LENGTHS), 6), np.uint64)
    pos = 0
    for t, n in enumerate(LENGTHS):
        tab[t] = (0, 0, 0, min(7 * t, ROW - n), n, pos)
        pos += n
    return rows, tab, pos


def tracks_device(rows, tab, dst_total, fmt, coefs, segment, gain, dith, write=True, pre=64):
    """RRX_tracks_finish_shaped_device with guard bytes around the packed destination: (bytes or None, peak bits, clipped)"""
    n, row_frames, nch = rows.shape
    nb = SM.NBYTES[fmt]
    F.ratelib._ensure_init()
    src = torch.from_numpy(rows).cuda()
    table = torch.from_numpy(tab.view(np.int64)).cuda()
    nbytes = dst_total * nch * nb
    buf = torch.full((pre + nbytes + 64,), GUARD, dtype=torch.uint8, device="cuda") if write else None
    g = None if gain is None else torch.from_numpy(np.ascontiguousarray(gain, dtype=np.float64)).cuda()
    pk = torch.zeros((n, nch), dtype=torch.int64, device="cuda")
    cl = torch.zeros((n, nch), dtype=torch.int64, device="cuda")
    k = np.ascontiguousarray(coefs, dtype=np.float64)
    vp = C.c_void_p
    rc = F.lib().RRX_tracks_finish_shaped_device(-1, None, vp(table.data_ptr()), n, nch, F.RRX_FMT_DOUBLE if rows.dtype == np.float64 else F.RRX_FMT_FLOAT,
                                                 vp(src.data_ptr()), row_frames, fmt, vp(buf.data_ptr() + pre) if write else None, dst_total,
                                                 vp(g.data_ptr()) if g is not None else None, int(dith), SEED, vp(k.ctypes.data), len(k), segment,
                                                 vp(pk.data_ptr()), vp(cl.data_ptr()))
    assert rc == 0, rc
    raw = None
    if write:
        host = buf.cpu().numpy()
        assert (host[:pre] == GUARD).all() and (host[pre + nbytes:] == GUARD).all(), "bytes around the destination were written"
        raw = host[pre:pre + nbytes]
    assert np.array_equal(src.cpu().numpy().view(np.uint8), rows.view(np.uint8)), "the rows were written"
    return raw, pk.cpu().numpy().view(np.uint64), cl.cpu().numpy().view(np.uint64)


def per_track(rows, slices, fmt, coefs, segment, gain, dith, device_too):
    """track by track: the model on the slice with the seed moved to the track's stream -- and, where asked, the one-stream device
    call, which must agree; slices: (track, first frame of the row, frames).  ({track: bytes}, peak bits, clipped)"""
    n, _, nch = rows.shape
    parts, pk, cl = {}, np.zeros((n, nch), np.uint64), np.zeros((n, nch), np.uint64)
    for t, of, cnt in slices:
        if not cnt:
            continue
        sl = np.array(rows[t, of:of + cnt])[None]
        seed = (SEED + t * nch * MIX) % 2 ** 64
        g = None if gain is None else gain[t:t + 1]
        want = SM.model(sl, fmt, coefs, segment, g, dith, seed, 0)
        if device_too:
            SM.same(SM.device(sl, fmt, coefs, segment, g, dith, seed, 0), want, sl, ("one-stream call", t))
        parts[t], pk[t], cl[t] = want[0].reshape(-1), want[1][0], want[2][0]
    return parts, pk, cl


def same_tracks(got, want, rows, slices, starts, nb, what):
    raw, pk, cl = got
    parts, wpk, wcl = want
    nch = rows.shape[2]
    for t, of, cnt in slices:
        if cnt:
            lo = starts[t] * nch * nb
            assert np.array_equal(raw[lo:lo + cnt * nch * nb], parts[t]), ("bytes of track", t) + what
    nan = np.zeros(pk.shape, bool)
    for t, of, cnt in slices:
        nan[t] = np.isnan(rows[t, of:of + cnt]).any(axis=0)
    assert np.array_equal(pk[~nan], wpk[~nan]) and np.isnan(pk.view(np.float64)[nan]).all(), ("peaks",) + what
    assert np.array_equal(cl, wcl), ("clip counts",) + what


@pytest.mark.parametrize("fmt,double,nch,segment", [(S16, False, 2, 64), (S24, False, 3, 1000), (S32, True, 1, 0), (S24, True, 2, 1)],
                         ids=["s16-f32-2ch-64", "s24-f32-3ch-1000", "s32-f64-1ch-0", "s24-f64-2ch-1"])
def test_tracks_form_is_the_per_track_one_stream_call(fmt, double, nch, segment):
    rows, tab, total = tracks_case(nch, double)
    gains = 0.5 + 0.4 * np.arange(len(LENGTHS))
    slices = [(t, int(tab[t, 3]), int(tab[t, 4])) for t in range(len(LENGTHS))]
    starts = [int(tab[t, 5]) for t in range(len(LENGTHS))]
    want = per_track(rows, slices, fmt, SM.W9, segment, gains, True, device_too=True)
    got = tracks_device(rows, tab, total, fmt, SM.W9, segment, gains, True, pre=65 if fmt == S24 else 66 if fmt == S16 else 64)
    same_tracks(got, want, rows, slices, starts, SM.NBYTES[fmt], (fmt, double, nch, segment))
    assert want[2].sum() > 0 and not got[1][0].any() and not got[2][0].any()         # clipped samples to count; the empty track
    measured = tracks_device(rows, tab, total, fmt, SM.W9, segment, gains, True, write=False)
    assert measured[0] is None and np.array_equal(measured[2], got[2])


def test_a_wrong_table_gives_the_clamped_model_and_stays_inside_the_buffers():
    """entries no plan makes, clamped as RRX_tracks_finish_device clamps them (tracks_slice): the slice is cut to the row and to the
    destination; guard bytes are checked inside tracks_device, and the other tracks are not disturbed"""
    rows, tab, total = tracks_case(2, False)
    last = len(LENGTHS) - 1
    dfl = int(tab[last, 5])
    good = tracks_device(rows, tab, total, S24, SM.W9, 64, None, True)
    for bad in ((0, 0, 0, 5, 2 ** 40, dfl),                    # out_frames beyond row and destination: cut to what the destination has left
                (0, 0, 0, ROW - 100, 2 ** 40, dfl),            # cut to the row: 100 frames
                (0, 0, 0, 5, 130, 2 ** 50),                    # a destination position past dst_total: nothing written
                (0, 0, 0, 2 ** 63, 130, dfl),                  # an output position past the row: nothing read or written
                (0, 0, 0, 2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1)):
        t2 = tab.copy()
        t2[last] = bad
        of = min(bad[3], ROW)
        df = min(bad[5], total)
        cnt = min(bad[4], ROW - of, total - df)
        slices = [(t, int(tab[t, 3]), int(tab[t, 4])) for t in range(last)] + [(last, of, cnt)]
        starts = [int(tab[t, 5]) for t in range(last)] + [df]
        want = per_track(rows, slices, S24, SM.W9, 64, None, True, device_too=False)
        got = tracks_device(rows, t2, total, S24, SM.W9, 64, None, True)
        same_tracks(got, want, rows, slices, starts, 3, (bad,))
        own = dfl * 2 * 3
        assert np.array_equal(got[0][:own], good[0][:own]), bad
        assert (got[0][own:df * 6] == GUARD).all() and (got[0][(df + cnt) * 6:] == GUARD).all(), bad   # nothing around the clamped slice


# ------------------------------------------------------------------------------------------------------------ Python, end to end

def music(lengths):
    from test_plugin_layer import music_like
    return [music_like(n, 2, 44100, 60 + i) for i, n in enumerate(lengths)]


def test_convert_tracks_to_pcm_device_with_shaping_is_the_model_on_the_rows():
    tracks = [torch.from_numpy(x).cuda() for x in music((3000, 65, 5200))]
    ys = [y.cpu().numpy() for y in F.Resampler(44100, 48000, nch=2, nstreams=3).convert_tracks_device(tracks)]
    r = F.Resampler(44100, 48000, nch=2, nstreams=3)
    views, peak, clipped = r.convert_tracks_to_pcm_device(tracks, S16, shaping="wannamaker9", segment=512, gain=1.5, dither=True, seed=SEED)
    assert views[0]._base is views[2]._base and views[0]._base.shape[0] == sum(y.shape[0] for y in ys)
    assert min(y.shape[0] for y in ys) < 512 < 3000 < max(y.shape[0] for y in ys)      # less than a segment, and several with a partial last one
    for t, y in enumerate(ys):
        want = SM.model(y[None], S16, SM.W9, 512, np.array([1.5]), True, (SEED + t * 2 * MIX) % 2 ** 64)
        assert np.array_equal(views[t].cpu().numpy().view(np.uint8).reshape(1, y.shape[0], 4), want[0]), t
        assert np.array_equal(peak[t].cpu().numpy().view(np.uint64), want[1][0]) and np.array_equal(clipped[t].cpu().numpy().view(np.uint64), want[2][0])
    plain = F.Resampler(44100, 48000, nch=2, nstreams=3).convert_tracks_to_pcm_device(tracks, S16, gain=1.5, dither=True, seed=SEED)
    assert not torch.equal(plain[0][0], views[0])                                      # shaping=None is the unshaped path
    # one stream, whole track: convert_track_to_pcm_device
    x = torch.from_numpy(music((4000,))[0][None]).cuda()
    y = F.Resampler(44100, 48000, nch=2).convert_track_device(x)
    got = F.Resampler(44100, 48000, nch=2).convert_track_to_pcm_device(x, S24, shaping="lipshitz5", segment=512, seed=SEED)
    want = SM.model(y.cpu().numpy(), S24, SM.L5, 512, None, True, SEED)
    assert len(got) == 3 and np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[2].cpu().numpy().view(np.uint64), want[2])
    # the windowed forms are not built
    with pytest.raises(ValueError, match="not built"):
        r.convert_tracks_to_pcm_streamed(tracks, S16, shaping="wannamaker9")
    with pytest.raises(ValueError, match="not built"):
        r.convert_library_to_pcm(tracks, S16, window=1024, shaping="wannamaker9")


def test_library_bytes_with_shaping_do_not_depend_on_the_stream_count():
    tracks = [torch.from_numpy(x).cuda() for x in music((2500, 0, 3100, 65, 2900))]
    got = {}
    for nstreams in (3, 2):
        r = F.Resampler(44100, 48000, nch=2, nstreams=nstreams)
        got[nstreams] = r.convert_library_to_pcm(tracks, S16, gain=[1.0, 1.0, 6.0, 1.0, 0.5], dither=True, seed=SEED, shaping="wannamaker9", segment=512)
        r.close()
    for a, b in zip(got[3][0], got[2][0]):
        assert torch.equal(a, b)
    assert torch.equal(got[3][1], got[2][1]) and torch.equal(got[3][2], got[2][2]) and int(got[3][2].sum()) > 0
    plain = F.Resampler(44100, 48000, nch=2, nstreams=3).convert_library_to_pcm(tracks, S16, gain=[1.0, 1.0, 6.0, 1.0, 0.5], dither=True, seed=SEED)
    assert not torch.equal(plain[0][0], got[3][0][0]) and torch.equal(plain[1], got[3][1])   # other bytes, the same peaks
