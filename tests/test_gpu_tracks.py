"""Ragged track batches on the device (csrc/tracks.hip): the stage pass, the conversion of tracks of unequal
length through one batch handle, and the ragged output stage.

The bar is EQUALITY of bits with what a caller gets today, one track at a time:
  stage       every row == the buffer Resampler.convert_track_device builds for that track (the copy and two
              lpc_extrapolate_device calls), as uint32; the rest of the row all-zero bits;
  conversion  every track == convert_track_device of that track alone on a fresh one-stream handle, shape and bits (and, once,
              the plugin harness over the CPU resampler under the parity bar of tests/test_plugin_layer.py);
  finish      every track's bytes, peak and clip count == finish_device on its slice with the seed moved to its stream, as raw
              bytes, cross-checked against the numpy restatement of tests/finish_model.py.
The table lives on the device and is not validated, so the kernels clamp what they take from it: the contract tests hand them
wrong entries and look at sentinels around the buffers.  That is a clamp at work, not a fault provoked."""
import ctypes as C
import functools

import numpy as np
import pytest

import foo_dsp_resampler_amd as F
import finish_model as M
from oracle_binding import OracleDsp
from test_plugin_layer import music_like, run_track

pytestmark = pytest.mark.gpu

RR_INVPARAM = 6
SENTINEL = 123.0
GUARD = 0xA5
SEED = 0x1234567887654321
MIX = 0xBF58476D1CE4E5B9
STAGE_LENGTHS = [40, 64, 65, 100, 1500, 2205, 2206, 5000]   # both sides of the 64-frame branch, prime == frames, both sides of prime_len


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(got, want):
    """Bit for bit; where the reference has a NaN, a NaN (tests/test_gpu_lpc.py)."""
    g, w = bits(got).copy(), bits(want).copy()
    g[np.isnan(got)] = w[np.isnan(want)] = 0x7fc00000
    return np.array_equal(g, w)


def todays_row(x, fs, fo):
    """the `src` Resampler.convert_track_device builds for one track [frames, nch] (numpy in, numpy out)"""
    import torch
    frames = x.shape[0]
    n_add, _, prime_len, _ = F.edge_geometry(fs, fo)
    t = torch.from_numpy(x).cuda()
    if frames <= 64:
        return x
    prime = min(frames, prime_len)
    src = t.new_empty((n_add + frames + n_add, x.shape[1]))
    src[n_add:n_add + frames] = t
    F.lpc_extrapolate_device(src, n_add, prime, n_add, 0)
    F.lpc_extrapolate_device(src, n_add + frames - prime, prime, 0, n_add)
    return src.cpu().numpy()


def stage(tracks, fs, fo, table=None, stream=None):
    """tracks_stage_device on numpy tracks, rows inside a buffer with 16 sentinel frames at either end: the rows as numpy.
    `table` (uint64 [ntracks, 6]) replaces the plan's."""
    import torch
    plan = F.tracks_plan(fs, fo, [x.shape[0] for x in tracks])
    nch, n = tracks[0].shape[1], len(tracks)
    R = plan.row_frames
    packed = torch.from_numpy(np.concatenate(tracks)).cuda()
    keep = packed.clone()
    tab = plan.to_device("cuda") if table is None else torch.from_numpy(table.view(np.int64)).cuda()
    buf = torch.full((16 + n * R + 16, nch), SENTINEL, dtype=torch.float32, device="cuda")
    rows = buf[16:16 + n * R].view(n, R, nch)
    got = F.tracks_stage_device(packed, tab, fs, fo, R, out=rows, stream=stream)
    assert got is rows
    if stream is not None:
        stream.synchronize()
    host = buf.cpu().numpy()
    assert (host[:16] == SENTINEL).all() and (host[-16:] == SENTINEL).all(), "frames outside the rows were written"
    assert torch.equal(packed.view(torch.int32), keep.view(torch.int32)), "the packed source was written"
    return host[16:-16].reshape(n, R, nch), plan


@functools.lru_cache(maxsize=None)
def stage_case(nch):
    tracks = [music_like(n, nch, 44100, 50 + i) for i, n in enumerate(STAGE_LENGTHS)]
    rows, plan = stage(tracks, 44100, 48000)
    return tracks, rows, plan


@pytest.mark.parametrize("nch", [2, 3])
def test_stage_rows_are_todays_buffers_bit_for_bit(nch):
    tracks, rows, plan = stage_case(nch)
    assert plan.row_frames == 5000 + 2 * 2205
    for t, x in enumerate(tracks):
        want = todays_row(x, 44100, 48000)
        ext = want.shape[0]
        assert ext == x.shape[0] + 2 * int(plan.table[t].lead)
        diff = bits(rows[t, :ext]) != bits(want)
        print(nch, x.shape[0], "differing samples:", int(diff.sum()), "of", diff.size)
        assert not diff.any(), (nch, x.shape[0])
        assert not bits(rows[t, ext:]).any(), "the tail of a row is all-zero bits"


def test_stage_with_a_nan_in_one_channel():
    lengths = [100, 1500, 5000]
    tracks = [music_like(n, 2, 44100, 60 + i) for i, n in enumerate(lengths)]
    tracks[1][1500 - 1 - 16, 0] = np.nan      # inside the last 32 frames, and (prime == frames) inside the backward base too
    rows, _ = stage(tracks, 44100, 48000)
    for t, x in enumerate(tracks):
        want = todays_row(x, 44100, 48000)
        assert same_bits(rows[t, :want.shape[0]], want), t
        assert not bits(rows[t, want.shape[0]:]).any()
    ext = rows[1, :1500 + 2 * 2205]
    edges = np.concatenate([ext[:2205], ext[2205 + 1500:]])
    assert np.isnan(edges[:, 0]).all() and np.isfinite(edges[:, 1]).all()   # through the clamp, and in its channel only
    assert np.isfinite(rows[0]).all() and np.isfinite(rows[2]).all()


def alone(x, fs, fo):
    """convert_track_device of one track on a fresh one-stream handle: what a caller writes today"""
    import torch
    r = F.Resampler(fs, fo, nch=x.shape[1])
    y = r.convert_track_device(torch.from_numpy(x[None]).cuda())[0].cpu().numpy()
    r.close()
    return y


@functools.lru_cache(maxsize=None)
def converted(fs, fo, lengths, nstreams):
    import torch
    tracks = [music_like(n, 2, fs, 70 + i) for i, n in enumerate(lengths)]
    r = F.Resampler(fs, fo, nch=2, nstreams=nstreams)
    ys = [y.cpu().numpy() for y in r.convert_tracks_device([torch.from_numpy(x).cuda() for x in tracks])]
    assert r.available == 0
    r.close()
    return tracks, ys


# The second batch has one stream more than it has tracks.  Its 500000 frames are ONE push (isamp_max is 1048576 at this ratio), so
# the third batch adds a track of more than isamp_max frames: two pushes, and eleven seconds of input for the counters' wrap.
@pytest.mark.parametrize("fs,fo,lengths,nstreams", [(44100, 48000, (40, 65, 1500, 7000, 30000), 5), (96000, 44100, (70, 3000, 500000), 4),
                                                    (96000, 44100, (3000, 1100000), 2)])
def test_ragged_conversion_equals_a_handle_of_its_own(fs, fo, lengths, nstreams):
    tracks, ys = converted(fs, fo, lengths, nstreams)
    assert len(ys) == len(lengths)
    pieces = -(-F.tracks_plan(fs, fo, lengths).row_frames // F.describe_plan(fs, fo)["isamp_max"])
    assert pieces == (2 if max(lengths) > 1000000 else 1)
    for x, y in zip(tracks, ys):
        want = alone(x, fs, fo)
        assert y.shape == want.shape == (F.track_geometry(fs, fo, x.shape[0])[3], 2), (x.shape, y.shape, want.shape)
        diff = bits(y) != bits(want)
        print(fs, fo, x.shape[0], "->", y.shape[0], "differing samples:", int(diff.sum()))
        assert not diff.any(), x.shape


def test_ragged_conversion_matches_plugin_harness():
    from parity import assert_parity
    fs, fo = 44100, 48000
    tracks, ys = converted(fs, fo, (1500, 30000), 2)
    for x, y in zip(tracks, ys):
        outs, _ = run_track(OracleDsp(fo), x, fs, [4096])
        ref = np.concatenate([c for c, _ in outs])
        assert y.shape == ref.shape, (y.shape, ref.shape)
        print(x.shape[0], assert_parity(y, ref))


# ------------------------------------------------------------------------------------------------------------- ragged finish

NB = M.NBYTES
R_OUT = 1100                                                  # pitch of the output rows: several workgroups per row at nch = 3
# (out_first, out_frames): single frames so that consecutive tracks start at every byte offset a format and channel count can
# give (9-byte frames of 3-channel S24: 0, 1, 2, 3 mod 4), an empty track, one across workgroups, one that ends with its row
SLICES = [(0, 1), (3, 1), (2, 1), (7, 1), (1, 5), (9, 0), (4, 700), (R_OUT - 3, 3), (5, 130)]


def finish_table(slices=SLICES):
    tab = np.zeros((len(slices), 6), np.uint64)
    dst = 0
    for t, (of, n) in enumerate(slices):
        tab[t] = (0, 0, 0, of, n, dst)
        dst += n
    return tab, dst


@functools.lru_cache(maxsize=None)
def finish_rows(nch, fmt, double):
    """rows of noise at +-0.5 with the format's edge values (0, exact ties, +-1, +-3, a NaN ...) planted inside the tracks' own
    ranges and a huge value on either side of each range; read-only"""
    rng = np.random.default_rng([5, nch, fmt, int(double)])
    x = rng.uniform(-0.5, 0.5, (len(SLICES), R_OUT, nch))
    p = M.planted(M.BITS[fmt])
    for t, (of, n) in enumerate(SLICES):
        flat = x[t, of:of + n].reshape(-1)
        k = (np.arange(flat.size) * 7 + 3 * t) % len(p)
        put = rng.uniform(size=flat.size) < (1.0 if flat.size < 40 else 0.1)
        if t != 6:
            put &= k != 0                                    # the NaN goes into one track only
        flat[put] = p[k[put]]
        if of > 0:
            x[t, of - 1] = 1e30                              # not this track's: must not show in its peak or clip count
        if of + n < R_OUT:
            x[t, of + n] = -1e30
    x = x.astype(np.float64 if double else np.float32)
    x.setflags(write=False)
    return x


def ragged_finish(x, tab, dst_total, fmt, gain, dith, pre=64, post=64, stream=None):
    """tracks_finish_device with the destination `pre` bytes into a guarded byte buffer: (bytes of the destination or None,
    peak bit patterns, clipped); every byte around the destination must keep the guard pattern"""
    import torch
    n, _, nch = x.shape
    rows = torch.from_numpy(np.array(x)).cuda()
    table = torch.from_numpy(tab.view(np.int64)).cuda()
    g = None if gain is None else torch.from_numpy(np.ascontiguousarray(gain, dtype=np.float64)).cuda()
    out = buf = None
    if fmt is not None:
        nbytes = dst_total * nch * NB[fmt]
        buf = torch.full((pre + nbytes + post,), GUARD, dtype=torch.uint8, device="cuda")
        out = buf[pre:pre + nbytes]
        out = out.view(dst_total, nch * 3) if fmt == F.RRX_FMT_S24_3 else out.view(torch.int16 if fmt == F.RRX_FMT_S16 else torch.int32).view(dst_total, nch)
    _, pk, cl = F.tracks_finish_device(rows, table, fmt, dst_total, gain=g, dither=dith, seed=SEED, out=out, stream=stream)
    if stream is not None:
        stream.synchronize()
    raw = None
    if buf is not None:
        host = buf.cpu().numpy()
        assert (host[:pre] == GUARD).all() and (host[pre + nbytes:] == GUARD).all(), "bytes around the destination were written"
        raw = host[pre:pre + nbytes]
    return raw, pk.cpu().numpy().view(np.uint64), cl.cpu().numpy().view(np.uint64)


def per_track_reference(x, tab, fmt, gain, dith):
    """today's call, one track at a time: finish_device on each slice with the seed moved to the track's stream, and the numpy
    model of the same; (bytes, peak bits [ntracks, nch], clipped [ntracks, nch])"""
    import torch
    n, _, nch = x.shape
    parts, pk, cl = [], np.zeros((n, nch), np.uint64), np.zeros((n, nch), np.uint64)
    for t in range(n):
        of, cnt = int(tab[t, 3]), int(tab[t, 4])
        if not cnt:
            continue                                          # an empty track: no bytes, statistics untouched
        sl = np.array(x[t, of:of + cnt])[None]
        seed = (SEED + t * nch * MIX) % 2 ** 64
        g = None if gain is None else gain[t:t + 1]
        mo, mp, mc = M.model(sl, fmt, g, dith, seed, 0)
        o, p, c = F.finish_device(torch.from_numpy(sl).cuda(), fmt, gain=None if g is None else float(g[0]), dither=dith, seed=seed)
        p, c = p.cpu().numpy().view(np.uint64), c.cpu().numpy().view(np.uint64)
        nan = M.nan_channels(sl)
        assert np.array_equal(p[~nan], mp[~nan]) and np.array_equal(c, mc), t
        if fmt is not None:
            o = o.cpu().numpy().view(np.uint8).reshape(1, cnt, -1)
            assert np.array_equal(o, mo), t
            parts.append(o.reshape(-1))
        pk[t], cl[t] = p[0], c[0]
    return (np.concatenate(parts) if parts else None), pk, cl


@pytest.mark.parametrize("nch", [1, 2, 3])
@pytest.mark.parametrize("double", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("fmt", M.FORMATS, ids=["s16", "s24", "s32"])
def test_ragged_finish_is_the_per_track_call(fmt, double, nch):
    x = finish_rows(nch, fmt, double)
    tab, dst_total = finish_table()
    starts = {int(tab[t, 5]) * nch * NB[fmt] % 4 for t in range(len(SLICES))}
    assert starts == ({0, 1, 2, 3} if (nch * NB[fmt]) % 2 else {0, 2} if (nch * NB[fmt]) % 4 else {0}), starts
    gains = 0.5 + 0.4 * np.arange(len(SLICES))               # from 0.5 to 3.7: the planted +-1 and the noise clip under the larger ones
    for gain, dith, pre in ((None, False, 64), (gains, True, 65 if fmt == F.RRX_FMT_S24_3 else 66 if fmt == F.RRX_FMT_S16 else 64)):
        want_bytes, want_pk, want_cl = per_track_reference(x, tab, fmt, gain, dith)
        raw, pk, cl = ragged_finish(x, tab, dst_total, fmt, gain, dith, pre=pre)     # (pre: the odd byte offsets even frames never give)
        assert np.array_equal(raw, want_bytes), (fmt, double, nch, dith)
        assert np.array_equal(pk, want_pk) and np.array_equal(cl, want_cl), (fmt, double, nch, dith)
        assert want_cl.sum() > 0
        assert not cl[5].any() and not pk[5].any()           # the empty track
    # measure only: the statistics of the S32 quantiser, nothing written
    _, mpk, mcl = per_track_reference(x, tab, None, gains, True)
    raw, pk, cl = ragged_finish(x, tab, dst_total, None, gains, True)
    assert raw is None and np.array_equal(pk, mpk) and np.array_equal(cl, mcl)


# ------------------------------------------------------------------------------------------------------------------ contract

def test_refused_calls_write_nothing_and_keep_the_device():
    import torch
    dev, ndev = torch.cuda.current_device(), torch.cuda.device_count()
    plan = F.tracks_plan(44100, 48000, [100, 300])
    table = plan.to_device("cuda")
    packed = torch.zeros((400, 2), dtype=torch.float32, device="cuda")
    rows = torch.full((2, plan.row_frames, 2), SENTINEL, dtype=torch.float32, device="cuda")
    vp = C.c_void_p
    rc = F.lib().RRX_tracks_stage_device(ndev, None, 44100, 48000, vp(table.data_ptr()), 2, 2, vp(packed.data_ptr()), 400,
                                         vp(rows.data_ptr()), plan.row_frames)
    assert rc == RR_INVPARAM and torch.cuda.current_device() == dev
    dst = torch.full((plan.dst_total, 2), 0x5a5a, dtype=torch.int16, device="cuda")
    stats = torch.zeros((2, 2), dtype=torch.int64, device="cuda")
    rc = F.lib().RRX_tracks_finish_device(ndev, None, vp(table.data_ptr()), 2, 2, F.RRX_FMT_FLOAT, vp(rows.data_ptr()), plan.row_frames,
                                          F.RRX_FMT_S16, vp(dst.data_ptr()), plan.dst_total, None, 0, 0, vp(stats.data_ptr()), vp(stats.data_ptr()))
    assert rc == RR_INVPARAM and torch.cuda.current_device() == dev
    torch.cuda.synchronize()
    assert (rows == SENTINEL).all() and (dst == 0x5a5a).all() and not stats.any()


def test_a_side_stream_gives_the_same_bits():
    import torch
    tracks, rows, _ = stage_case(2)
    side = torch.cuda.Stream()
    dev = torch.cuda.current_device()
    with torch.cuda.stream(side):                            # the buffers are filled on the side stream
        got, _ = stage(list(tracks), 44100, 48000, stream=side)
    assert torch.cuda.current_device() == dev
    assert np.array_equal(bits(got), bits(rows))
    x = finish_rows(2, F.RRX_FMT_S24_3, False)
    tab, dst_total = finish_table()
    gains = np.full(len(SLICES), 1.7)
    want = ragged_finish(x, tab, dst_total, F.RRX_FMT_S24_3, gains, True)
    with torch.cuda.stream(side):
        got = ragged_finish(x, tab, dst_total, F.RRX_FMT_S24_3, gains, True, stream=side)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def test_a_wrong_table_stays_inside_the_buffers():
    """Entries no plan makes: the kernels clamp them to the source, to the track's own row and to the destination (sentinels and
    guard bytes are checked inside stage() and ragged_finish()), and the other tracks are not disturbed."""
    tracks = [music_like(n, 2, 44100, 80 + i) for i, n in enumerate([300, 200, 400])]
    good, plan = stage(tracks, 44100, 48000)
    R = plan.row_frames
    for bad in ((2 ** 40, 200, 2205, 0, 0, 0),               # a source position past src_total: reads as zeros
                (300, 2 ** 40, 2205, 0, 0, 0),               # more frames than the row holds
                (300, 200, 2 ** 62, 0, 0, 0),                # a lead beyond the row
                (2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1, 0, 0, 0),
                (850, 200, 0, 0, 0, 0),                      # the last 150 frames lie past the source
                (300, 20, 2205, 0, 0, 0)):                   # a lead with too few frames to extrapolate from: zeros
        tab = plan.array()
        tab[1] = bad
        rows, _ = stage(tracks, 44100, 48000, table=tab)
        assert np.array_equal(bits(rows[0]), bits(good[0])) and np.array_equal(bits(rows[2]), bits(good[2])), bad
        assert np.isfinite(rows[1]).all() and (rows[1] != SENTINEL).all(), bad     # every frame of the row is still written
    rows, _ = stage(tracks, 44100, 48000, table=np.ascontiguousarray(plan.array()[::-1]))   # right entries, wrong rows: written all the same
    assert (rows != SENTINEL).all()
    x = finish_rows(2, F.RRX_FMT_S24_3, False)
    tab, dst_total = finish_table()
    want = ragged_finish(x, tab, dst_total, F.RRX_FMT_S24_3, None, False)
    last = len(SLICES) - 1
    for bad, same in (((0, 0, 0, 5, 2 ** 40, int(tab[last, 5])), True),    # out_frames beyond row and destination: cut to what is left, its own 130 frames
                      ((0, 0, 0, 5, 130, 2 ** 50), False),                # a destination position past dst_total: nothing written
                      ((0, 0, 0, 2 ** 63, 130, int(tab[last, 5])), False),  # an output position past the row: nothing read or written
                      ((0, 0, 0, 2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1), False)):
        t2 = tab.copy()
        t2[last] = bad
        raw, pk, cl = ragged_finish(x, t2, dst_total, F.RRX_FMT_S24_3, None, False)
        own = int(tab[last, 5]) * 2 * 3
        assert np.array_equal(raw[:own], want[0][:own]), bad
        assert np.array_equal(pk[:last], want[1][:last]) and np.array_equal(cl[:last], want[2][:last]), bad
        if same:
            assert np.array_equal(raw[own:], want[0][own:]) and np.array_equal(pk, want[1])
        else:
            assert (raw[own:] == GUARD).all() and not pk[last].any() and not cl[last].any(), bad


def test_tracks_to_pcm_end_to_end():
    import torch
    fs, fo, lengths = 44100, 48000, (65, 1500, 7000)
    tracks, ys = converted(fs, fo, lengths, 3)
    r = F.Resampler(fs, fo, nch=2, nstreams=3)
    views, peak, clipped = r.convert_tracks_to_pcm_device([torch.from_numpy(x).cuda() for x in tracks], F.RRX_FMT_S24_3, gain=9.0, dither=True, seed=SEED)
    r.close()
    assert len(views) == 3 and tuple(peak.shape) == tuple(clipped.shape) == (3, 2)
    assert views[0]._base is views[2]._base and views[0]._base.shape[0] == sum(y.shape[0] for y in ys)   # one packed buffer
    for t, y in enumerate(ys):
        o, p, c = F.finish_device(torch.from_numpy(y[None]).cuda(), F.RRX_FMT_S24_3, gain=9.0, dither=True, seed=(SEED + t * 2 * MIX) % 2 ** 64)
        assert tuple(views[t].shape) == (y.shape[0], 6)
        assert torch.equal(views[t], o[0]) and torch.equal(peak[t], p[0]) and torch.equal(clipped[t], c[0]), t
    assert int(clipped.sum()) > 0                                   # (0.6 peak times 9: the gain clips)
