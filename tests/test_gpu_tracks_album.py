"""Gapless albums on the device (csrc/tracks_album.hip; DESIGN.md 11, "Gapless albums"): tracks_stage_album_device against the numpy
model of tests/album_model.py, bit for bit, and the conversions with `gapless=` end to end.

What the model states -- the copied frames, neighbours included, and every zero -- is compared with it; the frames of an edge
without a link are tracks_stage_device's by contract and are compared with that call on the same table.  Sentinels around the rows
are looked at.  The shapes come from the copy kernel's tile (csrc/tracks_album.hpp): a track one sample under, at and over one
and two tiles, so that the borders of the regions fall on every side of a workgroup's seam."""
import functools

import numpy as np
import pytest

import album_cases as AC
import album_model as AM
import foo_dsp_resampler_amd as F
from oracle_binding import OracleDsp
from parity import assert_parity
from test_plugin_layer import music_like, run_track

pytestmark = pytest.mark.gpu

FS, FO = 44100, 48000
SENTINEL = 777.25
NONE = F.RRX_LINK_NONE


def tile_lengths(nch):
    t = AC.tile_samples()
    return [k * t // nch + d for k in (1, 2) for d in (-1, 0, 1)]


def batch(nch):
    """eight rows: two albums of three tracks around one and two tiles -- linked rows and album-edge rows -- and two singles"""
    return tile_lengths(nch) + [700, 70], [0, 0, 0, 1, 1, 1, -1, -1]


INSIDE = ([700, 3000, 100, 2500, 40], [5, 5, 5, 5, -1])     # the album begins inside the backward extension of its second track


def on_device(a, offset=0):
    """a host array as a device tensor whose first byte lies `offset` bytes behind an aligned allocation"""
    import torch
    a = np.ascontiguousarray(a)
    flat = torch.zeros(a.nbytes + 64, dtype=torch.uint8, device="cuda")
    flat[offset:offset + a.nbytes] = torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda()
    t = flat[offset:offset + a.nbytes].view({"float32": torch.float32, "int16": torch.int16, "int32": torch.int32, "uint8": torch.uint8}[str(a.dtype)])
    torch.cuda.synchronize()
    return t.view(a.shape)


def staged(call, n, R, nch):
    """call(out) on rows between two sentinel rows: the rows as numpy, with the sentinels checked and every frame written"""
    import torch
    big = torch.full((n + 2, R, nch), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    got = call(big[1:-1])
    torch.cuda.synchronize()
    assert got.data_ptr() == big[1:-1].data_ptr()
    host = big.cpu().numpy()
    assert (host[0] == SENTINEL).all() and (host[-1] == SENTINEL).all(), "rows around the batch were written"
    assert not (host[1:-1] == SENTINEL).any(), "a frame of a row was not written"
    return host[1:-1]


def check_stage(fmt, nch, lengths, groups, offset=0):
    import torch
    plan = F.tracks_plan_album(FS, FO, lengths, groups)
    table, links, R, S = plan.array(), plan.links_array(), plan.row_frames, plan.src_total
    raw, x = AC.source(fmt, S, nch, offset)
    packed = on_device(raw, offset)
    assert packed.data_ptr() % 4 == offset % 4
    keep = packed.clone()
    tab, lnk = plan.to_device("cuda"), plan.links_to_device("cuda")
    rows = staged(lambda out: F.tracks_stage_album_device(packed, tab, lnk, FS, FO, R, out=out), len(plan), R, nch)
    assert torch.equal(packed.view(torch.uint8), keep.view(torch.uint8)), "the packed source was written"
    want, written = AM.stage_model(table, links, x, R)
    w = np.broadcast_to(written[..., None], want.shape)
    assert (rows.view(np.uint32)[w] == want.view(np.uint32)[w]).all(), (fmt, nch, "copied frames and zeros")
    plain = F.tracks_stage_device(packed, tab, FS, FO, R).cpu().numpy()          # the extrapolated edges are that call's
    assert (rows.view(np.uint32)[~w] == plain.view(np.uint32)[~w]).all(), (fmt, nch, "extrapolated edges")
    return plan, packed, tab, rows, plain


@pytest.mark.parametrize("nch", [1, 2, 3, 6])
@pytest.mark.parametrize("fmt", AC.FORMATS)
def test_rows_are_the_model_bit_for_bit(fmt, nch):
    lengths, groups = batch(nch)
    plan, packed, tab, rows, plain = check_stage(fmt, nch, lengths, groups)
    t = AC.tile_samples()
    assert len(plan) == 8 and plan.row_frames * nch > 2 * t and max(lengths) <= 20000
    for k, at in ((1, 1), (4, 2)):                            # one frame under, at and over one tile and two, in whole frames
        assert [n - lengths[k] for n in lengths[k - 1:k + 2]] == [-1, 0, 1] and lengths[k] * nch <= at * t < (lengths[k] + 1) * nch
    assert (plan.links_array()[[1, 4]] != NONE).all() and (plan.links_array()[[6, 7]] == NONE).all()
    # a linked edge differs from the extrapolated one: the feature is at work
    assert not np.array_equal(rows[1], plain[1])
    # without links the call is tracks_stage_device, bit for bit
    none = staged(lambda out: F.tracks_stage_album_device(packed, tab, None, FS, FO, plan.row_frames, out=out), 8, plan.row_frames, nch)
    assert np.array_equal(none.view(np.uint32), plain.view(np.uint32))


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_s24_sources_at_every_byte_offset(offset):
    for nch in (1, 2):
        check_stage(F.RRX_FMT_S24_3, nch, *batch(nch), offset=offset)


@pytest.mark.parametrize("fmt", AC.FORMATS)
def test_an_album_that_begins_inside_an_extension(fmt):
    plan, _, _, rows, _ = check_stage(fmt, 2, *INSIDE)
    lead = int(plan.table[1].lead)
    assert lead > 700 and (rows[1, :lead - 700] == 0).all() and np.abs(rows[1, lead - 700:lead]).max() > 0


# ------------------------------------------------------------------------------------------------------------------ end to end

ALBUM = [9001, 64, 12000, 7000]                               # first and last above prime_len = 2205: the album's own LPC bases
SINGLE = 5000


@functools.lru_cache(maxsize=None)
def album_tracks():
    """a continuous stereo master cut into ALBUM, and a single behind it; read-only"""
    master = music_like(sum(ALBUM), 2, FS, 21)
    cuts = np.cumsum([0] + ALBUM)
    out = [master[a:b] for a, b in zip(cuts, cuts[1:])] + [music_like(SINGLE, 2, FS, 22)]
    for v in out:
        v.setflags(write=False)
    return master, tuple(out)


def device_tracks(dtype=np.float32):
    import torch
    out = []
    for v in album_tracks()[1]:
        a = v if dtype == np.float32 else np.rint(v.astype(np.float64) * 0.5 * 2.0 ** 15).astype(np.int16)
        out.append(torch.from_numpy(np.array(a)).cuda())
    torch.cuda.synchronize()
    return out


GROUPS = [3, 3, 3, 3, -1]


def one_stream_rows(rows, table):
    """every row pushed whole to a one-stream handle of its own, drained and pulled: the track's slice of what comes out"""
    import torch
    out = []
    for t, e in enumerate(table):
        r = F.Resampler(FS, FO, nch=2, nstreams=1)
        total = rows.shape[1]
        cap = total * FO // FS + 2
        y = torch.empty((1, cap, 2), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        got, step = 0, r.isamp_max
        for pos in range(0, total, step):
            r.push_device(rows[t:t + 1, pos:], min(step, total - pos), stride=total)
            while r.available:
                got += r.pull_device(y[:, got:], cap - got, stride=cap)
        r.drain()
        while r.available:
            got += r.pull_device(y[:, got:], cap - got, stride=cap)
        r.sync()
        assert got >= int(e.out_first + e.out_frames)
        out.append(y[0, int(e.out_first):int(e.out_first + e.out_frames)].cpu().numpy().copy())
        r.close()
    return out


def test_convert_tracks_device_gapless_is_the_album_as_one_track():
    import torch
    master, host = album_tracks()
    tracks = device_tracks()
    r = F.Resampler(FS, FO, nch=2, nstreams=5)
    ys = r.convert_tracks_device(tracks, gapless=GROUPS)
    torch.cuda.synchronize()
    ys = [y.cpu().numpy().copy() for y in ys]
    r.close()
    plan = F.tracks_plan_album(FS, FO, ALBUM + [SINGLE], GROUPS)
    assert [y.shape[0] for y in ys] == [int(e.out_frames) for e in plan.table]
    # every stream of the batch has the bits of a one-stream handle pushed the same row
    rows = F.tracks_stage_album_device(torch.cat(tracks).contiguous(), plan.to_device("cuda"), plan.links_to_device("cuda"), FS, FO, plan.row_frames)
    for t, (y, ref) in enumerate(zip(ys, one_stream_rows(rows, plan.table))):
        assert np.array_equal(y.view(np.uint32), ref.view(np.uint32)), ("row", t)
    # the album laid end to end against the plugin harness over the CPU resampler, fed the album as ONE track
    outs, _ = run_track(OracleDsp(FO), master, FS, [4096])
    ref = np.concatenate([c for c, _ in outs])
    got = np.concatenate(ys[:4])
    assert got.shape == ref.shape and ref.shape[0] == F.track_geometry(FS, FO, sum(ALBUM))[3]
    print("album as one track", assert_parity(got, ref))
    # the single is the single of the path without `gapless`
    r = F.Resampler(FS, FO, nch=2, nstreams=1)
    alone = r.convert_tracks_device([tracks[4]])[0].cpu().numpy()
    r.close()
    assert np.array_equal(alone.view(np.uint32), ys[4].view(np.uint32))
    # and without `gapless` the joins are not the album's: this is what the feature changes
    r = F.Resampler(FS, FO, nch=2, nstreams=5)
    islands = np.concatenate([y.cpu().numpy() for y in r.convert_tracks_device(tracks)[:4]])
    r.close()
    assert islands.shape != ref.shape or np.abs(islands - ref).max() > 1e-3


def as_host(views, peak, clipped):
    import torch
    torch.cuda.synchronize()
    return [v.cpu().numpy().tobytes() for v in views], peak.cpu().numpy().copy(), clipped.cpu().numpy().copy()


def assert_same(got, want, what):
    assert [len(b) for b in got[0]] == [len(b) for b in want[0]], what
    for i, (a, b) in enumerate(zip(got[0], want[0])):
        assert a == b, (what, "bytes of track", i)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), what


def test_streamed_equals_whole_rows_with_gapless():
    tracks = device_tracks(np.int16)
    kw = dict(gapless=GROUPS, dither=True, seed=0x1234567887654321, gain=1.5)
    r = F.Resampler(FS, FO, nch=2, nstreams=5)
    want = as_host(*r.convert_tracks_to_pcm_device(tracks, F.RRX_FMT_S16, **kw))
    r.reset()
    got = as_host(*r.convert_tracks_to_pcm_streamed(tracks, F.RRX_FMT_S16, window=1000, **kw))
    r.close()
    assert_same(got, want, "windows of 1000")
    plan = F.tracks_plan_album(FS, FO, ALBUM + [SINGLE], GROUPS)
    assert [len(b) for b in got[0]] == [int(e.out_frames) * 2 * 2 for e in plan.table]
    with pytest.raises(ValueError):
        r2 = F.Resampler(FS, FO, nch=2, nstreams=5)
        try:
            r2.convert_tracks_device(tracks, mix="swap", gapless=GROUPS)
        finally:
            r2.close()


def test_library_gapless_split_over_batches_equals_one_batch():
    """a five-track album and a single on two streams: the album's tracks land in three batches by length, and the packed
    destination still holds the album contiguous and in order, byte for byte what one batch of six streams writes"""
    import torch
    master = music_like(sum(ALBUM) + 3000, 2, FS, 31)
    lengths = ALBUM + [3000, SINGLE]
    groups = [0, 0, 0, 0, 0, -1]
    cuts = np.cumsum([0] + lengths[:5])
    host = [master[a:b] for a, b in zip(cuts, cuts[1:])] + [music_like(SINGLE, 2, FS, 32)]
    tracks = [torch.from_numpy(np.rint(v.astype(np.float64) * 0.5 * 2.0 ** 15).astype(np.int16)).cuda() for v in host]
    torch.cuda.synchronize()
    assert F.tracks_batches(FS, FO, lengths, 2).batches == [[2, 0], [3, 5], [4, 1]]
    one = F.Resampler(FS, FO, nch=2, nstreams=6)
    want = as_host(*one.convert_tracks_to_pcm_device(tracks, F.RRX_FMT_S24_3, gapless=groups, gain=1.25))
    one.close()
    for window in (None, 4096):
        r = F.Resampler(FS, FO, nch=2, nstreams=2)
        views, peak, clipped = r.convert_library_to_pcm(tracks, F.RRX_FMT_S24_3, gapless=groups, gain=1.25, window=window)
        assert_same(as_host(views, peak, clipped), want, ("library", window))
        # one packed destination, the album contiguous and in order in it
        base = views[0]._base if views[0]._base is not None else views[0]
        at = [v.data_ptr() - base.data_ptr() for v in views]
        assert all(at[k + 1] == at[k] + views[k].numel() for k in range(5)), at
        r.close()
