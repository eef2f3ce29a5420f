"""Channel mixing on the device (csrc/tracks_mix.hip; DESIGN.md 11, "Channel mixing"): tracks_stage_mix_device and its window
form, mix_device, and `mix=` on the track conversions.

The bar throughout is EQUALITY of bits with code that exists without the mix, fed numpy's mix (tests/mix_model.py):
tracks_stage_mix_device is held against tracks_stage_device on the float32 source whose frames are the model's mixed frames -- the
float call is held by tests/test_gpu_tracks.py, so nothing written together with the kernels under test is trusted.  The wrong
tables are a clamp at work, not a fault provoked: sentinels around the rows and the bytes around the source are looked at."""
import functools

import numpy as np
import pytest

import foo_dsp_resampler_amd as F
import mix_cases as MC
import mix_model as MM

pytestmark = pytest.mark.gpu

FS, FO = MC.FS, MC.FO
SENTINEL = 123.0
SEED = 0x1234567887654321
FMT_IDS = [MC.FMT_IDS[f] for f in MC.FMTS]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def stage(call, nch, lengths, table=None, stream=None):
    """a stage call -- call(device table, row_frames, rows) -- with the rows inside a buffer with 16 sentinel frames at either end:
    the rows as numpy.  `table` (uint64 [ntracks, 6]) replaces the plan's."""
    import torch
    plan = F.tracks_plan(FS, FO, lengths)
    n, R = len(lengths), plan.row_frames
    tab = plan.to_device("cuda") if table is None else torch.from_numpy(table.view(np.int64)).cuda()
    buf = torch.full((16 + n * R + 16, nch), SENTINEL, dtype=torch.float32, device="cuda")
    rows = buf[16:16 + n * R].view(n, R, nch)
    got = call(tab, R, rows)
    assert got is rows
    if stream is not None:
        stream.synchronize()
    host = buf.cpu().numpy()
    assert (host[:16] == SENTINEL).all() and (host[-16:] == SENTINEL).all(), "frames outside the rows were written"
    return host[16:-16].reshape(n, R, nch), plan


def source_view(raw, offset):
    """the packed source on the device as a view `offset` ELEMENTS into a larger buffer (bytes for packed S24, whole samples
    otherwise), so that its base pointer has the alignment of one sample only: (view, the larger buffer, its copy)"""
    import torch
    flat = torch.from_numpy(raw.reshape(-1))
    filler = 0x5a if flat.dtype != torch.float32 else 90.0
    big = torch.full((offset + flat.numel() + 8,), filler, dtype=flat.dtype).cuda()
    big[offset:offset + flat.numel()] = flat.cuda()
    packed = big[offset:offset + flat.numel()].view(raw.shape)
    assert packed.data_ptr() == big.data_ptr() + offset * flat.element_size()
    return packed, big, big.clone()


def stage_mix(fmt, M, tracks, offset=0, table=None, stream=None):
    """the mixed call.  The bytes of the source and around it must be unchanged."""
    import torch
    packed, big, keep = source_view(np.concatenate(tracks), offset)
    rows, plan = stage(lambda tab, R, rows: F.tracks_stage_mix_device(packed, tab, M, FS, FO, R, out=rows, stream=stream), M.shape[0],
                       [x.shape[0] for x in tracks], table=table, stream=stream)
    assert torch.equal(big, keep), "the packed source was written"
    return rows, plan


def mixed_source(fmt, M, tracks):
    """numpy's mix of the packed source: float32 [src_total, nch]"""
    return MM.mix_raw(np.concatenate(tracks), fmt, M)


def stage_reference(fmt, M, tracks, table=None):
    """the float call on the numpy-mixed source"""
    import torch
    packed = torch.from_numpy(mixed_source(fmt, M, tracks)).cuda()
    return stage(lambda tab, R, rows: F.tracks_stage_device(packed, tab, FS, FO, R, out=rows), M.shape[0], [x.shape[0] for x in tracks],
                 table=table)


@functools.lru_cache(maxsize=None)
def case(fmt, pair):
    """(matrix, tracks, reference rows, plan) of one (format, channel pair), computed once"""
    M = MC.MATRICES[pair]
    tracks = MC.tracks(fmt, M.shape[1], MC.lengths(fmt, M.shape[1]))
    want, plan = stage_reference(fmt, M, tracks)
    want.setflags(write=False)
    return M, tracks, want, plan


@pytest.mark.parametrize("pair", MC.PAIRS)
@pytest.mark.parametrize("fmt", MC.FMTS, ids=FMT_IDS)
def test_stage_rows_equal_the_float_call_on_the_mixed_source(fmt, pair):
    M, tracks, want, plan = case(fmt, pair)
    nch_src, tile = M.shape[1], MC.tile_frames(fmt, M.shape[1])
    lens = [x.shape[0] for x in tracks]
    assert {tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1} <= set(lens) and tile * nch_src * MC.BYTES[fmt] <= MC.tile_bytes()
    nbytes = nch_src * MC.BYTES[fmt]
    starts = {int(e.src_first) * nbytes % 4 for e in plan.table}
    assert starts == ({0, 1, 2, 3} if nbytes % 2 else {0, 2} if nbytes % 4 else {0}), starts
    assert not (want == SENTINEL).any()
    for offset in ((0, 1, 2, 3) if fmt == F.RRX_FMT_S24_3 else (0, 1)):      # S24: views at byte offsets 1 to 3
        got, _ = stage_mix(fmt, M, tracks, offset=offset)
        diff = bits(got) != bits(want)
        print(MC.FMT_IDS[fmt], pair, "offset", offset, "differing samples:", int(diff.sum()), "of", diff.size)
        assert not diff.any(), (fmt, pair, offset)
    mixed = mixed_source(fmt, M, tracks)                                      # and the copied frames are the model's, stated directly
    for t, e in enumerate(plan.table):
        lead, first, n = int(e.lead), int(e.src_first), lens[t]
        assert np.array_equal(bits(want[t, lead:lead + n]), bits(mixed[first:first + n]))


def test_the_identity_gives_the_rows_of_the_unmixed_stage():
    import torch
    fmt, nch = F.RRX_FMT_S32, 3
    tracks = MC.tracks(fmt, nch, (40, 65, 2300, 3001))
    got, _ = stage_mix(fmt, np.eye(nch), tracks)
    packed = torch.from_numpy(np.concatenate(tracks)).cuda()
    want, _ = stage(lambda tab, R, rows: F.tracks_stage_device(packed, tab, FS, FO, R, out=rows), nch, [x.shape[0] for x in tracks])
    assert np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("fmt", [F.RRX_FMT_FLOAT, F.RRX_FMT_S24_3], ids=["f32", "s24"])
def test_a_wrong_table_is_clamped_as_the_float_call_clamps_it(fmt):
    lengths = (300, 200, 400)
    M = MC.MATRICES["6to2"]
    tracks = MC.tracks(fmt, 6, lengths)
    plan = F.tracks_plan(FS, FO, lengths)
    for bad in ((850, 200, 0, 0, 0, 0),                      # src_first + frames past src_total: the last 150 frames are +0.0f
                (850, 200, 2205, 0, 0, 0),                   # the same behind a lead: the LPC base frames are cut short too
                (0, 2 ** 40, 0, 0, 0, 0),                    # frames past src_total and past the row
                (300, 200, 2 ** 62, 0, 0, 0),                # a lead beyond the row
                (300, 4000, 2205, 0, 0, 0),                  # lead + frames past the row: the row is cut
                (2 ** 40, 200, 2205, 0, 0, 0),               # a source position past src_total
                (2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1, 0, 0, 0)):
        tab = plan.array()
        tab[1] = bad
        got, _ = stage_mix(fmt, M, tracks, table=tab, offset=1)
        want, _ = stage_reference(fmt, M, tracks, table=tab)
        assert np.array_equal(bits(got), bits(want)), bad
        assert (got != SENTINEL).all(), bad                  # every frame of every row is still written
    tab = plan.array()
    tab[1] = (850, 200, 0, 0, 0, 0)
    got, _ = stage_mix(fmt, M, tracks, table=tab)
    assert np.array_equal(bits(got[1, 50:200]), np.zeros((150, 2), np.uint32))   # +0.0f, not -0.0f


@pytest.mark.parametrize("fmt,pair", [(F.RRX_FMT_S24_3, "6to2"), (F.RRX_FMT_FLOAT, "1to2"), (F.RRX_FMT_S16, "16to16")],
                         ids=["s24-6to2", "f32-1to2", "s16-16to16"])
def test_windows_have_the_bits_of_the_whole_rows(fmt, pair):
    import torch
    M = MC.MATRICES[pair]
    nch = M.shape[0]
    lengths = (40, 65, 2300, 3001)
    tracks = MC.tracks(fmt, M.shape[1], lengths)
    whole, plan = stage_mix(fmt, M, tracks)
    R, n = plan.row_frames, len(lengths)
    assert R == 3001 + 2 * 2205
    packed, big, keep = source_view(np.concatenate(tracks), 1)
    tab = plan.to_device("cuda")

    def window(first, frames, stride):
        buf = torch.full((n, stride, nch), SENTINEL, dtype=torch.float32, device="cuda")
        assert F.tracks_stage_mix_window_device(packed, tab, M, FS, FO, R, first, frames, out=buf) is buf
        host = buf.cpu().numpy()
        assert (host[:, frames:] == SENTINEL).all(), "frames behind the window were written"
        return host[:, :frames]

    # sizes 1, 63 and 1000; inside the backward extension (lead 2205), across its end, inside the forward extension of the 2300-
    # and the 3001-frame tracks, across the zeros, and the last frames of the rows
    for first, frames in ((0, 1), (2204, 1), (2205, 1), (R - 1, 1), (1000, 63), (2180, 63), (2205 + 2300 + 70, 63), (R - 63, 63),
                          (700, 1000), (2205 + 40 - 5, 1000), (2205 + 3001 + 100, 1000), (R - 1000, 1000)):
        got = window(first, frames, frames + 5)
        assert np.array_equal(bits(got), bits(whole[:, first:first + frames])), (first, frames)
    # a partition of the rows, descending
    out = np.full_like(whole, SENTINEL)
    edges = list(range(0, R, 1000)) + [R]
    for lo, hi in reversed(list(zip(edges[:-1], edges[1:]))):
        out[:, lo:hi] = window(lo, hi - lo, 1000)
    assert np.array_equal(bits(out), bits(whole))
    assert torch.equal(big, keep), "the packed source was written"


def rows_case(dtype, nstreams, frames, stride, dst_stride, M, stream=None):
    """mix_device on rows with pitches above `frames` and sentinel frames behind them, against the model and the hook"""
    import torch
    rng = np.random.default_rng(frames + nstreams)
    src = rng.standard_normal((nstreams, stride, M.shape[1])).astype(dtype)
    src[0, 0, 0] = -0.0
    x = torch.from_numpy(src).cuda()
    keep = x.clone()
    out = torch.full((nstreams, dst_stride, M.shape[0]), SENTINEL, dtype=x.dtype, device="cuda")
    assert F.mix_device(x, M, out=out, frames=frames, stream=stream) is out
    if stream is not None:
        stream.synchronize()
    got = out.cpu().numpy()
    assert torch.equal(x, keep), "the source rows were written"
    assert (got[:, frames:] == SENTINEL).all(), "frames outside [0, frames) were written"
    want = np.stack([MM.mix(src[s, :frames].astype(np.float64), M, dtype) for s in range(nstreams)])
    assert np.array_equal(bits(got[:, :frames]), bits(want)), (dtype, nstreams, frames)
    hook = np.full((nstreams, dst_stride, M.shape[0]), SENTINEL, dtype)
    Mc = np.ascontiguousarray(M, np.float64)
    rc = F.lib().RRX_debug_mix_host(F.RRX_FMT_DOUBLE if dtype == np.float64 else F.RRX_FMT_FLOAT, src.ctypes.data, stride, nstreams, frames,
                                    M.shape[1], hook.ctypes.data, dst_stride, M.shape[0], Mc.ctypes.data)
    assert rc == 0 and np.array_equal(bits(got), bits(hook))


@pytest.mark.parametrize("pair", ["1to2", "6to2", "16to16"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_mix_device_equals_the_model_and_the_hook(dtype, pair):
    M = MC.MATRICES[pair]
    tile = MC.tile_bytes() // (M.shape[1] * np.dtype(dtype).itemsize)
    for frames in (1, 63, 1025, tile, 2 * tile + 1):
        rows_case(dtype, 3, frames, frames + 7, frames + 3, M)


def test_mix_device_named_matrices_and_default_output():
    import torch
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((500, 2)).astype(np.float32)).cuda()
    for name in ("stereo_to_mono", "swap", "mid_side"):
        got = F.mix_device(x, name)
        assert tuple(got.shape) == (500, F.MIX_MATRICES[name].shape[0]) and got.dtype == torch.float32
        assert np.array_equal(bits(got.cpu().numpy()), bits(MM.mix(x.cpu().numpy().astype(np.float64), F.MIX_MATRICES[name])))
    with pytest.raises(ValueError):
        F.mix_device(x, "5.1_to_stereo")
    with pytest.raises(F.RRError):
        F.mix_device(x, "swap", out=x)                                         # d_dst == d_src is refused


def test_mix_device_past_the_grid_limit_of_streams():
    rows_case(np.float32, 65537, 2, 2, 2, MC.MATRICES["2to1"])


def test_mix_device_on_a_caller_stream():
    import torch
    side = torch.cuda.Stream()
    dev = torch.cuda.current_device()
    with torch.cuda.stream(side):
        rows_case(np.float64, 2, 1025, 1030, 1025, MC.MATRICES["6to2"], stream=side)
        M, tracks, want, _ = case(F.RRX_FMT_S24_3, "6to2")
        got, _ = stage_mix(F.RRX_FMT_S24_3, M, tracks, stream=side)
    assert torch.cuda.current_device() == dev
    assert np.array_equal(bits(got), bits(want))


def test_six_channel_tracks_to_stereo_pcm_end_to_end():
    import torch
    fmt, lengths = F.RRX_FMT_S24_3, (40, 65, 1500, 7000)
    M = F.mix_matrix("5.1_to_stereo")
    raw = MC.tracks(fmt, 6, lengths)
    six = [torch.from_numpy(np.array(x)).cuda() for x in raw]
    stereo = [torch.from_numpy(MM.mix_raw(x, fmt, M)).cuda() for x in raw]
    kw = dict(dither=True, seed=SEED)

    def same(a, b):
        (views, peak, clipped), (fviews, fpeak, fclipped) = a, b
        assert len(views) == len(fviews) == len(lengths)
        for t, (x, y) in enumerate(zip(views, fviews)):
            assert x.dtype == y.dtype == torch.int16 and tuple(x.shape) == (F.track_geometry(FS, FO, lengths[t])[3], 2)
            assert torch.equal(x, y), t
        assert torch.equal(peak.view(torch.int64), fpeak.view(torch.int64)) and torch.equal(clipped, fclipped)

    r = F.Resampler(FS, FO, nch=2, nstreams=len(lengths))
    want = r.convert_tracks_to_pcm_device(stereo, F.RRX_FMT_S16, **kw)
    assert float(want[1].max()) > 0.1
    r.reset()
    same(r.convert_tracks_to_pcm_device(six, F.RRX_FMT_S16, mix="5.1_to_stereo", **kw), want)
    r.reset()
    same(r.convert_tracks_to_pcm_device(stereo, F.RRX_FMT_S16, mix=None, **kw), want)
    r.reset()
    same(r.convert_tracks_to_pcm_streamed(six, F.RRX_FMT_S16, window=1000, mix=M, **kw), want)
    r.reset()
    ys, fs = r.convert_tracks_device(six, mix=M), None
    ys = [y.clone() for y in ys]
    r.reset()
    fs = r.convert_tracks_device(stereo)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(ys, fs))
    for window in (None, 1000):
        r.reset()
        lib_want = r.convert_library_to_pcm(stereo, F.RRX_FMT_S16, window=window, **kw)
        r.reset()
        same(r.convert_library_to_pcm(six, F.RRX_FMT_S16, window=window, mix="5.1_to_stereo", **kw), lib_want)
    # a matrix whose shape does not fit: the handle has two channels, the tracks six
    r.reset()
    for bad in ("stereo_to_mono", "7.1_to_stereo", np.zeros((3, 6))):
        with pytest.raises(ValueError):
            r.convert_tracks_to_pcm_device(six, F.RRX_FMT_S16, mix=bad)
    with pytest.raises(ValueError):
        r.convert_tracks_to_pcm_device(six, F.RRX_FMT_S16)                     # six channels without a mix
    same(r.convert_tracks_to_pcm_device(six, F.RRX_FMT_S16, mix=M, **kw), want)  # and the handle is still good
    r.close()
