"""Integer PCM sources of the ragged stage pass on the device (csrc/tracks.hip; DESIGN.md 11, "Integer sources"):
tracks_stage_device / convert_tracks_*_device fed int16, packed 3-byte S24 (uint8) and int32 tracks.

The bar throughout is EQUALITY of bits with the float call fed the numpy-converted source,
(s.astype(float64) * 2.0 ** -bits).astype(float32): the float call is held by tests/test_gpu_tracks.py and the conversion model is
numpy's, so nothing written together with the kernels under test is trusted.  The wrong tables are a clamp at work, not a fault
provoked: sentinels around the rows and the bytes around the source are looked at."""
import functools

import numpy as np
import pytest

import foo_dsp_resampler_amd as F
from test_plugin_layer import music_like

pytestmark = pytest.mark.gpu

FS, FO = 44100, 48000
SENTINEL = 123.0
SEED = 0x1234567887654321
BITS = {F.RRX_FMT_S16: 15, F.RRX_FMT_S24_3: 23, F.RRX_FMT_S32: 31}
FMTS = [F.RRX_FMT_S16, F.RRX_FMT_S24_3, F.RRX_FMT_S32]
IDS = ["s16", "s24", "s32"]
# both sides of the 64-frame branch, prime == frames, both sides of prime_len (2205); the odd lengths make tracks begin at every
# sample offset mod 2 (mono S16) and at every byte offset mod 4 (S24 with 3- and 9-byte frames); the longest row, 5001 + 2 * 2205
# frames, is more than one copy workgroup of 8192 samples
LENGTHS = [40, 65, 101, 1500, 2205, 2207, 5001]
PLANTED = {F.RRX_FMT_S16: [-2 ** 15, 2 ** 15 - 1],
           F.RRX_FMT_S24_3: [-2 ** 23, 2 ** 23 - 1, -1],                      # byte triples 00 00 80, ff ff 7f, ff ff ff
           F.RRX_FMT_S32: [-2 ** 31, 2 ** 31 - 1, 2 ** 24 + 1, 2 ** 24 + 3, 2 ** 25 + 2]}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def to_float(values, fmt):
    """the conversion model: one rounding, to nearest even"""
    return (values.astype(np.float64) * 2.0 ** -BITS[fmt]).astype(np.float32)


def to_raw(values, fmt):
    """integer samples [frames, nch] -> the array the call takes: int16 / int32 [frames, nch], or uint8 [frames, nch * 3]"""
    if fmt == F.RRX_FMT_S16:
        return values.astype(np.int16)
    if fmt == F.RRX_FMT_S32:
        return values.astype(np.int32)
    u = (values & 0xffffff).astype(np.uint32)
    return np.stack([u & 0xff, (u >> 8) & 0xff, u >> 16], axis=-1).astype(np.uint8).reshape(values.shape[0], -1)


@functools.lru_cache(maxsize=None)
def int_tracks(fmt, nch, lengths=tuple(LENGTHS)):
    """music_like at half of full scale, rounded; the format's extreme values planted in one track, inside its LPC base frames
    (read one sample at a time) and in its middle (read in groups); int64 [frames, nch] each, read-only"""
    out = []
    for i, n in enumerate(lengths):
        v = np.rint(music_like(n, nch, FS, 50 + i).astype(np.float64) * 0.5 * 2.0 ** BITS[fmt]).astype(np.int64)
        if n == max(lengths):
            flat = v.reshape(-1)
            p = PLANTED[fmt]
            for at in (7, flat.size // 2, flat.size // 2 + 101, flat.size - 9):
                flat[at:at + len(p)] = p
        v.setflags(write=False)
        out.append(v)
    return tuple(out)


def stage(packed, nch, lengths, table=None, stream=None):
    """tracks_stage_device on a device tensor of packed tracks, rows inside a buffer with 16 sentinel frames at either end: the
    rows as numpy.  `table` (uint64 [ntracks, 6]) replaces the plan's."""
    import torch
    plan = F.tracks_plan(FS, FO, lengths)
    n, R = len(lengths), plan.row_frames
    tab = plan.to_device("cuda") if table is None else torch.from_numpy(table.view(np.int64)).cuda()
    buf = torch.full((16 + n * R + 16, nch), SENTINEL, dtype=torch.float32, device="cuda")
    rows = buf[16:16 + n * R].view(n, R, nch)
    got = F.tracks_stage_device(packed, tab, FS, FO, R, out=rows, stream=stream)
    assert got is rows
    if stream is not None:
        stream.synchronize()
    host = buf.cpu().numpy()
    assert (host[:16] == SENTINEL).all() and (host[-16:] == SENTINEL).all(), "frames outside the rows were written"
    return host[16:-16].reshape(n, R, nch), plan


def stage_int(fmt, nch, tracks, offset=False, table=None, stream=None):
    """the integer call.  offset: the packed tensor is a view that starts one sample into a larger buffer, so that its base pointer
    has the alignment of one sample only.  The bytes of the source and around it must be unchanged."""
    import torch
    raw = to_raw(np.concatenate(tracks), fmt)
    flat = torch.from_numpy(raw.reshape(-1))
    width = 3 if fmt == F.RRX_FMT_S24_3 else 1                                   # elements a sample
    pre = width if offset else 0
    big = torch.full((pre + flat.numel() + 8,), 0x5a, dtype=flat.dtype).cuda()
    big[pre:pre + flat.numel()] = flat.cuda()
    keep = big.clone()
    packed = big[pre:pre + flat.numel()].view(raw.shape)
    assert packed.data_ptr() == big.data_ptr() + pre * flat.element_size()
    rows, plan = stage(packed, nch, [x.shape[0] for x in tracks], table=table, stream=stream)
    assert torch.equal(big, keep), "the packed source was written"
    return rows, plan


def stage_float(fmt, nch, tracks, table=None):
    """the float call on the numpy-converted source"""
    import torch
    packed = torch.from_numpy(to_float(np.concatenate(tracks), fmt)).cuda()
    return stage(packed, nch, [x.shape[0] for x in tracks], table=table)


@functools.lru_cache(maxsize=None)
def reference_rows(fmt, nch):
    rows, plan = stage_float(fmt, nch, int_tracks(fmt, nch))
    rows.setflags(write=False)
    return rows, plan


@functools.lru_cache(maxsize=None)
def staged_rows(fmt, nch):
    rows, _ = stage_int(fmt, nch, int_tracks(fmt, nch))
    rows.setflags(write=False)
    return rows


@pytest.mark.parametrize("nch", [1, 2, 3])
@pytest.mark.parametrize("fmt", FMTS, ids=IDS)
def test_stage_rows_equal_the_float_call_on_the_converted_source(fmt, nch):
    tracks = int_tracks(fmt, nch)
    want, plan = reference_rows(fmt, nch)
    assert plan.row_frames == 5001 + 2 * 2205 == 9411 and plan.row_frames * nch > 8192
    nbytes = nch * (3 if fmt == F.RRX_FMT_S24_3 else fmt // 8)
    starts = {int(e.src_first) * nbytes % 4 for e in plan.table}
    assert starts == ({0, 1, 2, 3} if nbytes % 2 else {0, 2} if nbytes % 4 else {0}), starts
    assert not (want == SENTINEL).any()
    for offset in (False, True):
        got = staged_rows(fmt, nch) if not offset else stage_int(fmt, nch, tracks, offset=True)[0]
        diff = bits(got) != bits(want)
        print(fmt, nch, "offset" if offset else "aligned", "differing samples:", int(diff.sum()), "of", diff.size)
        assert not diff.any(), (fmt, nch, offset)
    for t, x in enumerate(tracks):                                                # and the copied frames are the model's, stated directly
        lead = int(plan.table[t].lead)
        assert np.array_equal(bits(want[t, lead:lead + x.shape[0]]), bits(to_float(x, fmt)))


@pytest.mark.parametrize("nch", [1, 2, 3])
@pytest.mark.parametrize("fmt", [F.RRX_FMT_S16, F.RRX_FMT_S24_3], ids=["s16", "s24"])
def test_round_trip_gives_back_the_source_bytes(fmt, nch):
    import torch
    tracks = int_tracks(fmt, nch)
    rows = staged_rows(fmt, nch)
    _, plan = reference_rows(fmt, nch)
    for t, x in enumerate(tracks):
        lead = int(plan.table[t].lead)
        own = torch.from_numpy(np.array(rows[t, lead:lead + x.shape[0]])).cuda()
        out, _, clipped = F.finish_device(own, fmt)                               # no gain, no dither
        assert int(clipped.sum()) == 0
        assert np.array_equal(out.cpu().numpy().view(np.uint8).reshape(-1), to_raw(x, fmt).view(np.uint8).reshape(-1)), (fmt, nch, t)


@pytest.mark.parametrize("fmt", [F.RRX_FMT_S16, F.RRX_FMT_S24_3], ids=["s16", "s24"])
def test_a_wrong_table_reads_and_writes_as_the_float_call_does(fmt):
    """The tables of test_a_wrong_table_stays_inside_the_buffers (tests/test_gpu_tracks.py): the kernels clamp what they take
    from the table, the same way whatever the source holds."""
    lengths = (300, 200, 400)
    tracks = int_tracks(fmt, 2, lengths)
    plan = F.tracks_plan(FS, FO, lengths)
    for bad in ((850, 200, 0, 0, 0, 0),                      # src_first + frames past src_total: the last 150 frames read as zeros
                (850, 200, 2205, 0, 0, 0),                   # the same behind a lead: the LPC base frames are cut short too
                (300, 200, 2 ** 62, 0, 0, 0),                # a lead beyond the row
                (2 ** 40, 200, 2205, 0, 0, 0),               # a source position past src_total
                (2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1, 0, 0, 0)):
        tab = plan.array()
        tab[1] = bad
        got, _ = stage_int(fmt, 2, tracks, table=tab)
        want, _ = stage_float(fmt, 2, tracks, table=tab)
        assert np.array_equal(bits(got), bits(want)), bad
        assert (got != SENTINEL).all(), bad                  # every frame of every row is still written


def test_a_side_stream_gives_the_same_bits():
    import torch
    fmt, nch = F.RRX_FMT_S24_3, 3
    side = torch.cuda.Stream()
    dev = torch.cuda.current_device()
    with torch.cuda.stream(side):                            # the buffers are filled on the side stream
        got, _ = stage_int(fmt, nch, int_tracks(fmt, nch), stream=side)
    assert torch.cuda.current_device() == dev
    assert np.array_equal(bits(got), bits(staged_rows(fmt, nch)))


@pytest.mark.parametrize("fmt", [F.RRX_FMT_S16, F.RRX_FMT_S24_3], ids=["s16", "s24"])
def test_pcm_tracks_to_pcm_end_to_end(fmt):
    import torch
    lengths = (40, 65, 1500, 7000)
    tracks = int_tracks(fmt, 2, lengths)
    results = []
    for src in ([torch.from_numpy(to_raw(x, fmt)).cuda() for x in tracks], [torch.from_numpy(to_float(x, fmt)).cuda() for x in tracks]):
        r = F.Resampler(FS, FO, nch=2, nstreams=len(lengths))
        results.append(r.convert_tracks_to_pcm_device(src, fmt, dither=True, seed=SEED))
        r.close()
    (views, peak, clipped), (fviews, fpeak, fclipped) = results
    assert len(views) == len(fviews) == len(lengths)
    for t, (a, b) in enumerate(zip(views, fviews)):
        assert a.dtype == b.dtype and a.shape == b.shape and a.shape[0] == F.track_geometry(FS, FO, lengths[t])[3]
        assert torch.equal(a, b), t
    assert torch.equal(peak.view(torch.int64), fpeak.view(torch.int64)) and torch.equal(clipped, fclipped)
    assert float(peak.max()) > 0.1


def test_python_refusals():
    import torch
    r = F.Resampler(FS, FO, nch=2, nstreams=2)
    i16 = torch.zeros((100, 2), dtype=torch.int16, device="cuda")
    with pytest.raises(TypeError):
        r.convert_tracks_device([i16, torch.zeros((100, 2), dtype=torch.float32, device="cuda")])      # mixed dtypes
    with pytest.raises(TypeError):
        r.convert_tracks_device([i16, torch.zeros((100, 2), dtype=torch.int32, device="cuda")])
    with pytest.raises(TypeError):
        r.convert_tracks_device([torch.zeros((100, 2), dtype=torch.float64, device="cuda")])
    with pytest.raises(ValueError):
        r.convert_tracks_device([torch.zeros((100, 4), dtype=torch.uint8, device="cuda")])             # not nch * 3 bytes a frame
    with pytest.raises(ValueError):
        r.convert_tracks_to_pcm_device([torch.zeros((100, 2), dtype=torch.uint8, device="cuda")], F.RRX_FMT_S16)
    table = F.tracks_plan(FS, FO, [100]).to_device("cuda")
    with pytest.raises(ValueError):
        F.tracks_stage_device(torch.zeros((100, 4), dtype=torch.uint8, device="cuda"), table, FS, FO, 4510)
    with pytest.raises(TypeError):
        F.tracks_stage_device(torch.zeros((100, 2), dtype=torch.float64, device="cuda"), table, FS, FO, 4510)
    ys = r.convert_tracks_device([i16, i16[:70]])                                                       # and the handle is still good
    assert [tuple(y.shape) for y in ys] == [(F.track_geometry(FS, FO, n)[3], 2) for n in (100, 70)] and ys[0].dtype == torch.float32
    r.close()
