"""The limiter's release on the device (RRX_limit_release_device / RRX_tracks_limit_release_device, limit_release.hip) against the
numpy restatement of its arithmetic in limit_release_model.py, bit for bit: the summary, carry and run launches across their
workgroups, blocks and register tiles, strides and unaligned rows under guard values, in place and out of place, both formats on
either side, the per-track call, the Python wrappers and the conversion built on them.  The harness is test_gpu_limit.py's.

What the seams below are chosen by (limit_release.hip): a lane takes one block of `block` entries, 256 lanes to a workgroup, and
walks it in register tiles of 16 entries; a row has J = N + L - 1 entries.  A block is at least 64 entries, so it is the LAST
block of a row that can be one entry below, at and one above a tile (15, 16, 17), or a single entry; blocks of 65 and 100 entries
are no multiple of the tile and begin off a 128-byte line.  The summary and run launches take as many workgroups as the longest
row has pieces -- the grid's limit of 2^31 - 1 workgroups lies beyond any row of under 2^60 entries, so there is no capped grid to
walk past -- and the streams go to grid.y in chunks of 32768."""
import ctypes as C

import numpy as np
import pytest
import torch

import foo_dsp_resampler_amd as F
import limit_release_model as R
from test_gpu_limit import GUARD, TDT, as_bits, bed_with_bursts, rows_under_guards, same, signal
from test_gpu_limit import device as limit_device

pytestmark = pytest.mark.gpu
LH = [(1, 0), (64, 0), (72, 480), (1024, 4096)]
AB = [(R.coef(50, 44100), 64), (R.coef(200, 96000), 65), (R.coef(1000, 192000), 1024)]
SHAPES = [(1, 1, 1), (1, 2, 11), (3, 3, 4099), (2, 6, 1201), (2, 3, 70001), (2, 342, 40)]
# (nstreams, nch, frames, L, block): J = frames + L - 1
SEAMS = [(1, 2, 256 * 64 - 63, 64, 64),       # exactly 256 blocks: one full workgroup
         (2, 1, 256 * 64 - 62, 64, 64),       # 256 blocks + 1 entry: a second workgroup of one lane with one entry
         (1, 1, 1, 1, 64),                    # one entry
         (1, 2, 1, 64, 64), (1, 2, 2, 64, 64),                             # one block; one block + 1
         (2, 2, 3 * 64 + 15 - 63, 64, 64), (2, 2, 3 * 64 + 16 - 63, 64, 64), (2, 2, 3 * 64 + 17 - 63, 64, 64),   # the last block 15, 16, 17
         (2, 2, 5000, 72, 65), (1, 3, 5000, 72, 100), (1, 1, 257 * 65 + 1 - 71, 72, 65),                      # blocks off the tile
         (1, 2, 3000, 1024, 65536), (2, 1, 70000, 1, 65536)]                                                   # the longest block: one lane; two


def device(x, ceiling, L, H, a, block, coefs=R.BS1770, gain=None, dst=np.float64, pad=0, off=0, inplace=False, red=None, lim=None):
    """RRX_limit_release_device through the C ABI on x [nstreams, frames, nch], as test_gpu_limit.device does it: rows `pad` frames
    apart beyond their length, the first one `off` samples into a buffer filled with a guard value; the destination likewise, or
    the source itself; the work buffer three doubles longer than needed.  Everything outside the destination's frames must come
    back unchanged.  Returns (y, reduction bits, limited)."""
    ns, frames, nch = x.shape
    coefs = np.ascontiguousarray(coefs, dtype=np.float64)
    stride = frames + pad
    sdt, ddt = TDT[x.dtype], TDT[np.dtype(dst)]
    assert not inplace or sdt == ddt
    sbuf = torch.full((off + ns * stride * nch + 8,), GUARD, dtype=sdt, device="cuda")
    srows = sbuf[off:off + ns * stride * nch].view(ns, stride, nch)
    srows[:, :frames] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    dbuf = sbuf if inplace else torch.full((off + ns * stride * nch + 8,), GUARD, dtype=ddt, device="cuda")
    drows = dbuf[off:off + ns * stride * nch].view(ns, stride, nch)
    before_s, before_d = sbuf.clone(), dbuf.clone()
    d_red = torch.from_numpy((np.full(ns, R.ONE) if red is None else red).view(np.int64).copy()).cuda()
    d_lim = torch.from_numpy((np.zeros(ns, np.uint64) if lim is None else lim).view(np.int64).copy()).cuda()
    d_g = None if gain is None else torch.from_numpy(np.ascontiguousarray(gain, dtype=np.float64)).cuda()
    need = F.limit_release_work_doubles(ns, frames, coefs.shape[1], L, block)
    assert need == R.work_doubles(ns, frames, coefs.shape[1], L, block) and need > 0
    work = torch.full((need + 3,), GUARD, dtype=torch.float64, device="cuda")
    F.ratelib._ensure_init()
    torch.cuda.synchronize()
    rc = F.lib().RRX_limit_release_device(-1, None, int(x.dtype == np.float64), C.c_void_p(srows.data_ptr()), stride, int(np.dtype(dst) == np.float64),
                                          C.c_void_p(drows.data_ptr()), stride, ns, frames, nch, None if d_g is None else C.c_void_p(d_g.data_ptr()),
                                          float(ceiling), coefs.ctypes.data, coefs.shape[0], coefs.shape[1], L, H, float(a), block,
                                          C.c_void_p(d_red.data_ptr()), C.c_void_p(d_lim.data_ptr()), C.c_void_p(work.data_ptr()), need)
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((work[need:] == GUARD).all())
    y = drows[:, :frames].clone()
    if not inplace:
        assert torch.equal(as_bits(sbuf), as_bits(before_s))
    drows[:, :frames] = before_d[off:off + ns * stride * nch].view(ns, stride, nch)[:, :frames]  # put the frames back: the rest must be as it was
    assert torch.equal(as_bits(dbuf), as_bits(before_d))
    return y.cpu().numpy(), d_red.cpu().numpy().view(np.uint64), d_lim.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("nstreams,nch,frames", SHAPES)
def test_kernels_equal_the_model_bit_for_bit(nstreams, nch, frames):
    shape = (nstreams, nch, frames)
    x = signal(shape)
    gain = np.linspace(0.5, 1.7, nstreams)
    small = nstreams * nch * frames < 100000
    for i, (L, H) in enumerate(LH):
        for k, (a, block) in enumerate(AB):
            if not small and k != i % 3:  # (the long rows: every (L, H) and every (a, block), not every pair)
                continue
            want = R.limit_release(x, R.BS1770, 0.9, L, H, a, block, gain)
            same(device(x, 0.9, L, H, a, block, gain=gain), want, shape + (L, H, a, block))
            if (small and k == i % 3) or (L, H) == (72, 480):
                same(device(x, 0.9, L, H, a, block, gain=gain, pad=3, off=1), want, shape + (L, H, a, block, "strided, one sample off"))
                same(device(x, 0.9, L, H, a, block, gain=gain, dst=np.float32, inplace=True),
                     R.limit_release(x, R.BS1770, 0.9, L, H, a, block, gain, np.float32), shape + (L, H, a, block, "in place"))
    if small:
        for dtype in (np.float32, np.float64):
            x2 = signal(shape, dtype)
            for dst in (np.float32, np.float64):
                for g, (L, H), (a, block) in zip((None, 0.5, 1.7), ((64, 0), (72, 480), (1, 0)), AB):
                    g2 = None if g is None else np.full(nstreams, g)
                    same(device(x2, 0.7, L, H, a, block, gain=g2, dst=dst), R.limit_release(x2, R.BS1770, 0.7, L, H, a, block, g2, dst),
                         shape + (dtype, dst, g, L, H, a, block))


@pytest.mark.parametrize("nstreams,nch,frames,L,block", SEAMS)
def test_rows_at_and_one_past_the_seams_of_blocks_tiles_and_workgroups(nstreams, nch, frames, L, block):
    x = signal((nstreams, nch, frames))
    for a in (AB[0][0], AB[2][0]):
        same(device(x, 0.8, L, 0, a, block), R.limit_release(x, R.BS1770, 0.8, L, 0, a, block), (nstreams, nch, frames, L, block, a))


def test_more_streams_than_one_launch_takes():
    ns = 32768 + 3
    x = (np.random.default_rng(4).standard_normal((ns, 5, 1)) * 0.5).astype(np.float32)
    same(device(x, 0.5, 4, 3, AB[0][0], 64), R.limit_release(x, R.BS1770, 0.5, 4, 3, AB[0][0], 64), ("grid.y",))


def test_other_filter_shapes_and_accumulated_statistics():
    rng = np.random.default_rng(11)
    x = signal((2, 3, 4099))
    a, block = AB[1]
    for phases, taps in ((3, 5), (8, 16), (1, 1)):
        coefs = rng.standard_normal((phases, taps))
        same(device(x, 0.9, 72, 480, a, block, coefs=coefs), R.limit_release(x, coefs, 0.9, 72, 480, a, block), (phases, taps))
    # the statistics accumulate: a reduction already below what the call finds stays, the count is added to
    _, _, wred, wlim = R.limit_release(x, R.BS1770, 0.9, 64, 0, a, block)
    low = np.array([np.float64(1e-300).view(np.uint64), R.ONE])
    got = device(x, 0.9, 64, 0, a, block, red=low.copy(), lim=np.array([5, 7], np.uint64))
    assert np.array_equal(got[1], np.minimum(low, wred)) and np.array_equal(got[2], wlim + np.array([5, 7], np.uint64))
    # and over two calls on the same arrays
    again = device(x, 0.9, 64, 0, a, block, red=got[1].copy(), lim=got[2].copy())
    assert np.array_equal(again[1], got[1]) and np.array_equal(again[2], got[2] + wlim) and R.same_samples(again[0], got[0])


def test_release_zero_is_the_limiter_on_the_device():
    for shape in ((3, 3, 4099), (2, 6, 1201), (1, 2, 11)):
        for dtype, dst in ((np.float32, np.float32), (np.float64, np.float64), (np.float32, np.float64)):
            x = signal(shape, dtype)
            gain = np.linspace(0.5, 1.7, shape[0])
            for (L, H), block in zip(LH, (64, 65, 1024, 100)):
                y, red, lim = device(x, 0.9, L, H, 0.0, block, gain=gain, dst=dst)
                y0, red0, lim0 = limit_device(x, 0.9, L, H, gain=gain, dst=dst)
                assert y.tobytes() == y0.tobytes() and np.array_equal(red, red0) and np.array_equal(lim, lim0), (shape, dtype, dst, L, H, block)


def test_python_wrappers():
    x = signal((2, 3, 4099))
    t = torch.from_numpy(x).cuda()
    a = F.limit_release_coef(20, 48000)
    want = R.limit_release(x, R.BS1770, 0.9, 64, 0, a, 1024, np.full(2, 1.7), np.float32)

    def host(y, red, lim):
        return y.cpu().numpy(), red.cpu().numpy().view(np.uint64), lim.cpu().numpy().view(np.uint64)

    y, red, lim = F.limit_release_device(t, 0.9, a, gain=1.7)
    assert y.dtype == torch.float32 and y.data_ptr() != t.data_ptr() and torch.equal(as_bits(t), as_bits(torch.from_numpy(x).cuda()))
    same(host(y, red, lim), want, ("new tensor",))
    out = torch.empty(t.shape, dtype=torch.float64, device="cuda")
    y, red, lim = F.limit_release_device(t, 0.9, a, gain=torch.full((2,), 1.7, dtype=torch.float64, device="cuda"), lookahead=72, hold=480, block=65,
                                         out=out, stream=torch.cuda.current_stream())
    assert y is out
    same(host(y, red, lim), R.limit_release(x, R.BS1770, 0.9, 72, 480, a, 65, np.full(2, 1.7)), ("out",))
    y, red, lim = F.limit_release_device(t, 0.9, a, gain=1.7, out=t)
    assert y is t
    same(host(t, red, lim), want, ("in place",))
    y, red, lim = F.limit_release_device(torch.from_numpy(x[0]).cuda(), 0.9, a, filter=(3, 5, np.arange(15) / 15.0))
    same((y.cpu().numpy()[None],) + host(y, red, lim)[1:],
         R.limit_release(x[:1], (np.arange(15) / 15.0).reshape(3, 5), 0.9, 64, 0, a, 1024, None, np.float32), ("one stream",))
    y, red, lim = F.limit_release_device(torch.zeros((2, 0, 3), device="cuda"), 0.9, a)
    assert tuple(y.shape) == (2, 0, 3) and bool((red == 1.0).all()) and not lim.any()
    with pytest.raises(ValueError):
        F.limit_release_device(t, 0.9, 1.0)
    with pytest.raises(ValueError):
        F.limit_release_device(t, 0.9, a, block=63)


def table_of(slices):
    table = np.zeros((len(slices), 6), np.uint64)
    for t, (of, n) in enumerate(slices):
        table[t, 3:5] = (of, n)
    return table


def test_tracks_call_equals_one_stream_calls_on_each_slice():
    nch, row_frames = 2, 70100
    slices = [(0, 0), (3, 1), (17, 40), (1, 65), (333, 3000), (99, 70001), (70099, 1)]   # (out_first, out_frames), at odd offsets
    d_table = torch.from_numpy(table_of(slices).view(np.int64)).cuda()
    buf, rows = rows_under_guards(len(slices), row_frames, nch, 1)
    before = buf.clone()
    gain = torch.linspace(0.5, 1.7, len(slices), dtype=torch.float64, device="cuda")
    obuf, out = rows_under_guards(len(slices), row_frames, nch, 2, torch.float64)
    obefore, orows = obuf.clone(), out.clone()
    a = F.limit_release_coef(30, 48000)
    kw = dict(gain=gain, lookahead=72, hold=480, block=100)
    y, red, lim = F.tracks_limit_release_device(rows, d_table, 0.9, a, out=out, **kw)
    torch.cuda.synchronize()
    assert y is out and torch.equal(buf, before)
    inplace = rows.clone()
    y2, red2, lim2 = F.tracks_limit_release_device(inplace, d_table, 0.9, a, **kw)
    assert y2 is inplace and torch.equal(red2, red) and torch.equal(lim2, lim)
    x = rows.cpu().numpy()
    for t, (of, n) in enumerate(slices):
        # frames of the rows outside the slice are not written
        assert torch.equal(out[t, :of], orows[t, :of]) and torch.equal(out[t, of + n:], orows[t, of + n:])
        assert torch.equal(inplace[t, :of], rows[t, :of]) and torch.equal(inplace[t, of + n:], rows[t, of + n:])
        if not n:
            assert float(red[t]) == 1.0 and int(lim[t]) == 0
            continue
        one, one_red, one_lim = F.limit_release_device(rows[t, of:of + n].contiguous(), 0.9, a, gain=gain[t:t + 1], lookahead=72, hold=480, block=100,
                                                       out=torch.empty((n, nch), dtype=torch.float64, device="cuda"))
        assert torch.equal(as_bits(out[t, of:of + n]), as_bits(one)), t
        assert torch.equal(as_bits(red[t:t + 1]), as_bits(one_red)) and torch.equal(lim[t:t + 1], one_lim), t
        assert torch.equal(as_bits(inplace[t, of:of + n]), as_bits(one.float())), t  # (one rounding of the same double)
        if n <= 3000:  # and against the model for the short ones
            same((out[t:t + 1, of:of + n].cpu().numpy(), red[t:t + 1].cpu().numpy().view(np.uint64), lim[t:t + 1].cpu().numpy().view(np.uint64)),
                 R.limit_release(x[t:t + 1, of:of + n], R.BS1770, 0.9, 72, 480, a, 100, gain[t:t + 1].cpu().numpy()), ("track", t))
    out[:] = orows
    assert torch.equal(obuf, obefore)  # nothing but the rows was written


def test_a_wrong_table_gives_samples_and_stays_inside_the_rows():
    """out_first and out_frames beyond the row are clamped to it (tracks_slice): the guard rows around the buffers stay as they
    are, and what comes back is the clamped slices, limited.  That is a clamp at work, not a fault provoked."""
    nch, row_frames = 3, 500
    buf, rows = rows_under_guards(4, row_frames, nch, 2)
    before, was = buf.clone(), rows.clone()
    table = table_of([(100, 10 ** 9),           # runs past the end of its row: clamped to [100, 500)
                      (2 ** 63, 7),             # begins far outside: clamped to nothing
                      (499, 2 ** 64 - 1),       # the sum would wrap: clamped to [499, 500)
                      (0, 500)])                # a right entry
    d_table = torch.from_numpy(table.view(np.int64)).cuda()
    x = rows.cpu().numpy()
    a = AB[0][0]
    y, red, lim = F.tracks_limit_release_device(rows, d_table, 0.9, a, lookahead=1024, hold=4096, block=64)
    torch.cuda.synchronize()
    got = rows.clone()
    for t, (of, n) in enumerate([(100, 400), (500, 0), (499, 1), (0, 500)]):
        assert torch.equal(got[t, :of], was[t, :of]) and torch.equal(got[t, of + n:], was[t, of + n:])
        if n:
            same((got[t:t + 1, of:of + n].cpu().numpy(), red[t:t + 1].cpu().numpy().view(np.uint64), lim[t:t + 1].cpu().numpy().view(np.uint64)),
                 R.limit_release(x[t:t + 1, of:of + n], R.BS1770, 0.9, 1024, 4096, a, 64, None, np.float32), ("wrong table", t))
    rows.copy_(was)
    assert torch.equal(buf, before)


def test_convert_tracks_to_pcm_loudness_limited_with_a_release():
    nch, target, max_dbtp = 2, -14.0, -1.0
    ceiling = 10.0 ** (max_dbtp / 20.0)
    gen = torch.Generator(device="cuda").manual_seed(3)
    tracks = [torch.zeros((30000, nch), device="cuda"), torch.randn((60000, nch), generator=gen, device="cuda") * 0.05,
              bed_with_bursts(44100, 2.0, nch, gen)]
    r = F.Resampler(44100, 48000, nch=nch, nstreams=3)
    lookahead, hold = int(round(1.5 * 48)), int(round(10.0 * 48))

    def by_hand(limit):
        """the conversion's steps from the public calls, the limiter given"""
        r.reset()
        plan, table, rows = r._convert_tracks_rows(tracks)
        energy, hops = F.tracks_loudness_device(rows, table, 48000)
        gain, lufs = r._gain_by_loudness(energy, hops, 3, None, None, target, torch.cuda.current_stream())
        _, reduction, limited = limit(rows, table, gain)
        tp, pk = F.tracks_true_peak_device(rows, table)
        m = torch.maximum(tp, pk).amax(1)
        ok = torch.isfinite(m) & (m > 0)
        trim = torch.where(ok, torch.clamp(torch.full_like(m, ceiling) / torch.where(ok, m, torch.ones_like(m)), max=1.0), torch.ones_like(m)).contiguous()
        after = torch.maximum(*F.tracks_true_peak_device(rows, table, gain=trim)).amax(1)
        pcm, peak, clipped = F.tracks_finish_device(rows, table, F.RRX_FMT_S16, plan.dst_total, gain=trim)
        views = [pcm[int(e.dst_first):int(e.dst_first + e.out_frames)] for _, e in zip(range(3), plan.table)]
        return (views, peak[:3], clipped[:3], gain[:3], trim[:3], reduction[:3], limited[:3], lufs[:3]), after

    def equal(got, want):
        assert len(got) == 8 and all(torch.equal(a, b) for a, b in zip(got[0], want[0]))
        for a, b in zip(got[1:], want[1:]):
            assert a.dtype == b.dtype and torch.equal(as_bits(a) if a.dtype.is_floating_point else a, as_bits(b) if b.dtype.is_floating_point else b)

    # release_ms = None: the limiter without a release, as before
    want, _ = by_hand(lambda rows, table, gain: F.tracks_limit_device(rows, table, ceiling, gain=gain, lookahead=lookahead, hold=hold))
    r.reset()
    equal(r.convert_tracks_to_pcm_loudness_limited(tracks, F.RRX_FMT_S16, target_lufs=target, max_dbtp=max_dbtp), want)
    r.reset()
    equal(r.convert_tracks_to_pcm_loudness_limited(tracks, F.RRX_FMT_S16, target_lufs=target, max_dbtp=max_dbtp, release_ms=None, release_block=64), want)
    # release_ms = 100: the same steps around tracks_limit_release_device
    a = F.limit_release_coef(100, 48000)
    rel, after = by_hand(lambda rows, table, gain: F.tracks_limit_release_device(rows, table, ceiling, a, gain=gain, lookahead=lookahead, hold=hold,
                                                                                 block=1024))
    r.reset()
    got = r.convert_tracks_to_pcm_loudness_limited(tracks, F.RRX_FMT_S16, target_lufs=target, max_dbtp=max_dbtp, release_ms=100)
    equal(got, rel)
    for t in range(3):
        print("track %d: reduction %.6g, limited %d (without a release %d), trim %.17g, peak under trim %.17g (ceiling %.17g)"
              % (t, float(got[5][t]), int(got[6][t]), int(want[6][t]), float(got[4][t]), float(after[t]), ceiling))
        assert float(after[t]) <= ceiling * (1 + 1e-12)
    # the release lengthens the reduction; it deepens it by no more than the rounding of a * p + b * v on a plateau
    assert int(got[6][2]) > int(want[6][2]) > 0 and float(want[5][2]) * (1 - 1e-12) <= float(got[5][2]) <= float(want[5][2])
