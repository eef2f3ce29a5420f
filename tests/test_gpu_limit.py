"""The true-peak limiter on the device (RRX_limit_device / RRX_tracks_limit_device, limit.hip) against the numpy restatement of
its arithmetic in limit_model.py, bit for bit: the three launches across their workgroups and tiles, strides and unaligned rows
under guard values, in place and out of place, both formats on either side, the per-track call, the Python wrappers and the
conversion built on them.

The tile sizes the seams below are chosen by (limit.hpp): the window-minimum launch gives 8192 - (L + H + D - 1) values of m per
tile, of which a row has N + L - 1 -- one past a tile is N = 8040 at (L, H) = (72, 0) and N = 2036 at (1024, 4096), D = 11 -- and
the smoothing launch takes 1024 frames per workgroup, four consecutive ones to a lane: N = 1025, and lengths that leave a lane
one, two or three frames (257, 1026, 1027), with look-aheads below the four frames of a lane.  The detector takes 256 detector frames per workgroup, of which a
row has N + D (one past: N = 246), and stages at most 15 channels at a time: 15, 16 and 31 channels sit on and past that seam.

A NaN sample stays a NaN and +-inf leaves a NaN in its own place (inf * 0); the model has them in the same places, and every
other sample is compared by its bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import foo_dsp_resampler_amd as F
import limit_model as M

pytestmark = pytest.mark.gpu
GUARD = 777.25
BS = np.ascontiguousarray(M.BS1770.reshape(-1))
LH = [(1, 0), (2, 1), (64, 0), (72, 480), (1024, 4096)]
SHAPES = [(1, 1, 1), (1, 2, 11), (1, 2, 12), (1, 2, 13), (3, 3, 4099), (2, 6, 1201), (2, 3, 70001), (2, 342, 40), (2, 1025, 40)]
SEAMS = [(1, 2, 8040, 72, 0), (1, 2, 2036, 1024, 4096), (2, 2, 257, 64, 0), (1, 2, 8039, 72, 0), (2, 2, 256, 64, 0), (2, 2, 246, 64, 0),
         (2, 2, 245, 64, 0), (2, 15, 246, 64, 0), (2, 16, 246, 64, 0), (1, 31, 300, 72, 480), (2, 2, 1025, 64, 0), (2, 2, 1024, 1024, 0),
         (1, 3, 1026, 1, 0), (1, 3, 1027, 3, 2)]
TDT = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}


def as_bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def device(x, ceiling, L, H, coefs=M.BS1770, gain=None, dst=np.float64, pad=0, off=0, inplace=False, red=None, lim=None):
    """RRX_limit_device through the C ABI on x [nstreams, frames, nch]: rows `pad` frames apart beyond their length, the first one
    `off` samples into a buffer filled with a guard value; the destination likewise, or the source itself.  Everything outside the
    destination's frames must come back unchanged.  Returns (y, reduction bits, limited)."""
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
    d_red = torch.from_numpy((np.full(ns, M.ONE) if red is None else red).view(np.int64).copy()).cuda()
    d_lim = torch.from_numpy((np.zeros(ns, np.uint64) if lim is None else lim).view(np.int64).copy()).cuda()
    d_g = None if gain is None else torch.from_numpy(np.ascontiguousarray(gain, dtype=np.float64)).cuda()
    need = F.limit_work_doubles(ns, frames, coefs.shape[1], L)
    assert need == M.work_doubles(ns, frames, coefs.shape[1], L)
    work = torch.full((need + 3,), GUARD, dtype=torch.float64, device="cuda")
    F.ratelib._ensure_init()
    torch.cuda.synchronize()
    rc = F.lib().RRX_limit_device(-1, None, int(x.dtype == np.float64), C.c_void_p(srows.data_ptr()), stride, int(np.dtype(dst) == np.float64),
                                  C.c_void_p(drows.data_ptr()), stride, ns, frames, nch, None if d_g is None else C.c_void_p(d_g.data_ptr()),
                                  float(ceiling), coefs.ctypes.data, coefs.shape[0], coefs.shape[1], L, H, C.c_void_p(d_red.data_ptr()),
                                  C.c_void_p(d_lim.data_ptr()), C.c_void_p(work.data_ptr()), need)
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((work[need:] == GUARD).all())
    y = drows[:, :frames].clone()
    if not inplace:
        assert torch.equal(as_bits(sbuf), as_bits(before_s))
    drows[:, :frames] = before_d[off:off + ns * stride * nch].view(ns, stride, nch)[:, :frames]  # put the frames back: the rest must be as it was
    assert torch.equal(as_bits(dbuf), as_bits(before_d))
    return y.cpu().numpy(), d_red.cpu().numpy().view(np.uint64), d_lim.cpu().numpy().view(np.uint64)


def same(got, want, what):
    y, red, lim = got
    wy, _, wred, wlim = want
    assert M.same_samples(y, wy), ("samples",) + tuple(what)
    assert np.array_equal(red, wred), ("reduction",) + tuple(what)
    assert np.array_equal(lim, wlim), ("limited",) + tuple(what)


_inputs = {}


def signal(shape, dtype=np.float32):
    """noise that crosses the ceilings used below in some frames and not in others; from 1000 frames on with the values that break
    careless arithmetic planted in it (0, +-1, -0.0, +-inf, denormals, one NaN), as in the true-peak tests"""
    key = (shape, np.dtype(dtype).name)
    if key not in _inputs:
        ns, nch, frames = shape
        rng = np.random.default_rng(sum(shape) + (dtype == np.float64))
        if frames >= 1000:
            x = M.planted(rng, (ns, frames, nch), dtype)
        else:
            x = (rng.standard_normal((ns, frames, nch)) * 0.5).astype(dtype)
        _inputs[key] = x
    return _inputs[key]


@pytest.mark.parametrize("nstreams,nch,frames", SHAPES)
def test_kernels_equal_the_model_bit_for_bit(nstreams, nch, frames):
    shape = (nstreams, nch, frames)
    x = signal(shape)
    gain = np.linspace(0.5, 1.7, nstreams)
    small = nstreams * nch * frames < 100000
    for L, H in LH:
        want = M.limit(x, M.BS1770, 0.9, L, H, gain)
        same(device(x, 0.9, L, H, gain=gain), want, shape + (L, H))
        if small or (L, H) == (72, 480):
            same(device(x, 0.9, L, H, gain=gain, pad=3, off=1), want, shape + (L, H, "strided, one sample off"))
            same(device(x, 0.9, L, H, gain=gain, dst=np.float32, inplace=True), M.limit(x, M.BS1770, 0.9, L, H, gain, np.float32),
                 shape + (L, H, "in place"))
    if small:
        for dtype in (np.float32, np.float64):
            x2 = signal(shape, dtype)
            for dst in (np.float32, np.float64):
                for g, (L, H) in ((None, (64, 0)), (0.5, (72, 480)), (1.7, (2, 1))):
                    g2 = None if g is None else np.full(nstreams, g)
                    same(device(x2, 0.7, L, H, gain=g2, dst=dst), M.limit(x2, M.BS1770, 0.7, L, H, g2, dst), shape + (dtype, dst, g, L, H))


@pytest.mark.parametrize("nstreams,nch,frames,L,H", SEAMS)
def test_rows_one_frame_past_a_tile_and_exactly_a_tile(nstreams, nch, frames, L, H):
    x = signal((nstreams, nch, frames))
    same(device(x, 0.8, L, H), M.limit(x, M.BS1770, 0.8, L, H), (nstreams, nch, frames, L, H))


def test_more_streams_than_one_launch_takes():
    ns = 32768 + 3
    x = (np.random.default_rng(4).standard_normal((ns, 5, 1)) * 0.5).astype(np.float32)
    same(device(x, 0.5, 4, 3), M.limit(x, M.BS1770, 0.5, 4, 3), ("grid.y",))


@pytest.mark.parametrize("off", [1, 2, 3])
def test_rows_off_a_16_byte_boundary_under_guards(off):
    for shape, dtype in (((2, 5, 1201), np.float32), ((2, 342, 40), np.float32), ((2, 5, 1201), np.float64)):
        x = signal(shape, dtype)
        gain = np.linspace(0.5, 1.7, shape[0])
        want = M.limit(x, M.BS1770, 0.9, 72, 480, gain, dtype)
        same(device(x, 0.9, 72, 480, gain=gain, dst=dtype, pad=2, off=off), want, shape + (off,))
        same(device(x, 0.9, 72, 480, gain=gain, dst=dtype, pad=2, off=off, inplace=True), want, shape + (off, "in place"))


def test_other_filter_shapes_and_accumulated_statistics():
    rng = np.random.default_rng(11)
    x = signal((2, 3, 4099))
    for phases, taps in ((3, 5), (8, 16), (1, 1)):
        coefs = rng.standard_normal((phases, taps))
        same(device(x, 0.9, 72, 480, coefs=coefs), M.limit(x, coefs, 0.9, 72, 480), (phases, taps))
    # the statistics accumulate: a reduction already below what the call finds stays, the count is added to
    y, _, wred, wlim = M.limit(x, M.BS1770, 0.9, 64, 0)
    low = np.array([np.float64(1e-300).view(np.uint64), M.ONE])
    got = device(x, 0.9, 64, 0, red=low.copy(), lim=np.array([5, 7], np.uint64))
    assert np.array_equal(got[1], np.minimum(low, wred)) and np.array_equal(got[2], wlim + np.array([5, 7], np.uint64))


def test_a_ceiling_above_every_level_returns_the_gained_frames():
    x = (np.random.default_rng(12).standard_normal((2, 3000, 3)) * 0.1).astype(np.float32)
    gain = np.array([0.5, 1.7])
    for dst in (np.float32, np.float64):
        y, red, lim = device(x, 50.0, 72, 480, gain=gain, dst=dst)
        want = (x.astype(np.float64) * gain[:, None, None]).astype(dst)
        assert M.same_samples(y, want) and np.all(red == M.ONE) and not lim.any()


def test_python_wrappers():
    x = signal((2, 3, 4099))
    t = torch.from_numpy(x).cuda()
    want = M.limit(x, M.BS1770, 0.9, 64, 0, np.full(2, 1.7), np.float32)
    y, red, lim = F.limit_device(t, 0.9, gain=1.7)
    assert y.dtype == torch.float32 and y.data_ptr() != t.data_ptr() and torch.equal(as_bits(t), as_bits(torch.from_numpy(x).cuda()))
    same((y.cpu().numpy(), red.cpu().numpy().view(np.uint64), lim.cpu().numpy().view(np.uint64)), want, ("new tensor",))
    out = torch.empty(t.shape, dtype=torch.float64, device="cuda")
    y, red, lim = F.limit_device(t, 0.9, gain=torch.full((2,), 1.7, dtype=torch.float64, device="cuda"), lookahead=72, hold=480, out=out,
                                 stream=torch.cuda.current_stream())
    assert y is out
    same((y.cpu().numpy(), red.cpu().numpy().view(np.uint64), lim.cpu().numpy().view(np.uint64)), M.limit(x, M.BS1770, 0.9, 72, 480, np.full(2, 1.7)),
         ("out",))
    y, red, lim = F.limit_device(t, 0.9, gain=1.7, out=t)
    assert y is t
    same((t.cpu().numpy(), red.cpu().numpy().view(np.uint64), lim.cpu().numpy().view(np.uint64)), want, ("in place",))
    y, red, lim = F.limit_device(torch.from_numpy(x[0]).cuda(), 0.9, filter=(3, 5, np.arange(15) / 15.0))
    same((y.cpu().numpy()[None], red.cpu().numpy().view(np.uint64), lim.cpu().numpy().view(np.uint64)),
         M.limit(x[:1], (np.arange(15) / 15.0).reshape(3, 5), 0.9, 64, 0, None, np.float32), ("one stream",))
    y, red, lim = F.limit_device(torch.zeros((2, 0, 3), device="cuda"), 0.9)
    assert tuple(y.shape) == (2, 0, 3) and bool((red == 1.0).all()) and not lim.any()
    with pytest.raises(TypeError):
        F.limit_device(t, 0.9, out=t.double()[:, :10])
    with pytest.raises(F.RRError):
        F.limit_device(t.view(-1)[:-3].view(-1, 3), 0.9, out=t.view(-1)[3:].view(-1, 3))  # overlapping, not equal


LENGTHS = [0, 1, 40, 65, 3000, 70001]


def rows_under_guards(ntracks, row_frames, nch, seed, dtype=torch.float32):
    """random rows [ntracks, row_frames, nch] inside a buffer with a guard row in front and behind"""
    buf = torch.full(((ntracks + 2) * row_frames * nch,), GUARD, dtype=dtype, device="cuda")
    rows = buf[row_frames * nch:(ntracks + 1) * row_frames * nch].view(ntracks, row_frames, nch)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    rows.copy_(torch.randn((ntracks, row_frames, nch), generator=gen, device="cuda") * 0.5)
    return buf, rows


def test_tracks_call_equals_one_stream_calls_on_each_slice():
    nch = 2
    plan = F.tracks_plan(44100, 48000, LENGTHS)
    table = plan.array()
    buf, rows = rows_under_guards(len(LENGTHS), plan.out_row_cap, nch, 1)
    before = buf.clone()
    gain = torch.linspace(0.5, 1.7, len(LENGTHS), dtype=torch.float64, device="cuda")
    obuf, out = rows_under_guards(len(LENGTHS), plan.out_row_cap, nch, 2, torch.float64)
    obefore, orows = obuf.clone(), out.clone()
    y, red, lim = F.tracks_limit_device(rows, plan.to_device("cuda"), 0.9, gain=gain, lookahead=72, hold=480, out=out)
    torch.cuda.synchronize()
    assert y is out and torch.equal(buf, before)
    inplace = rows.clone()
    y2, red2, lim2 = F.tracks_limit_device(inplace, plan.to_device("cuda"), 0.9, gain=gain, lookahead=72, hold=480)
    assert y2 is inplace and torch.equal(red2, red) and torch.equal(lim2, lim)
    x = rows.cpu().numpy()
    for t, e in enumerate(table):
        of, n = int(e[3]), int(e[4])
        assert n > 0 or LENGTHS[t] == 0
        # frames of the rows outside the slice are not written
        assert torch.equal(out[t, :of], orows[t, :of]) and torch.equal(out[t, of + n:], orows[t, of + n:])
        assert torch.equal(inplace[t, :of], rows[t, :of]) and torch.equal(inplace[t, of + n:], rows[t, of + n:])
        if not n:
            assert float(red[t]) == 1.0 and int(lim[t]) == 0
            continue
        assert of > 0 or LENGTHS[t] < 65  # (the longer tracks' rows hold frames in front of the slice: they must not act as history)
        one, one_red, one_lim = F.limit_device(rows[t, of:of + n].contiguous(), 0.9, gain=gain[t:t + 1], lookahead=72, hold=480,
                                               out=torch.empty((n, nch), dtype=torch.float64, device="cuda"))
        assert torch.equal(as_bits(out[t, of:of + n]), as_bits(one)), t
        assert torch.equal(as_bits(red[t:t + 1]), as_bits(one_red)) and torch.equal(lim[t:t + 1], one_lim), t
        assert torch.equal(as_bits(inplace[t, of:of + n]), as_bits(one.float())), t  # (one rounding of the same double)
        if t < 5:  # and against the model for the short ones
            same((out[t:t + 1, of:of + n].cpu().numpy(), red[t:t + 1].cpu().numpy().view(np.uint64), lim[t:t + 1].cpu().numpy().view(np.uint64)),
                 M.limit(x[t:t + 1, of:of + n], M.BS1770, 0.9, 72, 480, gain[t:t + 1].cpu().numpy()), ("track", t))
    out[:] = orows
    assert torch.equal(obuf, obefore)  # nothing but the rows was written


def test_a_wrong_table_gives_samples_and_stays_inside_the_rows():
    """out_first and out_frames beyond the row are clamped to it (tracks_slice): the guard rows around the buffers stay as they
    are, and what comes back is the clamped slices, limited.  That is a clamp at work, not a fault provoked."""
    nch, row_frames = 3, 500
    buf, rows = rows_under_guards(4, row_frames, nch, 2)
    before, was = buf.clone(), rows.clone()
    table = np.zeros((4, 6), np.uint64)
    table[0, 3:5] = (100, 10 ** 9)              # runs past the end of its row: clamped to [100, 500)
    table[1, 3:5] = (2 ** 63, 7)                # begins far outside: clamped to nothing
    table[2, 3:5] = (499, 2 ** 64 - 1)          # the sum would wrap: clamped to [499, 500)
    table[3, 3:5] = (0, 500)                    # a right entry
    d_table = torch.from_numpy(table.view(np.int64)).cuda()
    x = rows.cpu().numpy()
    y, red, lim = F.tracks_limit_device(rows, d_table, 0.9, lookahead=1024, hold=4096)
    torch.cuda.synchronize()
    got = rows.clone()
    for t, (of, n) in enumerate([(100, 400), (500, 0), (499, 1), (0, 500)]):
        assert torch.equal(got[t, :of], was[t, :of]) and torch.equal(got[t, of + n:], was[t, of + n:])
        if n:
            same((got[t:t + 1, of:of + n].cpu().numpy(), red[t:t + 1].cpu().numpy().view(np.uint64), lim[t:t + 1].cpu().numpy().view(np.uint64)),
                 M.limit(x[t:t + 1, of:of + n], M.BS1770, 0.9, 1024, 4096, None, np.float32), ("wrong table", t))
    rows.copy_(was)
    assert torch.equal(buf, before)


def bed_with_bursts(rate, seconds, nch, gen):
    """noise at -30 dBFS RMS with eight 40-frame fs/4 bursts at 0.9: loud transients over a quiet bed"""
    n = int(rate * seconds)
    x = torch.randn((n, nch), generator=gen, device="cuda") * 10.0 ** (-30.0 / 20.0)
    k = torch.arange(40, device="cuda", dtype=torch.float64)
    burst = (0.9 * torch.sin(2 * np.pi * k / 4 + np.pi / 4)).float()[:, None]
    for b in range(8):
        at = (b + 1) * n // 10
        x[at:at + 40] = burst
    return x.contiguous()


def test_convert_tracks_to_pcm_loudness_limited():
    nch, target, max_dbtp = 2, -14.0, -1.0
    ceiling = 10.0 ** (max_dbtp / 20.0)
    gen = torch.Generator(device="cuda").manual_seed(3)
    tracks = [torch.zeros((30000, nch), device="cuda"), torch.randn((60000, nch), generator=gen, device="cuda") * 0.05,
              bed_with_bursts(44100, 2.0, nch, gen)]
    r = F.Resampler(44100, 48000, nch=nch, nstreams=3)
    views, peak, clipped, gain, trim, reduction, limited, lufs = r.convert_tracks_to_pcm_loudness_limited(tracks, F.RRX_FMT_S16, target_lufs=target,
                                                                                                         max_dbtp=max_dbtp)
    assert len(views) == 3 and all(tuple(t.shape) == (3,) for t in (gain, trim, reduction, limited, lufs))
    assert float(gain[0]) == 1.0 and float(trim[0]) == 1.0 and int(limited[0]) == 0 and float(reduction[0]) == 1.0 and not views[0].any()
    assert float(lufs[0]) == float("-inf") and not clipped.any()
    for t in (1, 2):
        assert abs(float(gain[t]) / 10.0 ** ((target - float(lufs[t])) / 20.0) - 1) < 1e-12  # by loudness alone
        assert 0 < float(trim[t]) <= 1.0
    assert int(limited[2]) > 0 and float(reduction[2]) < 1.0
    # the same rows again (a handle's output is a function of its input): limited under the returned gain, re-measured under trim
    r.reset()
    plan, table, rows = r._convert_tracks_rows(tracks)
    lookahead, hold = int(round(1.5 * 48)), int(round(10.0 * 48))
    # the bursts are shorter than the window: the gain comes all the way down to what the highest level demands
    level = float(torch.maximum(*F.tracks_true_peak_device(rows, table, gain=gain)).amax(1)[2])
    assert level > ceiling and abs(float(reduction[2]) * level / ceiling - 1) < 1e-12
    F.tracks_limit_device(rows, table, ceiling, gain=gain, lookahead=lookahead, hold=hold)
    tp, pk = F.tracks_true_peak_device(rows, table, gain=trim)
    m = torch.maximum(tp, pk).amax(1)
    raw = torch.maximum(*F.tracks_true_peak_device(rows, table)).amax(1)
    for t in range(3):
        print("track %d: gain %.6g, reduction %.6g, limited %d, peak after the limiter %.9g, trim %.17g, peak under trim %.17g (ceiling %.17g)"
              % (t, float(gain[t]), float(reduction[t]), int(limited[t]), float(raw[t]), float(trim[t]), float(m[t]), ceiling))
        assert float(m[t]) <= ceiling * (1 + 1e-12)
    pcm, pk3, cl3 = F.tracks_finish_device(rows, table, F.RRX_FMT_S16, plan.dst_total, gain=trim)
    for t, e in enumerate(plan.table):
        assert torch.equal(views[t], pcm[int(e.dst_first):int(e.dst_first + e.out_frames)])
    assert torch.equal(pk3[:3], peak) and torch.equal(cl3[:3], clipped)
    energy, hops = F.tracks_loudness_device(rows, table, 48000, gain=trim)
    after = F.integrated_lufs(F.loudness_gate_device(energy, 4800, hops=hops))
    # what the peak-bound gain leaves for the same tracks
    r.reset()
    _, _, _, ngain, _, nlufs = r.convert_tracks_to_pcm_loudness_normalized(tracks, F.RRX_FMT_S16, target_lufs=target, max_dbtp=max_dbtp)
    assert torch.equal(nlufs, lufs)
    r.reset()
    plan, table, rows = r._convert_tracks_rows(tracks)
    energy, hops = F.tracks_loudness_device(rows, table, 48000, gain=ngain)
    normalized = float(F.integrated_lufs(F.loudness_gate_device(energy, 4800, hops=hops))[2])
    d_lim, d_norm = abs(float(after[2]) - target), abs(normalized - target)
    print("burst track: measured %.3f LUFS; limited to %.3f LUFS (%.3f LU from the target), peak-bound gain leaves %.3f LUFS (%.3f LU): margin %.3f LU"
          % (float(lufs[2]), float(after[2]), d_lim, normalized, d_norm, d_norm - d_lim))
    assert d_lim < d_norm
    # plain noise needs no limiter to speak of: both forms land on the target
    print("noise track: limited to %.3f LUFS, limited frames %d" % (float(after[1]), int(limited[1])))
    # albums and shaping take the same path
    r.reset()
    v2 = r.convert_tracks_to_pcm_loudness_limited(tracks, F.RRX_FMT_S16, target_lufs=target, max_dbtp=max_dbtp, album=[0, 1, 1], shaping="wannamaker3",
                                                  dither=True, seed=5)
    assert float(v2[3][1]) == float(v2[3][2]) and float(v2[7][1]) == float(v2[7][2]) and float(v2[3][0]) == 1.0
