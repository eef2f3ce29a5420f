"""Noise-shaped dither in the windowed track path on the device (tracks_finish_shaped_window_kernel, csrc/finish_shaped.hip;
DESIGN.md 11, "Windows with noise shaping"): RRX_tracks_finish_shaped_window_device, tracks_finish_shaped_window_device and the two Resampler methods
built on it.

The bar throughout is EQUALITY of bits with the whole-row shaped forms, which tests/test_gpu_finish_shaped.py holds to the model:
windows that partition the rows, taken in ascending order with the state handed on, give the bytes, peaks and clip counts of
RRX_tracks_finish_shaped_device; the streamed conversions give convert_tracks_to_pcm_device(shaping=) and
convert_library_to_pcm(shaping=), in memory that does not grow with the longest track.  The wrong tables are a clamp at work, not a
fault provoked: guard bytes around the destination and around the state are looked at."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import foo_dsp_resampler_amd as F
import shaped_model as SM
import shaped_window_cases as W
from test_gpu_finish_shaped import tracks_device
from test_gpu_tracks_window import e2e_tracks

pytestmark = pytest.mark.gpu

S16, S24, S32 = F.RRX_FMT_S16, F.RRX_FMT_S24_3, F.RRX_FMT_S32
SEED = W.SEED
ORDERS = (4, 5, 9)                                            # kK = 4, 8 and 16
SEGMENTS = (0, 1, 16, 64)
GAINS = 0.5 + 0.4 * np.arange(len(W.SLICES))
PRE = {S16: 66, S24: 65, S32: 64}                             # the odd byte offsets even frames never give (tests/test_gpu_tracks_window.py)


def same(got, want, what):
    assert (got[0] is None) == (want[0] is None), what
    if want[0] is not None:
        assert np.array_equal(got[0], want[0]), ("output bytes", int((got[0] != want[0]).sum())) + what
    assert np.array_equal(got[1], want[1]), ("peak bit patterns",) + what      # kernel against kernel: a NaN is the same NaN
    assert np.array_equal(got[2], want[2]), ("clip counts",) + what


@pytest.mark.parametrize("nch", [1, 2, 3])
@pytest.mark.parametrize("double", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("fmt", [S16, S24, S32], ids=["s16", "s24", "s32"])
def test_windows_are_the_whole_row_call(fmt, double, nch):
    x = W.rows_of(len(W.SLICES), nch, fmt, double)
    tab, total = W.table_of()
    for order in ORDERS:
        coefs = SM.coefs_of(order)
        for segment in SEGMENTS:
            want = tracks_device(np.array(x), tab, total, fmt, coefs, segment, GAINS, True, pre=PRE[fmt])
            assert want[2].sum() > 0 and not (want[0] == W.GUARD).all()
            for name, part in W.PARTITIONS.items():
                got = W.device_windows(x, tab, total, part, fmt, True, coefs, segment, GAINS, True, pre=PRE[fmt])
                same(got, want, (fmt, double, nch, order, segment, name))
                assert not got[3][2].any()                   # the zero-length track: its state is handed on as zeros


@pytest.mark.parametrize("nch", [8, 257])
def test_windows_with_many_channels(nch):
    """more channels than a wave has lanes: the lanes of one segment span workgroups, and so do the lanes that hand a state on"""
    x = W.rows_of(len(W.SLICES), nch, S24, False)
    tab, total = W.table_of()
    want = tracks_device(np.array(x), tab, total, S24, SM.W9, 64, GAINS, True, pre=PRE[S24])
    for name in ("333", "on segment boundaries", "16 singles"):
        same(W.device_windows(x, tab, total, W.PARTITIONS[name], S24, True, SM.W9, 64, GAINS, True, pre=PRE[S24]), want, (nch, name))


def test_windows_measure_only_and_without_dither():
    x = W.rows_of(len(W.SLICES), 3, S16, False)
    tab, total = W.table_of()
    for dith in (True, False):
        want = tracks_device(np.array(x), tab, total, S16, SM.L5, 64, GAINS, dith, write=False)
        written = tracks_device(np.array(x), tab, total, S16, SM.L5, 64, GAINS, dith)
        for name in ("7", "333"):
            got = W.device_windows(x, tab, total, W.PARTITIONS[name], S16, False, SM.L5, 64, GAINS, dith)
            same(got, want, (dith, name))
            assert got[0] is None and np.array_equal(got[2], written[2]) and got[2].sum() > 0   # the clip count the write produces
            same(W.device_windows(x, tab, total, W.PARTITIONS[name], S16, True, SM.L5, 64, GAINS, dith), written, (dith, name, "written"))


def test_windows_on_a_side_stream():
    x = W.rows_of(len(W.SLICES), 2, S24, True)
    tab, total = W.table_of()
    want = tracks_device(np.array(x), tab, total, S24, SM.W9, 16, None, True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    dev = torch.cuda.current_device()
    with torch.cuda.stream(side):                            # the buffers are filled on the side stream
        got = W.device_windows(x, tab, total, W.PARTITIONS["7"], S24, True, SM.W9, 16, None, True, pre=64, stream=side)
    assert torch.cuda.current_device() == dev
    same(got, want, ("side stream",))


def test_windows_under_a_wrong_table_are_the_whole_row_call_under_it():
    x = W.rows_of(len(W.SLICES), 2, S24, False)
    tab, total = W.table_of()
    last = len(W.SLICES) - 1
    for bad in ((0, 0, 0, 5, 2 ** 40, int(tab[last, 5])), (0, 0, 0, 5, 130, 2 ** 50), (0, 0, 0, 2 ** 63, 130, int(tab[last, 5])),
                (0, 0, 0, 2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1)):
        t2 = tab.copy()
        t2[last] = bad
        want = tracks_device(np.array(x), t2, total, S24, SM.W9, 64, None, True)
        for name in ("7", "16 singles"):
            same(W.device_windows(x, t2, total, W.PARTITIONS[name], S24, True, SM.W9, 64, None, True, pre=64), want, (bad, name))


def test_long_rows_in_windows_of_4099():
    """some tens of thousands of frames at segment 16: every window holds hundreds of segments of every track, each cut at its own
    place, so a launch has many workgroups of lanes.  (The grid-stride loop behind 2^24 workgroups takes a second turn only for a
    window of some 2^30 lanes: no test reaches it, here or in the whole-row shaped kernels.)"""
    rows, nch = 40000, 2
    x = W.rows_of(3, nch, S16, False, rows)
    tab, total = W.table_of([(3, 39990), (1000, 20001), (4099, 30000)])
    want = tracks_device(np.array(x), tab, total, S16, SM.W9, 16, None, True, pre=PRE[S16])
    got = W.device_windows(x, tab, total, W.even(4099, rows), S16, True, SM.W9, 16, None, True, pre=PRE[S16])
    same(got, want, ("4099",))


@pytest.mark.parametrize("fmt", [S16, S24, S32], ids=["s16", "s24", "s32"])
def test_host_twin_equals_the_kernel(fmt):
    x = W.rows_of(len(W.SLICES), 2, fmt, fmt == S32)
    tab, total = W.table_of()
    for name in ("7", "on segment boundaries"):
        host = W.host_windows(x, tab, total, W.PARTITIONS[name], fmt, True, SM.W9, 64, GAINS, True)
        got = W.device_windows(x, tab, total, W.PARTITIONS[name], fmt, True, SM.W9, 64, GAINS, True)
        nan = np.isnan(host[1].view(np.float64))             # (a NaN channel's peak is a NaN on both sides)
        assert np.array_equal(got[0], host[0]) and np.array_equal(got[2], host[2]), (fmt, name)
        assert np.array_equal(got[1][~nan], host[1][~nan]) and np.isnan(got[1].view(np.float64)[nan]).all(), (fmt, name)
        assert np.array_equal(got[3].view(np.uint64), host[3].view(np.uint64)) and got[3].any(), (fmt, name)


def test_empty_windows_are_ok_and_touch_nothing():
    tab, total = W.table_of([(0, 40), (3, 30)])
    table = torch.from_numpy(tab.view(np.int64)).cuda()
    F.ratelib._ensure_init()
    win = torch.zeros((2, 8, 2), dtype=torch.float32, device="cuda")
    dst = torch.full((total, 2), 0x5a5a, dtype=torch.int16, device="cuda")
    stats = torch.zeros((2, 2), dtype=torch.int64, device="cuda")
    st = torch.full((2, 2, 2, 16), 77.0, dtype=torch.float64, device="cuda")
    k = np.array([1.0, -0.5])
    vp, fn = C.c_void_p, F.lib().RRX_tracks_finish_shaped_window_device
    for rows, first, sin in ((50, 0, None), (50, 17, st[0]), (50, 50, st[0]), (0, 0, None)):
        assert fn(-1, None, vp(table.data_ptr()), 2, 2, F.RRX_FMT_FLOAT, vp(win.data_ptr()), 8, rows, first, 0, S16, vp(dst.data_ptr()), total, None, 1, 0,
                  vp(k.ctypes.data), 2, 8, None if sin is None else vp(sin.data_ptr()), vp(st[1].data_ptr()), vp(stats.data_ptr()),
                  vp(stats.data_ptr())) == 0
    assert fn(-1, None, vp(table.data_ptr()), 2, 2, F.RRX_FMT_FLOAT, vp(win.data_ptr()), 8, 50, 17, 8, S16, vp(dst.data_ptr()), total, None, 1, 0,
              vp(k.ctypes.data), 2, 8, None, vp(st[1].data_ptr()), vp(stats.data_ptr()), vp(stats.data_ptr())) == 6   # no state behind frame 0
    torch.cuda.synchronize()
    assert (dst == 0x5a5a).all() and not stats.any() and (st == 77.0).all()


def test_python_call_returns_a_new_state_every_time():
    x = W.rows_of(len(W.SLICES), 2, S16, False)
    tab, total = W.table_of()
    want = tracks_device(np.array(x), tab, total, S16, SM.W9, 64, GAINS, True, pre=64)
    rows = torch.from_numpy(np.array(x)).cuda()
    table = torch.from_numpy(tab.view(np.int64)).cuda()
    g = torch.from_numpy(GAINS).cuda()
    out = pk = cl = state = None
    seen = []
    for wf, wn in W.PARTITIONS["333"]:
        win = rows[:, wf:wf + wn].contiguous()
        out, pk, cl, new = F.tracks_finish_shaped_window_device(win, table, W.R, wf, wn, S16, total, "wannamaker9", 64, gain=g, seed=SEED, state=state,
                                                                 out=out, peak=pk, clipped=cl)
        assert new is not state and all(new.data_ptr() != s.data_ptr() for s in seen) and tuple(new.shape) == (len(W.SLICES), 2, 16)
        seen.append(new)
        state = new
    same((out.cpu().numpy().view(np.uint8).reshape(-1), pk.cpu().numpy().view(np.uint64), cl.cpu().numpy().view(np.uint64)), want, ("python",))
    # an empty window: the state that came in, or zeros, and nothing else touched
    o2, p2, c2, s2 = F.tracks_finish_shaped_window_device(rows[:, :8].contiguous(), table, W.R, 100, 0, S16, total, "wannamaker9", 64, state=state,
                                                          out=out, peak=pk, clipped=cl)
    assert o2 is out and s2 is not state and torch.equal(s2, state)
    s3 = F.tracks_finish_shaped_window_device(rows[:, :8].contiguous(), table, W.R, 0, 0, S16, total, "wannamaker9", 64)[3]
    assert not s3.any()
    with pytest.raises(ValueError):
        F.tracks_finish_shaped_window_device(rows[:, :8].contiguous(), table, W.R, 8, 8, S16, total, "wannamaker9", 64)
    measured = F.tracks_finish_shaped_window_device(rows, table, W.R, 0, W.R, S16, total, "wannamaker9", 64, gain=g, seed=SEED, out=False)
    assert measured[0] is None and np.array_equal(measured[2].cpu().numpy().view(np.uint64), want[2])


# ---------------------------------------------------------------------------------------------------------------- end to end

def both_forms(fs, fo, lengths, nstreams, int16, window, fmt, shaping, segment, **kw):
    tracks = e2e_tracks(fs, lengths, int16)
    out = []
    for streamed in (False, True):
        r = F.Resampler(fs, fo, nch=2, nstreams=nstreams)    # a fresh handle each
        if streamed:
            out.append(r.convert_tracks_to_pcm_streamed_shaped(tracks, fmt, shaping, segment, window=window, **dict(kw)))
        else:
            out.append(r.convert_tracks_to_pcm_device(tracks, fmt, shaping=shaping, segment=segment, **dict(kw)))
        assert r.available == 0
        r.close()
    return out


@pytest.mark.parametrize("fs,fo,lengths,nstreams,int16,window,fmt,shaping,segment,kw", [
    (44100, 48000, (40, 65, 1500, 7000, 30000), 5, False, 4099, S16, "wannamaker9", 512, {}),                                      # A
    (44100, 48000, (40, 65, 1500, 7000, 30000), 5, False, 4099, S16, "wannamaker9", 65536, {}),                                    # A, one segment
    (96000, 44100, (70, 3000, 50000), 4, True, 10007, S24, "lipshitz5", 65536, dict(gain=1.9, dither=True, seed=SEED)),            # B
], ids=["A-512", "A-65536", "B"])
def test_streamed_shaped_conversion_equals_the_whole_row_form(fs, fo, lengths, nstreams, int16, window, fmt, shaping, segment, kw):
    plan = F.tracks_plan(fs, fo, lengths)
    assert plan.row_frames > 3 * window                      # several pushes, hence several output windows
    (views, peak, clipped), (sviews, speak, sclipped) = both_forms(fs, fo, lengths, nstreams, int16, window, fmt, shaping, segment, **kw)
    assert len(views) == len(sviews) == len(lengths)
    for t, (v, s) in enumerate(zip(views, sviews)):
        assert v.shape == s.shape and v.dtype == s.dtype and v.shape[0] == int(plan.table[t].out_frames)
        assert torch.equal(v, s), (t, int((v != s).sum()))
    assert sviews[0]._base is sviews[-1]._base                # one packed buffer
    assert torch.equal(peak.view(torch.int64), speak.view(torch.int64)) and torch.equal(clipped, sclipped)
    assert float(peak.max()) > 0.1


def test_streamed_shaped_refusals():
    r = F.Resampler(44100, 48000, nch=2, nstreams=2)
    x = [torch.zeros((100, 2), device="cuda")]
    with pytest.raises(ValueError):
        r.convert_tracks_to_pcm_streamed_shaped(x, S16, "wannamaker9", window=r.isamp_max + 1)
    with pytest.raises(ValueError):
        r.convert_tracks_to_pcm_streamed_shaped(x, S16, "nobody")
    with pytest.raises(ValueError):
        r.convert_tracks_to_pcm_streamed_shaped(x, None, "wannamaker9")
    with pytest.raises(ValueError):
        r.convert_tracks_to_pcm_streamed_shaped(x, S16, "wannamaker9", peak=torch.zeros((2, 2), dtype=torch.float64, device="cuda"))
    views, peak, clipped = r.convert_tracks_to_pcm_streamed_shaped([torch.zeros((0, 2), device="cuda")], S16, "wannamaker9")   # an empty track
    assert tuple(views[0].shape) == (0, 2) and not peak.any() and not clipped.any()
    r.close()


@functools.lru_cache(maxsize=None)
def library():
    from test_plugin_layer import music_like
    return tuple(torch.from_numpy(music_like(n, 2, 44100, 60 + i)).cuda() for i, n in enumerate((2500, 0, 3100, 65, 2900, 9000)))


def test_library_bytes_depend_neither_on_the_stream_count_nor_on_the_window():
    tracks = list(library())
    kw = dict(gain=[1.0, 1.0, 6.0, 1.0, 0.5, 1.0], dither=True, seed=SEED)
    r = F.Resampler(44100, 48000, nch=2, nstreams=3)
    want = r.convert_library_to_pcm(tracks, S16, shaping="wannamaker9", segment=512, **kw)
    r.close()
    assert int(want[2].sum()) > 0
    for nstreams in (2, 5):
        for window in (1000, 4099):
            r = F.Resampler(44100, 48000, nch=2, nstreams=nstreams)
            got = r.convert_library_to_pcm_streamed_shaped(tracks, S16, window, "wannamaker9", 512, **kw)
            r.close()
            for t, (a, b) in enumerate(zip(got[0], want[0])):
                assert a.shape == b.shape and torch.equal(a, b), (nstreams, window, t)
            assert torch.equal(got[1].view(torch.int64), want[1].view(torch.int64)) and torch.equal(got[2], want[2]), (nstreams, window)


def test_streamed_shaped_memory_is_bounded_by_the_windows():
    """The rise of torch's peak allocation over the call: at most the bound of
    tests/test_gpu_tracks_window.py::test_streamed_memory_is_bounded_by_the_windows -- the packed source, the destination, the two
    windows, the table and the statistics, plus 1 MiB -- and two state tensors of nstreams * nch * 16 doubles; the whole-row shaped
    form on the same input is above that bound."""
    fs, fo, lengths, nstreams, window = 44100, 48000, (40, 65, 1500, 7000, 30000), 5, 4099
    tracks = e2e_tracks(fs, lengths, False)
    plan = F.tracks_plan(fs, fo, lengths)
    win_out = -(-window * fo // fs)
    bound = (plan.src_total * 2 * 4 + plan.dst_total * 2 * 2 + nstreams * window * 2 * 4 + nstreams * win_out * 2 * 4 +
             nstreams * 48 + 2 * nstreams * 2 * 8 + (1 << 20)) + 2 * nstreams * 2 * 16 * 8
    rise = []
    for streamed in (True, False):
        r = F.Resampler(fs, fo, nch=2, nstreams=nstreams)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        if streamed:
            res = r.convert_tracks_to_pcm_streamed_shaped(tracks, S16, "wannamaker9", 512, window=window)
        else:
            res = r.convert_tracks_to_pcm_device(tracks, S16, shaping="wannamaker9", segment=512)
        torch.cuda.synchronize()
        rise.append(torch.cuda.max_memory_allocated() - before)
        del res
        r.close()
    print("bound", bound, "streamed shaped", rise[0], "whole rows shaped", rise[1])
    assert rise[0] <= bound, (rise, bound)
    assert rise[1] > bound, (rise, bound)
