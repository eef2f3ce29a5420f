"""The limiter by windows on the device (RRX_tracks_limit_window_device; DESIGN.md 11, "Windows with the limiter"): window
partitions of ragged rows, each window from a minimal-coverage buffer, against tracks_limit_device on the whole rows, bit for bit,
in every format pair; past the grid.y split; against the host twin; and the streamed limited conversion against the whole-row
method."""
import ctypes as C

import numpy as np
import pytest
import torch

import foo_dsp_resampler_amd as F
import limit_model as M
import limit_window_cases as W

pytestmark = pytest.mark.gpu
GUARD = W.GUARD
DT = {np.float32: torch.float32, np.float64: torch.float64}


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def device_table(table):
    return torch.from_numpy(np.ascontiguousarray(table).view(np.int64)).cuda()


class Windows:
    """RRX_tracks_limit_window_device over the windows of one partition.  Every window gets a minimal-coverage buffer copied out of
    the rows at a pitch of `pad` frames more, the padding +inf so that a stray read shows -- everything of the rows outside the
    copied range is absent -- a destination of its own under GUARD, and a work buffer sized exactly with a guard behind it."""

    def __init__(self, rows, table, gain, L, H, dst_dtype, ceiling=W.CEILING, pad=3):
        self.rows, self.table, self.gain, self.L, self.H, self.ceiling, self.pad = rows, table, gain, L, H, ceiling, pad
        nt = rows.shape[0]
        self.out = torch.full(rows.shape, GUARD, dtype=dst_dtype, device="cuda")
        self.red = torch.ones((nt,), dtype=torch.float64, device="cuda")
        self.lim = torch.zeros((nt,), dtype=torch.int64, device="cuda")
        self.bad = torch.zeros((), dtype=torch.bool, device="cuda")
        self.phases, self.taps, coefs = F.TRUE_PEAK_FILTERS["bs1770"]
        self.co = (C.c_double * len(coefs))(*coefs)
        self.back, self.ahead = F.limit_window_reach(L, H)

    def window(self, first, frames):
        nt, row, nch = self.rows.shape
        b0, bn = W.coverage(first, frames, self.back, self.ahead, row)
        buf = torch.full((nt, bn + self.pad, nch), float("inf"), dtype=self.rows.dtype, device="cuda")
        buf[:, :bn] = self.rows[:, b0:b0 + bn]
        dst = torch.full((nt, frames + self.pad, nch), GUARD, dtype=self.out.dtype, device="cuda")
        need = F.tracks_limit_window_work_doubles(nt, frames, self.taps, self.L, self.H)
        work = torch.full((need + 8,), GUARD, dtype=torch.float64, device="cuda")
        rc = F.lib().RRX_tracks_limit_window_device(
            -1, None, C.c_void_p(self.table.data_ptr()), nt, nch, int(self.rows.dtype == torch.float64), C.c_void_p(buf.data_ptr()), bn + self.pad,
            b0, bn, row, first, frames, int(self.out.dtype == torch.float64), C.c_void_p(dst.data_ptr()), frames + self.pad,
            C.c_void_p(self.gain.data_ptr()) if self.gain is not None else None, self.ceiling, C.cast(self.co, C.c_void_p), self.phases,
            self.taps, self.L, self.H, C.c_void_p(self.red.data_ptr()), C.c_void_p(self.lim.data_ptr()), C.c_void_p(work.data_ptr()), need)
        assert rc == 0, rc
        self.bad |= (dst[:, frames:] != GUARD).any() | (work[need:] != GUARD).any()
        self.out[:, first:first + frames] = dst[:, :frames]  # the frames that were not emitted bring their sentinel along

    def run(self, windows):
        for first, frames in windows:
            self.window(first, frames)
        return self


@pytest.fixture(scope="module")
def batches():
    out = {}
    for nch in (1, 2, 17):
        rows, table, gain = W.batch(nch, np.float64)
        out[nch] = (rows, device_table(table), torch.from_numpy(gain).cuda())
    return out


@pytest.fixture(scope="module")
def whole(batches):
    """tracks_limit_device on the whole rows, into a tensor under GUARD: computed once per case, shared and left unchanged"""
    cache = {}

    def get(nch, L, H, src, dst):
        key = (nch, L, H, src, dst)
        if key not in cache:
            rows, table, gain = batches[nch]
            x = torch.from_numpy(rows.astype(src)).cuda()  # (float32 rows are the float64 noise rounded)
            want = torch.full(x.shape, GUARD, dtype=DT[dst], device="cuda")
            _, red, lim = F.tracks_limit_device(x, table, W.CEILING, gain=gain, lookahead=L, hold=H, out=want)
            cache[key] = (x, want, red, lim)
        return cache[key]
    return get


@pytest.mark.parametrize("src,dst", [(np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float32), (np.float64, np.float64)])
@pytest.mark.parametrize("L,H", W.LH)
@pytest.mark.parametrize("nch", (1, 2, 17))
def test_window_partitions_equal_the_whole_row_call(batches, whole, nch, L, H, src, dst):
    _, table, gain = batches[nch]
    x, want, wred, wlim = whole(nch, L, H, src, dst)
    before = x.clone()
    assert int((wlim > 0).sum()) >= 20
    for name, windows in W.partitions().items():
        w = Windows(x, table, gain, L, H, DT[dst]).run(windows)
        assert torch.equal(bits(w.out), bits(want)), name
        assert torch.equal(bits(w.red), bits(wred)) and torch.equal(w.lim, wlim), name
        assert not bool(w.bad), name
    assert torch.equal(bits(x), bits(before))


def test_the_launch_split():
    """32768 + 3 tracks of 64 mono frames in two windows: the smallest shape that crosses the grid.y split of every launch"""
    nt, row, L, H = 32768 + 3, 64, 7, 0
    gen = torch.Generator(device="cuda").manual_seed(9)
    rows = torch.randn((nt, row, 1), generator=gen, device="cuda") * 0.5
    table = np.zeros((nt, 6), np.uint64)
    table[:, 3] = np.arange(nt) % 5
    table[:, 4] = 64 - np.arange(nt) % 9
    table = device_table(table)
    want = torch.full(rows.shape, GUARD, dtype=torch.float32, device="cuda")
    _, wred, wlim = F.tracks_limit_device(rows, table, W.CEILING, lookahead=L, hold=H, out=want)
    for windows in ([(0, 29), (29, 35)], [(29, 35), (0, 29)]):
        w = Windows(rows, table, None, L, H, torch.float32).run(windows)
        assert torch.equal(bits(w.out), bits(want)) and torch.equal(bits(w.red), bits(wred)) and torch.equal(w.lim, wlim)
        assert not bool(w.bad)
    assert int((wlim[32768:] > 0).sum()) == 3 and int((wlim > 0).sum()) > 32000


def test_the_device_call_equals_the_host_twin():
    rows, table, gain = W.batch(2, np.float32)
    L, H = 72, 480
    windows = W.partitions()["widths-descending"]
    out = np.full(rows.shape, GUARD)
    red, lim = np.full(len(table), M.ONE), np.zeros(len(table), np.uint64)
    for first, frames in windows:
        W.twin_window(rows, table, gain, L, H, first, frames, out, red, lim)
    w = Windows(torch.from_numpy(rows).cuda(), device_table(table), torch.from_numpy(gain).cuda(), L, H, torch.float64).run(windows)
    assert np.array_equal(w.out.cpu().numpy().view(np.uint64), out.view(np.uint64))
    assert np.array_equal(w.red.cpu().numpy().view(np.uint64), red) and np.array_equal(w.lim.cpu().numpy().view(np.uint64), lim)
    assert not bool(w.bad)


def test_the_python_wrapper():
    """the wrapper allocates what it is not given, accumulates into what it is, and refuses a buffer that is one frame short"""
    rows, table, gain = W.batch(2, np.float32)
    x, tab, g = torch.from_numpy(rows).cuda(), device_table(table), torch.from_numpy(gain).cuda()
    L, H = 7, 3
    back, ahead = F.limit_window_reach(L, H)
    want = torch.full(x.shape, GUARD, dtype=torch.float32, device="cuda")
    _, wred, wlim = F.tracks_limit_device(x, tab, W.CEILING, gain=g, lookahead=L, hold=H, out=want)
    red = lim = None
    for first, frames in ((4000, 5000), (0, 4000)):
        b0, bn = W.coverage(first, frames, back, ahead)
        buf = x[:, b0:b0 + bn].contiguous()
        out, red, lim = F.tracks_limit_window_device(buf, tab, W.ROW, b0, first, frames, W.CEILING, gain=g, lookahead=L, hold=H, reduction=red,
                                                     limited=lim)
        assert tuple(out.shape) == (x.shape[0], frames, 2) and out.dtype == torch.float32
        for t, (of, n) in enumerate(W.clamped(table, W.ROW)):
            lo, hi = max(of, first), min(of + n, first + frames)
            if hi > lo:
                assert torch.equal(bits(out[t, lo - first:hi - first]), bits(want[t, lo:hi]))
    assert torch.equal(bits(red), bits(wred)) and torch.equal(lim, wlim)
    with pytest.raises(ValueError):
        F.tracks_limit_window_device(x[:, 3:5000].contiguous(), tab, W.ROW, 3, back + 2, 100, W.CEILING, lookahead=L, hold=H)
    with pytest.raises(ValueError):
        F.tracks_limit_window_device(x[:, :100 + ahead - 1].contiguous(), tab, W.ROW, 0, 0, 100, W.CEILING, lookahead=L, hold=H)
    with pytest.raises(ValueError):
        F.tracks_limit_window_device(x, tab, W.ROW, 0, 0, W.ROW, W.CEILING, lookahead=L, hold=H, out=x)


def bed_with_bursts(rate, seconds, nch, gen):
    """noise at -30 dBFS RMS with eight 40-frame fs/4 bursts at 0.9: loud transients over a quiet bed (as in test_gpu_limit.py)"""
    n = int(rate * seconds)
    x = torch.randn((n, nch), generator=gen, device="cuda") * 10.0 ** (-30.0 / 20.0)
    k = torch.arange(40, device="cuda", dtype=torch.float64)
    burst = (0.9 * torch.sin(2 * np.pi * k / 4 + np.pi / 4)).float()[:, None]
    for b in range(8):
        at = (b + 1) * n // 10
        x[at:at + 40] = burst
    return x.contiguous()


@pytest.fixture(scope="module")
def conversion():
    gen = torch.Generator(device="cuda").manual_seed(3)
    tracks = [bed_with_bursts(44100, s, 2, gen) for s in (0.1, 0.25, 0.4)]
    r = F.Resampler(44100, 48000, nch=2, nstreams=3)
    cache = {}

    def whole_rows(**kw):
        key = tuple(sorted((k, str(v)) for k, v in kw.items()))
        if key not in cache:
            r.reset()
            cache[key] = r.convert_tracks_to_pcm_loudness_limited(tracks, F.RRX_FMT_S16, **kw)
        return cache[key]
    return r, tracks, whole_rows


def same_returns(got, want):
    assert len(got) == len(want) == 8
    for a, b in zip(got[0], want[0]):
        assert torch.equal(a, b)
    for a, b in zip(got[1:], want[1:]):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(bits(a) if a.dtype.is_floating_point else a, bits(b) if b.dtype.is_floating_point else b)


@pytest.mark.parametrize("window,kw", [(None, dict()), (4096, dict()), (300, dict()), (300, dict(lookahead_ms=20.0)),
                                       (300, dict(album=[0, 1, 1], shaping="wannamaker3", segment=4096, dither=True, seed=5))],
                         ids=["whole-window", "4096", "300", "300-lookahead-20ms", "300-album-shaped"])
def test_streamed_limited_conversion_equals_the_whole_row_method(conversion, window, kw):
    r, tracks, whole_rows = conversion
    want = whole_rows(**kw)
    assert int((want[6] > 0).sum()) >= 1  # the limiter has lowered frames: the equality is not vacuous
    if "lookahead_ms" in kw:  # `ahead` exceeds a pulled window
        assert F.limit_window_reach(min(int(round(20.0 * 48)), 1024), int(round(10.0 * 48)))[1] > -(-300 * 48000 // 44100)
    r.reset()
    got = r.convert_tracks_to_pcm_streamed_loudness_limited(tracks, F.RRX_FMT_S16, window=window, **kw)
    same_returns(got, want)
