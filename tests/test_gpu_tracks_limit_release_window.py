"""The limiter's release by windows on the device (RRX_tracks_limit_release_window_device; DESIGN.md 11, "Windows with the limiter's
release"): ascending window partitions of ragged rows, each window from a minimal-coverage buffer and the state of the one before,
against tracks_limit_release_device on the whole rows, bit for bit; the states against the host twin; past 256 pieces in a window
and past the grid.y split; release 0.0 against the plain window call; and the streamed limited conversion with release_ms against
the whole-row method."""
import ctypes as C

import numpy as np
import pytest
import torch

import foo_dsp_resampler_amd as F
import limit_release_model as R
import limit_release_window_model as RW
import limit_window_cases as W

pytestmark = pytest.mark.gpu
GUARD = W.GUARD
DT = {np.float32: torch.float32, np.float64: torch.float64}
AB = [(R.coef(50, 44100), 64), (R.coef(200, 96000), 65), (R.coef(1000, 192000), 1024)]
ASCENDING = ("one", "k1024", "widths", "random")


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def device_table(table):
    return torch.from_numpy(np.ascontiguousarray(table).view(np.int64)).cuda()


class Windows:
    """RRX_tracks_limit_release_window_device over the windows of one partition, in the order given, each with the state the one
    before left (the first: none).  Every window gets a minimal-coverage buffer copied out of the rows at a pitch of `pad` frames
    more, the padding +inf so that a stray read shows, a destination of its own under GUARD, and a work buffer and an outgoing
    state sized exactly with a guard behind each.  `states` keeps every outgoing state."""

    def __init__(self, rows, table, gain, L, H, a, block, dst_dtype, ceiling=W.CEILING, pad=3):
        self.rows, self.table, self.gain, self.L, self.H, self.a, self.block = rows, table, gain, L, H, a, block
        self.ceiling, self.pad = ceiling, pad
        nt = rows.shape[0]
        self.out = torch.full(rows.shape, GUARD, dtype=dst_dtype, device="cuda")
        self.red = torch.ones((nt,), dtype=torch.float64, device="cuda")
        self.lim = torch.zeros((nt,), dtype=torch.int64, device="cuda")
        self.bad = torch.zeros((), dtype=torch.bool, device="cuda")
        self.phases, self.taps, coefs = F.TRUE_PEAK_FILTERS["bs1770"]
        self.co = (C.c_double * len(coefs))(*coefs)
        self.back, self.ahead = F.limit_window_reach(L, H)
        self.state, self.states = None, []

    def window(self, first, frames):
        nt, row, nch = self.rows.shape
        b0, bn = W.coverage(first, frames, self.back, self.ahead, row)
        buf = torch.full((nt, bn + self.pad, nch), float("inf"), dtype=self.rows.dtype, device="cuda")
        buf[:, :bn] = self.rows[:, b0:b0 + bn]
        dst = torch.full((nt, frames + self.pad, nch), GUARD, dtype=self.out.dtype, device="cuda")
        need = F.tracks_limit_release_window_work_doubles(nt, frames, self.taps, self.L, self.H, self.block)
        assert need == RW.work_doubles(nt, frames, self.taps, self.L, self.H, self.block) and need > 0
        work = torch.full((need + 8,), GUARD, dtype=torch.float64, device="cuda")
        sout = torch.full((nt * RW.STATE + 8,), GUARD, dtype=torch.float64, device="cuda")
        rc = F.lib().RRX_tracks_limit_release_window_device(
            -1, None, C.c_void_p(self.table.data_ptr()), nt, nch, int(self.rows.dtype == torch.float64), C.c_void_p(buf.data_ptr()), bn + self.pad,
            b0, bn, row, first, frames, int(self.out.dtype == torch.float64), C.c_void_p(dst.data_ptr()), frames + self.pad,
            C.c_void_p(self.gain.data_ptr()) if self.gain is not None else None, self.ceiling, C.cast(self.co, C.c_void_p), self.phases,
            self.taps, self.L, self.H, self.a, self.block, C.c_void_p(self.state.data_ptr()) if self.state is not None else None,
            C.c_void_p(sout.data_ptr()), C.c_void_p(self.red.data_ptr()), C.c_void_p(self.lim.data_ptr()), C.c_void_p(work.data_ptr()), need)
        assert rc == 0, rc
        self.bad |= (dst[:, frames:] != GUARD).any() | (work[need:] != GUARD).any() | (sout[nt * RW.STATE:] != GUARD).any()
        self.out[:, first:first + frames] = dst[:, :frames]  # the frames that were not emitted bring their sentinel along
        self.state = sout[:nt * RW.STATE].reshape(nt, RW.STATE).clone()
        self.states.append(self.state)

    def run(self, windows):
        for first, frames in windows:
            self.window(first, frames)
        return self


@pytest.fixture(scope="module")
def batches():
    out = {}
    for nch in (1, 2):
        for dtype in (np.float32, np.float64):
            rows, table, gain = W.batch(nch, dtype)
            out[nch, dtype] = (rows, table, gain, torch.from_numpy(rows).cuda(), device_table(table), torch.from_numpy(gain).cuda())
    return out


@pytest.mark.parametrize("ab", range(len(AB)))
@pytest.mark.parametrize("L,H", W.LH)
@pytest.mark.parametrize("dtype", (np.float32, np.float64), ids=("float32", "float64"))
@pytest.mark.parametrize("nch", (1, 2))
def test_ascending_windows_equal_the_whole_row_release(batches, nch, dtype, L, H, ab):
    rows, table, gain, x, tab, g = batches[nch, dtype]
    a, block = AB[ab]
    want = torch.full(x.shape, GUARD, dtype=DT[dtype], device="cuda")
    _, wred, wlim = F.tracks_limit_release_device(x, tab, W.CEILING, a, gain=g, lookahead=L, hold=H, block=block, out=want)
    assert int((wlim > 0).sum()) >= 20
    before = x.clone()
    runs = {}
    for name in ASCENDING:
        w = runs[name] = Windows(x, tab, g, L, H, a, block, DT[dtype]).run(W.partitions()[name])
        assert torch.equal(bits(w.out), bits(want)), name  # (GUARD wherever nothing is emitted: nothing else of the destination is written)
        assert torch.equal(bits(w.red), bits(wred)) and torch.equal(w.lim, wlim), name
        assert not bool(w.bad), name
    assert torch.equal(bits(x), bits(before))
    # the final and one mid-way state against the host twin's
    windows = W.partitions()["random"]
    out = np.full(rows.shape, GUARD, dtype)
    red, lim = np.full(len(table), R.ONE), np.zeros(len(table), np.uint64)
    state, mid = None, len(windows) // 2
    for k, (first, frames) in enumerate(windows):
        state = RW.twin_window(rows, table, gain, L, H, a, block, first, frames, out, red, lim, state)
        if k in (mid, len(windows) - 1):
            assert np.array_equal(runs["random"].states[k].cpu().numpy().view(np.uint64), state.view(np.uint64)), k
    assert runs["random"].out.cpu().numpy().tobytes() == out.tobytes()


def test_the_lane_seam():
    """more than 256 pieces in a window -- several workgroups of 64 pieces a track -- and cuts at a workgroup's edge, one entry in
    front of it and one behind: two mono tracks at firsts 0 and 5"""
    row, L, H, block = 2 * 256 * 64 + 77, 7, 3, 64
    a = AB[0][0]
    gen = torch.Generator(device="cuda").manual_seed(12)
    rows = torch.randn((2, row, 1), generator=gen, device="cuda", dtype=torch.float64) * 0.5
    table = device_table(W.table_of([(0, row), (5, row - 5)]))
    want = torch.full(rows.shape, GUARD, dtype=torch.float64, device="cuda")
    _, wred, wlim = F.tracks_limit_release_device(rows, table, W.CEILING, a, lookahead=L, hold=H, block=block, out=want)
    plain = torch.full(rows.shape, GUARD, dtype=torch.float64, device="cuda")
    F.tracks_limit_device(rows, table, W.CEILING, lookahead=L, hold=H, out=plain)
    assert int((wlim > 0).sum()) == 2 and not torch.equal(bits(plain), bits(want))
    for cut in (None, 256 * 64 - 1, 256 * 64, 256 * 64 + 1):
        windows = [(0, row)] if cut is None else [(0, cut), (cut, row - cut)]
        w = Windows(rows, table, None, L, H, a, block, torch.float64).run(windows)
        assert torch.equal(bits(w.out), bits(want)), cut
        assert torch.equal(bits(w.red), bits(wred)) and torch.equal(w.lim, wlim), cut
        assert not bool(w.bad), cut


def test_the_launch_split():
    """32768 + 3 tracks of 64 mono frames in two windows with a mid-block cut: the smallest shape that crosses the grid.y split of
    every launch"""
    nt, row, L, H, block = 32768 + 3, 64, 7, 0, 64
    a = AB[0][0]
    gen = torch.Generator(device="cuda").manual_seed(9)
    rows = torch.randn((nt, row, 1), generator=gen, device="cuda") * 0.5
    table = np.zeros((nt, 6), np.uint64)
    table[:, 3] = np.arange(nt) % 5
    table[:, 4] = 64 - np.arange(nt) % 9
    table = device_table(table)
    want = torch.full(rows.shape, GUARD, dtype=torch.float32, device="cuda")
    _, wred, wlim = F.tracks_limit_release_device(rows, table, W.CEILING, a, lookahead=L, hold=H, block=block, out=want)
    w = Windows(rows, table, None, L, H, a, block, torch.float32).run([(0, 29), (29, 35)])
    assert torch.equal(bits(w.out), bits(want)) and torch.equal(bits(w.red), bits(wred)) and torch.equal(w.lim, wlim)
    assert not bool(w.bad)
    assert int((wlim[32768:] > 0).sum()) == 3 and int((wlim > 0).sum()) > 32000


def test_without_a_release_the_call_is_the_window_call(batches):
    rows, table, gain, x, tab, g = batches[2, np.float32]
    L, H = 72, 480
    back, ahead = F.limit_window_reach(L, H)
    junk = torch.full((x.shape[0], RW.STATE), GUARD, dtype=torch.float64, device="cuda")
    red = lim = rred = rlim = None
    for first, frames in W.partitions()["random-descending"]:
        b0, bn = W.coverage(first, frames, back, ahead)
        buf = x[:, b0:b0 + bn].contiguous()
        out, red, lim, _ = F.tracks_limit_release_window_device(buf, tab, W.ROW, b0, first, frames, W.CEILING, 0.0, state_in=junk, gain=g,
                                                               lookahead=L, hold=H, block=64, reduction=red, limited=lim)
        ref, rred, rlim = F.tracks_limit_window_device(buf, tab, W.ROW, b0, first, frames, W.CEILING, gain=g, lookahead=L, hold=H,
                                                       reduction=rred, limited=rlim, out=torch.full_like(out, GUARD))
        for t, (of, n) in enumerate(W.clamped(table, W.ROW)):
            lo, hi = max(of, first), min(of + n, first + frames)
            if hi > lo:
                assert torch.equal(bits(out[t, lo - first:hi - first]), bits(ref[t, lo - first:hi - first]))
    assert torch.equal(bits(red), bits(rred)) and torch.equal(lim, rlim) and int((lim > 0).sum()) >= 20


def test_the_python_wrapper(batches):
    """the wrapper allocates what it is not given, hands the state on, and refuses what the C call would"""
    rows, table, gain, x, tab, g = batches[2, np.float32]
    L, H = 7, 3
    a, block = AB[1]
    back, ahead = F.limit_window_reach(L, H)
    want = torch.full(x.shape, GUARD, dtype=torch.float32, device="cuda")
    _, wred, wlim = F.tracks_limit_release_device(x, tab, W.CEILING, a, gain=g, lookahead=L, hold=H, block=block, out=want)
    red = lim = state = None
    for first, frames in ((0, 4000), (4000, 5000)):
        b0, bn = W.coverage(first, frames, back, ahead)
        buf = x[:, b0:b0 + bn].contiguous()
        out, red, lim, state = F.tracks_limit_release_window_device(buf, tab, W.ROW, b0, first, frames, W.CEILING, a, state_in=state, gain=g,
                                                                   lookahead=L, hold=H, block=block, reduction=red, limited=lim)
        assert tuple(out.shape) == (x.shape[0], frames, 2) and out.dtype == torch.float32
        assert tuple(state.shape) == (x.shape[0], RW.STATE) and state.dtype == torch.float64
        for t, (of, n) in enumerate(W.clamped(table, W.ROW)):
            lo, hi = max(of, first), min(of + n, first + frames)
            if hi > lo:
                assert torch.equal(bits(out[t, lo - first:hi - first]), bits(want[t, lo:hi]))
    assert torch.equal(bits(red), bits(wred)) and torch.equal(lim, wlim)
    buf = x[:, 4000 - back:].contiguous()
    with pytest.raises(ValueError):  # only a window at frame 0 starts without a state
        F.tracks_limit_release_window_device(buf, tab, W.ROW, 4000 - back, 4000, 5000, W.CEILING, a, lookahead=L, hold=H, block=block)
    with pytest.raises(ValueError):  # the two states share memory
        F.tracks_limit_release_window_device(buf, tab, W.ROW, 4000 - back, 4000, 5000, W.CEILING, a, state_in=state, state_out=state,
                                             lookahead=L, hold=H, block=block)
    with pytest.raises(TypeError):
        F.tracks_limit_release_window_device(buf, tab, W.ROW, 4000 - back, 4000, 5000, W.CEILING, a, state_in=state[:, :7].contiguous(),
                                             lookahead=L, hold=H, block=block)
    with pytest.raises(ValueError):  # the coverage rule is the window call's
        F.tracks_limit_release_window_device(x[:, :100 + ahead - 1].contiguous(), tab, W.ROW, 0, 0, 100, W.CEILING, a, lookahead=L, hold=H)


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


SHAPED = dict(album=[0, 1, 1], shaping="wannamaker3", segment=4096, dither=True, seed=5)


@pytest.mark.parametrize("window,block,kw", [(w, b, dict()) for b in (64, 1024) for w in (None, 4096, 300)] + [(300, 64, SHAPED)],
                         ids=["%s-block%d" % (w, b) for b in (64, 1024) for w in ("whole-window", 4096, 300)] + ["300-block64-album-shaped"])
def test_streamed_limited_conversion_with_a_release_equals_the_whole_row_method(conversion, window, block, kw):
    r, tracks, whole_rows = conversion
    want = whole_rows(release_ms=50.0, release_block=block, **kw)
    plain = whole_rows(**kw)
    assert int((want[6] > 0).sum()) >= 1  # the limiter has lowered frames ...
    assert any(not torch.equal(a, b) for a, b in zip(want[0], plain[0]))  # ... and the release has changed what they became
    r.reset()
    got = r.convert_tracks_to_pcm_streamed_loudness_limited(tracks, F.RRX_FMT_S16, window=window, release_ms=50.0, release_block=block, **kw)
    same_returns(got, want)
