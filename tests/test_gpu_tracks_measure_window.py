"""True peak and loudness in the windowed track path on the device (RRX_tracks_true_peak_window_device,
RRX_tracks_loudness_window_device; DESIGN.md 11, "Windows with true peak and loudness"): the window calls against the whole-row
calls on the same rows and against the host twins, bit for bit, with guard doubles around states, energies and work; past the
grid.y split; on long rows with windows shorter than a hop; and the two streamed normalising conversions against the whole-row
methods in every element of their tuples."""
import functools

import numpy as np
import pytest

import foo_dsp_resampler_amd as F
import measure_window_cases as MW
import shaped_window_cases as W

pytestmark = pytest.mark.gpu
N = len(W.SLICES)


def u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def check(x, tab, part, filt, gains, hop, stride, what, stream=None, rows=None):
    """the device window calls == the whole-row device calls == the host twins, on one partition"""
    (tp, pk, tst), (energy, hops, lst) = MW.device_windows(x, tab, part, filt, gains, hop, stride, rows=rows, stream=stream)
    wtp, wpk, wenergy, whops = whole(x, tab, filt, gains, hop, stride, what)
    htp, hpk, htst = MW.tp_host_windows(x, tab, part, filt, gains, rows=rows)
    henergy, hhops, hlst = MW.ld_host_windows(x, tab, part, hop, gains, stride, rows=rows)
    assert np.array_equal(tp, wtp) and np.array_equal(pk, wpk), ("true peak against the whole-row call",) + what
    assert np.array_equal(tp, htp) and np.array_equal(pk, hpk), ("true peak against the host twin",) + what
    assert np.array_equal(u64(tst), u64(htst)), ("true-peak state",) + what
    assert np.array_equal(u64(energy), u64(wenergy)) and np.array_equal(hops, whops), ("energies against the whole-row call",) + what
    assert np.array_equal(u64(energy), u64(henergy)) and np.array_equal(hops, hhops), ("energies against the host twin",) + what
    assert np.array_equal(u64(lst), u64(hlst)), ("loudness state",) + what


_whole = {}


def whole(x, tab, filt, gains, hop, stride, what):
    """the whole-row device calls, once per case"""
    key = what[:-1]
    if key not in _whole:
        _whole.clear()
        _whole[key] = MW.device_whole(x, tab, filt, gains, hop, stride)
    return _whole[key]


# (filter, channels, float64, gains, hop): 8 channels is the LDS form with idle lanes, 257 the direct form
CASES = [("bs1770", 2, False, True, 64), ("8x16", 3, True, False, 7), ("1x1", 1, False, True, 333), ("2x2", 2, True, False, 1000),
         ("bs1770", 8, False, True, 100), ("bs1770", 257, False, False, 1), ("8x16", 257, True, True, 100)]


@pytest.mark.parametrize("name,nch,double,gain,hop", CASES, ids=["%s-%dch-%s-hop%d" % (c[0], c[1], "f64" if c[2] else "f32", c[4]) for c in CASES])
def test_window_calls_equal_the_whole_row_calls_and_the_host_twins(name, nch, double, gain, hop):
    assert F.lib().RRX_tracks_true_peak_window_device is not None
    x = MW.rows_of(N, nch, double)
    tab, _ = W.table_of()
    for pname, part in W.PARTITIONS.items():
        if nch == 257 and pname == "7":
            continue                                             # (a hundred windows of 257 channels add seconds and no path)
        # (hop 1000: no row holds a hop; one entry a channel, never written, so that the energies have a pointer)
        check(x, tab, part, MW.FILTERS[name], MW.GAINS if gain else None, hop, max(W.R // hop, 1), (name, nch, double, gain, hop, pname))


def test_energy_stride_smaller_than_the_hop_count_and_a_wrong_table():
    x = MW.rows_of(N, 2, False)
    tab, _ = W.table_of()
    check(x, tab, W.PARTITIONS["333"], MW.FILTERS["bs1770"], MW.GAINS, 64, 3, ("stride 3", "333"))
    wrong = tab.copy()
    wrong[-1] = (0, 0, 0, 650, 2 ** 40, 0)
    wrong[1] = (0, 0, 0, 2 ** 63, 130, 7)
    wrong[0] = (0, 0, 0, 2 ** 64 - 1, 2 ** 64 - 1, 0)
    check(x, wrong, W.PARTITIONS["on segment boundaries"], MW.FILTERS["bs1770"], MW.GAINS, 7, 100, ("wrong table", "cuts"))


def test_window_calls_on_a_side_stream():
    import torch
    x = MW.rows_of(N, 2, False)
    tab, _ = W.table_of()
    check(x, tab, W.PARTITIONS["333"], MW.FILTERS["bs1770"], MW.GAINS, 100, 7, ("side stream", "333"), stream=torch.cuda.Stream())


def test_past_the_grid_y_split():
    """32768 + 3 tracks of 24-frame stereo rows, hop 8, in two windows of 13 and 11 frames: the smallest shape that crosses the
    split of grid.y in both calls"""
    n = 32768 + 3
    x = (np.random.default_rng(9).standard_normal((n, 24, 2)) * 0.4).astype(np.float32)
    tab = np.zeros((n, 6), np.uint64)
    t = np.arange(n)
    tab[:, 3] = t % 3
    tab[:, 4] = 24 - t % 3 - t % 2
    gains = 0.5 + (t % 7) * 0.25
    check(x, tab, [(0, 13), (13, 11)], MW.FILTERS["bs1770"], gains, 8, 3, ("grid.y", "13 + 11"))


def test_long_rows_in_windows_shorter_than_a_hop():
    rows, hop, step = 40000, 4410, 4099
    x = MW.rows_of(3, 2, False, frames=rows)
    tab, _ = W.table_of([(5, 39990), (1000, 20000), (0, 40000)])
    check(x, tab, W.even(step, rows), MW.FILTERS["bs1770"], None, hop, rows // hop, ("long rows", step))


# ---------------------------------------------------------------------------------------------------------------- the methods
FS, FO, NSTREAMS = 44100, 48000, 4
LENGTHS = (300, 5000, 23000, 41000)                              # the first: under 400 ms of output, no block passes the gate
ALBUMS = [1, 0, 1, 0]


@functools.lru_cache(maxsize=None)
def method_tracks():
    import torch
    out = []
    for i, n in enumerate(LENGTHS):
        rng = np.random.default_rng(40 + i)
        t = np.arange(n) / FS
        x = np.stack([0.3 * np.sin(2 * np.pi * (220.0 + 60 * i + 17 * c) * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 1.5 * t)) for c in range(2)], axis=1)
        out.append(torch.from_numpy((x + 0.02 * rng.standard_normal((n, 2))).astype(np.float32)).cuda())
    return out


@functools.lru_cache(maxsize=None)
def whole_row(loudness, shaping, album):
    r = F.Resampler(FS, FO, nch=2, nstreams=NSTREAMS)
    kw = dict(shaping=shaping, segment=4096, dither=True, seed=W.SEED)
    if loudness:
        res = r.convert_tracks_to_pcm_loudness_normalized(method_tracks(), F.RRX_FMT_S16, album=ALBUMS if album else None, **kw)
    else:
        res = r.convert_tracks_to_pcm_normalized(method_tracks(), F.RRX_FMT_S16, **kw)
    r.close()
    return res


def same_tuple(got, want):
    import torch
    assert len(got) == len(want)
    for g, w in zip(got[0], want[0]):
        assert g.shape == w.shape and g.dtype == w.dtype and torch.equal(g, w), int((g != w).sum())
    for k in range(1, len(want)):
        g, w = got[k], want[k]
        assert g.shape == w.shape and g.dtype == w.dtype, k
        assert torch.equal(g.contiguous().view(torch.int64), w.contiguous().view(torch.int64)), (k, g, w)


@pytest.mark.parametrize("window", [None, 1000])
@pytest.mark.parametrize("shaping", [None, "wannamaker9"])
def test_streamed_normalized_equals_the_whole_row_method(window, shaping):
    import torch
    want = whole_row(False, shaping, False)
    r = F.Resampler(FS, FO, nch=2, nstreams=NSTREAMS)
    got = r.convert_tracks_to_pcm_streamed_normalized(method_tracks(), F.RRX_FMT_S16, window=window, shaping=shaping, segment=4096, dither=True,
                                                      seed=W.SEED)
    same_tuple(got, want)
    assert float(want[4].max()) > 0.2 and torch.isfinite(want[3]).all()
    r.close()


@pytest.mark.parametrize("window", [None, 1000])
@pytest.mark.parametrize("shaping", [None, "wannamaker9"])
@pytest.mark.parametrize("album", [False, True])
def test_streamed_loudness_normalized_equals_the_whole_row_method(window, shaping, album):
    import torch
    want = whole_row(True, shaping, album)
    r = F.Resampler(FS, FO, nch=2, nstreams=NSTREAMS)
    got = r.convert_tracks_to_pcm_streamed_loudness_normalized(method_tracks(), F.RRX_FMT_S16, window=window, shaping=shaping, segment=4096,
                                                               dither=True, seed=W.SEED, album=ALBUMS if album else None)
    same_tuple(got, want)
    lufs = want[5].cpu().numpy()
    if not album:
        assert np.isneginf(lufs[0]) and np.isneginf(lufs[1]) and np.isfinite(lufs[2:]).all()   # too short for a block: no loudness, gain 1
        assert float(want[3][0]) == 1.0
    else:
        assert np.isfinite(lufs).all() and lufs[0] == lufs[2] and lufs[1] == lufs[3]
    # the handle is usable afterwards
    r.reset()
    again = r.convert_tracks_to_pcm_streamed(method_tracks(), F.RRX_FMT_S16, window=window)
    r.close()
    r = F.Resampler(FS, FO, nch=2, nstreams=NSTREAMS)
    plain = r.convert_tracks_to_pcm_device(method_tracks(), F.RRX_FMT_S16)
    r.close()
    assert all(torch.equal(a, b) for a, b in zip(again[0], plain[0]))


def test_streamed_loudness_normalized_memory_is_that_of_the_streamed_form():
    """The existing streamed memory test's shape and method.  The rise of torch's peak allocation over the streamed
    loudness-normalised call is at most that of convert_tracks_to_pcm_streamed measured here, plus the states (one [nstreams, nch,
    16] per measurement), the hop energies and one window's work buffer, from their stated sizes: pass A holds two of each state
    but no destination, pass B is the streamed form beside the returned statistics."""
    import torch
    fs, fo, lengths, nstreams, window = 44100, 48000, (40, 65, 1500, 7000, 30000), 5, 4099
    rng = np.random.default_rng(3)
    tracks = [torch.from_numpy((0.3 * rng.standard_normal((n, 2))).astype(np.float32)).cuda() for n in lengths]
    plan = F.tracks_plan(fs, fo, lengths)
    hop, nch = fo // 10, 2
    win_out = -(-window * fo // fs)
    longest = max(int(e.out_first + e.out_frames) for e in plan.table)
    extra = 8 * (2 * nstreams * nch * 16 + nstreams * nch * -(-longest // hop) + nstreams * nch * (win_out // hop + 2) * 4)
    rise = []
    for normalised in (False, True):
        r = F.Resampler(fs, fo, nch=2, nstreams=nstreams)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        if normalised:
            res = r.convert_tracks_to_pcm_streamed_loudness_normalized(tracks, F.RRX_FMT_S16, window=window)
        else:
            res = r.convert_tracks_to_pcm_streamed(tracks, F.RRX_FMT_S16, window=window)
        torch.cuda.synchronize()
        rise.append(torch.cuda.max_memory_allocated() - before)
        del res
        r.close()
    print("streamed", rise[0], "streamed loudness-normalised", rise[1], "allowed on top", extra)
    assert rise[1] <= rise[0] + extra, (rise, extra)
