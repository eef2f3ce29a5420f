"""The limiter by windows, host side (RRX_limit_window_reach / RRX_tracks_limit_window_work_doubles / RRX_tracks_limit_window_device /
RRX_debug_tracks_limit_window_host): the symbols and the header's text, the refusals that need no device, and the host twin -- a
serial loop per track over the very functions the kernels call -- over window partitions of ragged rows against the one-stream
call on every slice and against limit_model.py, bit for bit.  CPU only."""
import os

import numpy as np
import pytest

import foo_dsp_resampler_amd as F
import limit_model as M
import limit_window_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RR_OK, RR_INVPARAM = 0, 6
GUARD = W.GUARD
NAMES = ("RRX_limit_window_reach", "RRX_tracks_limit_window_work_doubles", "RRX_tracks_limit_window_device",
         "RRX_debug_tracks_limit_window_host")


def test_symbols_are_exported_listed_and_declared():
    header = open(os.path.join(ROOT, "include", "ratelib_amd.h")).read()
    for name in NAMES:
        assert name in F.EXPECTED_SYMBOLS and name in F.available_symbols()
        assert name + "(" in header
    for name in ("limit_window_reach", "tracks_limit_window_work_doubles", "tracks_limit_window_device"):
        assert callable(getattr(F, name)) and name in F.__all__
    assert hasattr(F.Resampler, "convert_tracks_to_pcm_streamed_loudness_limited")
    assert "back  = (L - 1) + H + D,   ahead = (L - 1) + D" in header and "in ANY order" in header
    assert "buf_first <= max(0, win_first - back)" in header and "reads as +0.0" in header


def test_reach_and_work_doubles():
    for (L, H), want in zip(W.LH, W.REACH):
        assert F.limit_window_reach(L, H) == want
    import ctypes as C
    b, a = C.c_size_t(7), C.c_size_t(7)
    reach = F.lib().RRX_limit_window_reach
    assert reach(1, 1, 0, C.byref(b), C.byref(a)) == RR_OK and (b.value, a.value) == (0, 0)
    assert reach(16, 1024, 4096, C.byref(b), C.byref(a)) == RR_OK and (b.value, a.value) == (1023 + 4096 + 15, 1023 + 15)
    for bad in ((0, 1, 0), (17, 1, 0), (12, 0, 0), (12, 1025, 0), (12, 1, 4097)):
        assert reach(*bad, C.byref(b), C.byref(a)) == RR_INVPARAM, bad
    assert reach(12, 1, 0, None, C.byref(a)) == RR_INVPARAM and reach(12, 1, 0, C.byref(b), None) == RR_INVPARAM
    w = F.lib().RRX_tracks_limit_window_work_doubles
    assert w(3, 1000, 12, 64, 5) == 3 * 2 * (1000 + 128 + 5 + 24) == F.tracks_limit_window_work_doubles(3, 1000, hold=5)
    assert w(1, 0, 1, 1, 0) == 2 * 4
    # room for r (win + 2 L - 2 + H + D entries) and m (win + L - 1)
    for (L, H) in W.LH:
        assert w(1, 10, 12, L, H) // 2 >= max(10 + 2 * L - 2 + H + 11, 10 + L - 1)
    for bad in ((0, 10, 12, 64, 0), (-1, 10, 12, 64, 0), (1, 10, 0, 64, 0), (1, 10, 17, 64, 0), (1, 10, 12, 0, 0), (1, 10, 12, 1025, 0),
                (1, 10, 12, 64, 4097)):
        assert w(*bad) == 0, bad
    # the product reaches 2^60 or not: 2 * (win + 128 + 0 + 24)
    assert w(1, 2 ** 59 - 152, 12, 64, 0) == 0 and w(1, 2 ** 59 - 153, 12, 64, 0) == 2 ** 60 - 2
    assert w(2 ** 31 - 1, 2 ** 29, 12, 64, 0) == 0 and w(1, 2 ** 64 - 1, 12, 64, 0) == 0 and w(3, 2 ** 63, 16, 1024, 4096) == 0


def test_refusals_need_no_device_and_leave_everything_alone():
    nt, nch, row, L, H = 2, 2, 400, 7, 3
    back, ahead = F.limit_window_reach(L, H)
    table = W.table_of([(0, 400), (10, 100)])
    first, frames = 100, 50
    b0, bn = W.coverage(first, frames, back, ahead, row)
    mem = np.ones((nt * (bn + 4) * nch + nt * (frames + 4) * nch,), np.float32)  # the buffer, then the destination: one allocation
    buf, dst = mem[:nt * (bn + 4) * nch], mem[nt * (bn + 4) * nch:]
    dst[:] = GUARD
    red, lim = np.full(nt, 5, np.uint64), np.full(nt, 6, np.uint64)
    need = F.tracks_limit_window_work_doubles(nt, frames, 12, L, H)
    work = np.full(need, GUARD)
    fn = F.lib().RRX_debug_tracks_limit_window_host

    def call(**kw):
        co = kw.get("coefs", W.BS)
        return fn(kw.get("table", table.ctypes.data), kw.get("nt", nt), kw.get("nch", nch), kw.get("sf", 0), kw.get("buf", buf.ctypes.data),
                  kw.get("bs", bn + 4), kw.get("b0", b0), kw.get("bn", bn), kw.get("row", row), kw.get("first", first), kw.get("frames", frames),
                  kw.get("df", 0), kw.get("dst", dst.ctypes.data), kw.get("ds", frames + 4), None, kw.get("c", 0.5),
                  None if co is None else co.ctypes.data, kw.get("phases", 4), kw.get("taps", 12), kw.get("L", L), kw.get("H", H),
                  red.ctypes.data, lim.ctypes.data, kw.get("work", work.ctypes.data), kw.get("wd", need))

    inf = W.BS.copy()
    inf[17] = -np.inf
    refused = [dict(table=None), dict(buf=None), dict(dst=None), dict(nt=0), dict(nch=0), dict(sf=16), dict(df=16), dict(coefs=None),
               dict(phases=9), dict(taps=17), dict(coefs=inf), dict(row=2 ** 59), dict(c=0.0), dict(c=np.nan), dict(L=0), dict(L=1025),
               dict(H=4097), dict(work=None), dict(wd=need - 1),
               # the three window refusals of the siblings
               dict(first=2 ** 64 - 10, frames=20), dict(first=380, frames=21), dict(ds=frames - 1),
               # the coverage rule: one frame short at either end, past the rows, wrapping, a pitch below the frames
               dict(b0=b0 + 1, bn=bn - 1), dict(bn=bn - 1), dict(b0=0, bn=row + 1, bs=row + 1), dict(b0=2 ** 64 - 1, bn=2),
               dict(bs=bn - 1), dict(L=8, wd=need + 4 * nt), dict(H=4, wd=need + 2 * nt),
               # any overlap of the two extents, in place included
               dict(dst=buf.ctypes.data), dict(dst=buf.ctypes.data + 4), dict(dst=buf.ctypes.data + buf.nbytes - 4),
               dict(dst=buf.ctypes.data - 4), dict(dst=buf.ctypes.data - nt * (frames + 4) * nch * 8 + 8, df=1)]
    for kw in refused:
        assert call(**kw) == RR_INVPARAM, kw
        assert np.all(dst == GUARD) and np.all(red == 5) and np.all(lim == 6) and np.all(work == GUARD) and np.all(buf == 1), kw
    for kw in (dict(frames=0), dict(row=0, first=0, frames=0, b0=0, bn=0)):  # nothing to do: nothing is touched
        assert call(**kw) == RR_OK, kw
        assert np.all(dst == GUARD) and np.all(red == 5) and np.all(lim == 6) and np.all(work == GUARD)
    # a window at the head or the tail of the rows needs no halo beyond them
    assert call(first=0, frames=50, b0=0, bn=50 + ahead) == RR_OK
    assert call(first=350, frames=50, b0=350 - back, bn=50 + back) == RR_OK
    whole = np.ones(nt * row * nch, np.float32)
    assert call(b0=0, bn=row, bs=row, buf=whole.ctypes.data) == RR_OK  # more than the halo is fine
    assert call() == RR_OK and np.all(lim > 6) and np.all(red == 5)  # the ones are over the ceiling; a reduction below what is found stays
    assert np.all(dst.reshape(nt, frames + 4, nch)[:, frames:] == GUARD) and np.all(buf == 1)
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r)\nimport foo_dsp_resampler_amd as F\n"
            "print(F.lib().RRX_debug_tracks_limit_window_host(None, 1, 1, 0, None, 0, 0, 0, 0, 0, 0, 0, None, 0, None, 1.0, None, 4, 12, 1, 0, "
            "None, None, None, 0))\n" % ROOT)
    env = {k: v for k, v in os.environ.items() if k != "RSMP_TEST_HOOKS"}
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-1] == "-1"


def test_python_wrapper_checks_on_the_host():
    class Fake:  # stands in for a device tensor: the wrapper must refuse before any C call
        def __init__(self, shape, dtype="torch.float32", contiguous=True, cuda=True):
            self.shape, self.dtype, self._c, self.is_cuda = shape, dtype, contiguous, cuda

        def dim(self):
            return len(self.shape)

        def is_contiguous(self):
            return self._c

    with pytest.raises(TypeError):
        F.tracks_limit_window_device(Fake((2, 100, 2), "torch.int16"), None, 100, 0, 0, 10, 0.5)
    with pytest.raises(TypeError):
        F.tracks_limit_window_device(Fake((2, 100, 2), contiguous=False), None, 100, 0, 0, 10, 0.5)
    with pytest.raises(TypeError):
        F.tracks_limit_window_device(Fake((100, 2)), None, 100, 0, 0, 10, 0.5)
    with pytest.raises(ValueError):
        F.tracks_limit_window_device(Fake((2, 100, 2)), None, 100, 0, 95, 10, 0.5)  # the window leaves the rows
    with pytest.raises(ValueError):
        F.limit_window_reach(0, 0)
    with pytest.raises(ValueError):
        F.limit_window_reach(1, 4097)


FORMATS = {1: (np.float32, np.float64), 2: (np.float64, np.float64), 17: (np.float32, np.float32)}


@pytest.fixture(scope="module")
def batches():
    return {nch: W.batch(nch, FORMATS[nch][0]) for nch in FORMATS}


@pytest.mark.parametrize("L,H", W.LH)
@pytest.mark.parametrize("nch", sorted(FORMATS))
def test_twin_over_window_partitions_equals_the_one_stream_call(batches, nch, L, H):
    rows, table, gain = batches[nch]
    dst = FORMATS[nch][1]
    want, wred, wlim = W.expected(rows, table, gain, L, H, dst)
    assert int((wlim > 0).sum()) >= 20 and int((wred < M.ONE).sum()) >= 20  # the limiter has work to do
    for t, (of, n) in enumerate(W.clamped(table, W.ROW)):  # the numpy restatement says the same, on a few slices
        if n and t % 7 == 0:
            y, _, red, lim = M.limit(rows[t:t + 1, of:of + n], M.BS1770, W.CEILING, L, H, gain[t:t + 1], dst)
            assert M.same_samples(want[t:t + 1, of:of + n], y) and red[0] == wred[t] and lim[0] == wlim[t]
    before = rows.copy()
    for name, windows in W.partitions().items():
        out = np.full(rows.shape, GUARD, dst)
        red, lim = np.full(len(table), M.ONE), np.zeros(len(table), np.uint64)
        for first, frames in windows:
            W.twin_window(rows, table, gain, L, H, first, frames, out, red, lim)
        assert M.same_samples(out, want), name
        assert np.array_equal(red, wred) and np.array_equal(lim, wlim), name
    assert np.array_equal(rows, before)


def test_the_reach_is_needed_not_only_sufficient():
    """a single sample of 4.0 in silence under a filter whose every tap lifts it over the ceiling: the gain is below 1.0 exactly on
    [p - ahead, p + back]"""
    coefs = np.full((4, 12), 0.25)
    p, row = 6000, 12000
    for (L, H), (back, ahead) in zip(W.LH, W.REACH):
        rows = np.zeros((1, row, 1))
        rows[0, p, 0] = 4.0
        table = W.table_of([(0, row)])
        _, s, _, _ = M.limit(rows, coefs, 0.5, L, H)
        low = np.flatnonzero(s[0] < 1.0)
        assert low[0] == p - ahead and low[-1] == p + back and len(low) == back + ahead + 1
        for frame, count in ((p - ahead, 1), (p + back, 1), (p - ahead - 1, 0), (p + back + 1, 0)):
            out = np.full(rows.shape, GUARD)
            red, lim = np.full(1, M.ONE), np.zeros(1, np.uint64)
            W.twin_window(rows, table, None, L, H, frame, 1, out, red, lim, coefs=coefs)
            assert lim[0] == count and (red[0] < M.ONE) == bool(count), (L, H, frame)


def test_non_finite_samples_behave_as_in_the_whole_row_call():
    rng = np.random.default_rng(3)
    rows = (rng.standard_normal((3, 3000, 2)) * 0.5).astype(np.float32)
    rows[0, 700, 1] = np.nan
    rows[1, 1500, 0] = np.inf
    rows[1, 2999, 1] = -np.inf
    rows[2, 0, 0] = np.nan
    rows[2, 1024, 1] = np.inf
    table = W.table_of([(0, 3000), (100, 2900), (0, 2000)])
    gain = np.array([1.0, 0.75, 1.5])
    for L, H in ((7, 3), (72, 480)):
        want, wred, wlim = W.expected(rows, table, gain, L, H, np.float64)
        for windows in (W.partitions(3000)["k1024"], W.partitions(3000)["random-descending"]):
            out = np.full(rows.shape, GUARD)
            red, lim = np.full(3, M.ONE), np.zeros(3, np.uint64)
            for first, frames in windows:
                W.twin_window(rows, table, gain, L, H, first, frames, out, red, lim)
            assert M.same_samples(out, want) and np.isnan(out).any()
            assert np.array_equal(red, wred) and np.array_equal(lim, wlim)


def test_a_wrong_table_stays_inside_the_buffers():
    rng = np.random.default_rng(4)
    row, nch, L, H = 2000, 2, 7, 3
    big = 2 ** 64 - 1
    table = np.array([(0, 0, 0, big, big, 0), (0, 0, 0, 0, big, 0), (0, 0, 0, 1999, 2 ** 63, 0), (0, 0, 0, 2 ** 63, 5, 0),
                      (0, 0, 0, 500, big - 400, 0), (0, 0, 0, 2001, 1, 0)], np.uint64)
    rows = (rng.standard_normal((len(table), row, nch)) * 0.5).astype(np.float32)
    want, wred, wlim = W.expected(rows, table, None, L, H, np.float32)  # (the clamped slices)
    for windows in (W.partitions(row)["random"], [(0, row)], [(1999, 1), (0, 1999)]):
        out = np.full(rows.shape, GUARD, np.float32)
        red, lim = np.full(len(table), M.ONE), np.zeros(len(table), np.uint64)
        for first, frames in windows:
            W.twin_window(rows, table, None, L, H, first, frames, out, red, lim, pad=0)  # exactly sized, guards checked there
        assert M.same_samples(out, want) and np.array_equal(red, wred) and np.array_equal(lim, wlim)
