"""The limiter's release by windows, host side (RRX_tracks_limit_release_window_work_doubles / RRX_tracks_limit_release_window_device
/ RRX_debug_tracks_limit_release_window_host): the symbols and the header's text, the refusals that need no device, and the host
twin -- serial loops over the very functions the kernels call -- over ascending window partitions of ragged rows against the
one-stream release call on every slice, bit for bit, with the state after every window against limit_release_window_model.py.
CPU only."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

import foo_dsp_resampler_amd as F
import limit_release_model as R
import limit_release_window_model as RW
import limit_window_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RR_OK, RR_EXTUNINIT, RR_INVPARAM = 0, 5, 6
GUARD = W.GUARD
NAMES = ("RRX_tracks_limit_release_window_work_doubles", "RRX_tracks_limit_release_window_device",
         "RRX_debug_tracks_limit_release_window_host")
AB = [(R.coef(50, 44100), 64), (R.coef(200, 96000), 65), (R.coef(1000, 192000), 1024)]
ASCENDING = ("one", "k1024", "widths", "random")
FORMATS = {1: np.float32, 2: np.float64}  # source and destination alike


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def test_symbols_are_exported_listed_and_declared():
    header = open(os.path.join(ROOT, "include", "ratelib_amd.h")).read()
    for name in NAMES:
        assert name in F.EXPECTED_SYMBOLS and name in F.available_symbols()
        assert name + "(" in header
    assert "#define RRX_LIMIT_RELEASE_WIN_STATE 8" in header and F.RRX_LIMIT_RELEASE_WIN_STATE == 8 == RW.STATE
    for name in ("tracks_limit_release_window_work_doubles", "tracks_limit_release_window_device", "RRX_LIMIT_RELEASE_WIN_STATE"):
        assert hasattr(F, name) and name in F.__all__
    # the layout of the state, the snapshot rule and the order rule are stated
    assert "[0]    = S, the carry's S_i (1.0 at e = 0)" in header
    assert "[1..3] = C, A, B, the summary of the entries [i*block, e)" in header
    assert "[4]    = p, q[e - 1] run from S_i; S when r == 0" in header
    assert "[5..7] = +0.0" in header
    assert "the piece is never split at e1" in header
    assert "leave the bits of ONE RRX_tracks_limit_release_device call, for any cut positions" in header
    assert "4 * ((win_frames + lookahead - 1) / block + 2)" in header
    makefile = open(os.path.join(ROOT, "foo_dsp_resampler_amd", "csrc", "Makefile")).read()
    assert "limit_release_window.hip" in makefile and "FP_limit_release_window := -ffp-contract=off" in makefile
    sig = inspect.signature(F.Resampler.convert_tracks_to_pcm_streamed_loudness_limited)
    assert list(sig.parameters)[-2:] == ["release_ms", "release_block"]
    assert sig.parameters["release_ms"].default is None and sig.parameters["release_block"].default == 1024
    sig = inspect.signature(F.tracks_limit_release_window_device)
    assert list(sig.parameters) == ["buf", "table", "row_frames", "buf_first", "win_first", "win_frames", "ceiling", "release", "state_in", "gain",
                                    "lookahead", "hold", "block", "filter", "out", "reduction", "limited", "state_out", "buf_frames", "stream"]


def test_work_doubles():
    w = F.lib().RRX_tracks_limit_release_window_work_doubles
    assert w(3, 1000, 12, 64, 5, 1024) == 3 * (2 * (1000 + 128 + 5 + 24) + 4 * (1 + 2)) == F.tracks_limit_release_window_work_doubles(3, 1000, hold=5)
    assert w(1, 0, 1, 1, 0, 64) == 2 * 4 + 4 * 2 and w(1, 1, 12, 64, 0, 64) == 2 * 153 + 4 * 3 and w(1, 2, 12, 64, 0, 64) == 2 * 154 + 4 * 3
    for args in ((2, 100, 12, 64, 7, 65), (5, 4096, 12, 72, 480, 1024), (1, 9000, 12, 1024, 4096, 64), (7, 300, 16, 1, 0, 65536)):
        assert w(*args) == RW.work_doubles(*args) == F.tracks_limit_release_window_work_doubles(*args) > 0
        assert w(*args) > F.tracks_limit_window_work_doubles(*args[:5])  # the window call's share and the pieces' summaries
    for bad in ((0, 10, 12, 64, 0, 64), (-1, 10, 12, 64, 0, 64), (1, 10, 0, 64, 0, 64), (1, 10, 17, 64, 0, 64), (1, 10, 12, 0, 0, 64),
                (1, 10, 12, 1025, 0, 64), (1, 10, 12, 64, 4097, 64), (1, 10, 12, 64, 0, 63), (1, 10, 12, 64, 0, 65537), (1, 10, 12, 64, 0, 0)):
        assert w(*bad) == 0, bad
    # the total reaches 2^60 or not: the first frame count at which it does, by bisection on the formula
    for nt, block in ((1, 65536), (1, 64), (3, 1000)):
        lo, hi = 0, 2 ** 60
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if RW.work_doubles(nt, mid, 12, 64, 0, block) == 0 else (mid, hi)
        assert w(nt, lo, 12, 64, 0, block) == RW.work_doubles(nt, lo, 12, 64, 0, block) > 0 and w(nt, hi, 12, 64, 0, block) == 0
    assert w(2 ** 31 - 1, 2 ** 29, 12, 64, 0, 1024) == 0 and w(1, 2 ** 64 - 1, 12, 64, 0, 1024) == 0 and w(3, 2 ** 63, 16, 1024, 4096, 64) == 0


@pytest.fixture(scope="module")
def batches():
    return {nch: W.batch(nch, FORMATS[nch]) for nch in FORMATS}


@pytest.mark.parametrize("ab", range(len(AB)))
@pytest.mark.parametrize("L,H", W.LH)
@pytest.mark.parametrize("nch", sorted(FORMATS))
def test_twin_over_ascending_windows_equals_the_one_stream_release(batches, nch, L, H, ab):
    rows, table, gain = batches[nch]
    a, block = AB[ab]
    dst = FORMATS[nch]
    want, wred, wlim = RW.expected(rows, table, gain, L, H, a, block, dst)
    plain, _, _ = W.expected(rows, table, gain, L, H, dst)
    assert int((wlim > 0).sum()) >= 20 and not R.same_samples(want, plain)  # the limiter has work to do, and so has the release
    scan = RW.scans(rows, table, gain, L, H, a, block)
    before = rows.copy()
    parts = W.partitions()
    for name in ASCENDING:
        out = np.full(rows.shape, GUARD, dst)
        red, lim = np.full(len(table), R.ONE), np.zeros(len(table), np.uint64)
        state = None
        for first, frames in parts[name]:
            state = RW.twin_window(rows, table, gain, L, H, a, block, first, frames, out, red, lim, state)
            model = RW.states_after(scan, table, W.ROW, first + frames)
            assert np.array_equal(bits(state), bits(model)), (name, first, frames, np.argwhere(bits(state) != bits(model))[:4])
        assert R.same_samples(out, want), name
        assert np.array_equal(red, wred) and np.array_equal(lim, wlim), name
    assert np.array_equal(rows, before)


def test_the_cuts_cover_what_the_issue_asks_for():
    """block boundaries, mid-block, several windows inside one block, inside the last L - 1 entries of a slice; begun, not begun,
    ended tracks after a window; 157 blocks of 64 entries"""
    slices = W.clamped(W.batch(1, np.float32)[1], W.ROW)
    cuts = {name: [f for f, _ in W.partitions()[name][1:]] for name in ASCENDING}
    rel = {(c - of) for c in cuts["k1024"] + cuts["widths"] + cuts["random"] for of, n in slices if of < c < of + n}
    assert any(e % 64 == 0 for e in rel) and any(e % 64 for e in rel) and any(e % 1024 == 0 for e in rel)
    assert cuts["widths"][:3] == [1, 3, 14]
    assert any(max(of, of + n - 1023) < c < of + n for c in cuts["k1024"] for of, n in slices)  # fewer than L - 1 frames behind the cut
    c = cuts["k1024"][0]
    assert any(of >= c for of, n in slices) and any(n and of + n <= c for of, n in slices) and any(of < c < of + n for of, n in slices)
    assert -(-(W.ROW + 1024 - 1) // 64) == 157


def test_without_a_release_any_order_and_any_state_give_the_window_call():
    rows, table, gain = W.batch(2, np.float32, seed=6)
    L, H = 72, 480
    for name in ("k1024-descending", "random-descending", "widths-descending"):
        out, ref = np.full(rows.shape, GUARD, np.float32), np.full(rows.shape, GUARD, np.float32)
        red, lim = np.full(len(table), R.ONE), np.zeros(len(table), np.uint64)
        rred, rlim = red.copy(), lim.copy()
        junk = np.full((len(table), RW.STATE), GUARD)
        for first, frames in W.partitions()[name]:
            RW.twin_window(rows, table, gain, L, H, 0.0, 64, first, frames, out, red, lim, junk)
            W.twin_window(rows, table, gain, L, H, first, frames, ref, rred, rlim)
        assert out.tobytes() == ref.tobytes() and np.array_equal(red, rred) and np.array_equal(lim, rlim), name
        assert int((lim > 0).sum()) >= 20


def test_a_wrong_order_changes_samples_and_stays_inside_the_buffers():
    rows, table, gain = W.batch(1, np.float64, seed=7)
    L, H = 7, 3
    a, block = AB[0]
    want, _, _ = RW.expected(rows, table, gain, L, H, a, block, np.float64)
    out = np.full(rows.shape, GUARD)
    red, lim = np.full(len(table), R.ONE), np.zeros(len(table), np.uint64)
    state = np.zeros((len(table), RW.STATE))
    for first, frames in W.partitions()["k1024-descending"]:  # (the fences and the guards are twin_window's to check)
        state = RW.twin_window(rows, table, gain, L, H, a, block, first, frames, out, red, lim, state)
    assert not R.same_samples(out, want)
    assert np.all(np.isfinite(out)) and np.all((out == GUARD) == (want == GUARD))
    # a state of nonsense: other numbers, the same footprint
    out2 = np.full(rows.shape, GUARD)
    for first, frames in W.partitions()["random"]:
        RW.twin_window(rows, table, gain, L, H, a, block, first, frames, out2, red, lim, np.full((len(table), RW.STATE), -GUARD), pad=0)
    assert not R.same_samples(out2, want) and np.all((out2 == GUARD) == (want == GUARD))
    # no outgoing state asked for: the samples of the first window are the same
    out3 = np.full(rows.shape, GUARD)
    RW.twin_window(rows, table, gain, L, H, a, block, 0, 1024, out3, red, lim, None, state_out=False)
    assert R.same_samples(out3[:, :1024], np.where(out3[:, :1024] == GUARD, GUARD, want[:, :1024]))


def test_a_wrong_table_stays_inside_the_buffers():
    rng = np.random.default_rng(4)
    row, nch, L, H = 2000, 2, 7, 3
    a, block = AB[1]
    big = 2 ** 64 - 1
    table = np.array([(0, 0, 0, big, big, 0), (0, 0, 0, 0, big, 0), (0, 0, 0, 1999, 2 ** 63, 0), (0, 0, 0, 2 ** 63, 5, 0),
                      (0, 0, 0, 500, big - 400, 0), (0, 0, 0, 2001, 1, 0)], np.uint64)
    rows = (rng.standard_normal((len(table), row, nch)) * 0.5).astype(np.float32)
    want, wred, wlim = RW.expected(rows, table, None, L, H, a, block, np.float32)  # (the clamped slices)
    for windows in (W.partitions(row)["random"], [(0, row)], [(0, 1999), (1999, 1)]):
        out = np.full(rows.shape, GUARD, np.float32)
        red, lim = np.full(len(table), R.ONE), np.zeros(len(table), np.uint64)
        state = None
        for first, frames in windows:
            state = RW.twin_window(rows, table, None, L, H, a, block, first, frames, out, red, lim, state, pad=0)
        assert R.same_samples(out, want) and np.array_equal(red, wred) and np.array_equal(lim, wlim)


def test_host_twin_refuses_as_the_device_call_does_and_leaves_everything_alone():
    nt, nch, row, L, H = 2, 2, 400, 7, 3
    back, ahead = F.limit_window_reach(L, H)
    table = W.table_of([(0, 400), (10, 100)])
    first, frames = 100, 50
    b0, bn = W.coverage(first, frames, back, ahead, row)
    mem = np.ones((nt * (bn + 4) * nch + nt * (frames + 4) * nch,), np.float32)  # the buffer, then the destination: one allocation
    buf, dst = mem[:nt * (bn + 4) * nch], mem[nt * (bn + 4) * nch:]
    dst[:] = GUARD
    red, lim = np.full(nt, 5, np.uint64), np.full(nt, 6, np.uint64)
    need = F.tracks_limit_release_window_work_doubles(nt, frames, 12, L, H, 64)
    work = np.full(need, GUARD)
    states = np.full(3 * nt * RW.STATE, 0.25)  # the incoming state, then the outgoing one, then room to slide into
    sin, sout = states[:nt * RW.STATE], states[nt * RW.STATE:2 * nt * RW.STATE]
    fn = F.lib().RRX_debug_tracks_limit_release_window_host

    def call(**kw):
        return fn(kw.get("table", table.ctypes.data), kw.get("nt", nt), nch, kw.get("sf", 0), kw.get("buf", buf.ctypes.data), bn + 4,
                  kw.get("b0", b0), kw.get("bn", bn), kw.get("row", row), kw.get("first", first), kw.get("frames", frames), 0,
                  kw.get("dst", dst.ctypes.data), kw.get("ds", frames + 4), None, kw.get("c", 0.5), W.BS.ctypes.data, 4, 12, kw.get("L", L),
                  kw.get("H", H), kw.get("a", 0.99), kw.get("block", 64), kw.get("sin", sin.ctypes.data), kw.get("sout", sout.ctypes.data),
                  red.ctypes.data, lim.ctypes.data, kw.get("work", work.ctypes.data), kw.get("wd", need))

    refused = [dict(a=-0.1), dict(a=1.0), dict(a=1.5), dict(a=np.nan), dict(block=63), dict(block=65537), dict(wd=need - 1), dict(work=None),
               dict(wd=F.tracks_limit_window_work_doubles(nt, frames, 12, L, H)),
               # the two state rules
               dict(sin=None), dict(sout=sin.ctypes.data), dict(sout=sin.ctypes.data + 8), dict(sout=sin.ctypes.data + sin.nbytes - 8),
               dict(sin=sout.ctypes.data + 8), dict(sin=sout.ctypes.data + sout.nbytes - 8),
               # what the window call refuses
               dict(table=None), dict(buf=None), dict(dst=None), dict(nt=0), dict(sf=16), dict(c=0.0), dict(L=0), dict(H=4097),
               dict(first=380, frames=21), dict(ds=frames - 1), dict(b0=b0 + 1, bn=bn - 1), dict(bn=bn - 1), dict(dst=buf.ctypes.data)]
    for kw in refused:
        assert call(**kw) == RR_INVPARAM, kw
        assert np.all(dst == GUARD) and np.all(red == 5) and np.all(lim == 6) and np.all(work == GUARD) and np.all(buf == 1), kw
        assert np.all(states == 0.25), kw
    for kw in (dict(frames=0), dict(row=0, first=0, frames=0, b0=0, bn=0, sin=None)):  # nothing to do: nothing is touched, the state included
        assert call(**kw) == RR_OK, kw
        assert np.all(dst == GUARD) and np.all(red == 5) and np.all(lim == 6) and np.all(work == GUARD) and np.all(states == 0.25)
    assert call(sout=sin.ctypes.data + sin.nbytes) == RR_OK and call(sin=sout.ctypes.data + sout.nbytes) == RR_OK  # adjacent is apart
    assert call(sout=None) == RR_OK
    assert call(first=0, frames=50, b0=0, bn=50 + ahead, sin=None) == RR_OK  # a window at frame 0 needs no state
    states[:] = 0.25
    assert call() == RR_OK and np.all(lim > 6) and np.all(red == 5) and np.all(sin == 0.25)
    so = sout.reshape(nt, RW.STATE)
    # track 0 goes from entry 100 to 150, into block 2 of 64; track 1 from entry 90 to its last, 100, inside block 1: S stays
    assert np.all(so[:, 5:] == 0) and so[0, 0] != 0.25 and so[1, 0] == 0.25
    assert np.all(states[2 * nt * RW.STATE:] == 0.25)
    code = ("import sys; sys.path.insert(0, %r)\nimport foo_dsp_resampler_amd as F\n"
            "print(F.lib().RRX_debug_tracks_limit_release_window_host(None, 1, 1, 0, None, 0, 0, 0, 0, 0, 0, 0, None, 0, None, 1.0, None, 4, 12, 1, 0, "
            "0.5, 64, None, None, None, None, None, 0))\n" % ROOT)
    env = {k: v for k, v in os.environ.items() if k != "RSMP_TEST_HOOKS"}
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-1] == "-1"


CHILD = r"""
import sys, ctypes as C
sys.path.insert(0, %r)
import foo_dsp_resampler_amd as F
L = F.lib()
cb = F.ratelib._ALLOC_CB(lambda: None)
p = 1 << 24  # never dereferenced: every call below is answered from its arguments, or from the library's state, alone
q = p + (1 << 24)
w = p + (1 << 26)
s1 = p + (1 << 27)
s2 = s1 + 3 * 8 * 8
co = (C.c_double * 128)(*([0.25] * 128))
co_p = C.cast(co, C.c_void_p)
need = L.RRX_tracks_limit_release_window_work_doubles(3, 1024, 12, 64, 0, 1024)
good = dict(device=-1, stream=None, table=p, ntracks=3, nch=2, sf=0, buf=p, bs=1200, b0=926, bn=1172, row=4096, first=1000, frames=1024, df=0, dst=q,
            ds=1024, gain=None, c=0.9, coefs=co_p, phases=4, taps=12, L=64, H=0, a=0.999, block=1024, sin=s1, sout=s2, red=p, lim=p, work=w, wd=need)
def call(**kw):
    a = dict(good, **kw)
    return L.RRX_tracks_limit_release_window_device(a["device"], a["stream"], a["table"], a["ntracks"], a["nch"], a["sf"], a["buf"], a["bs"], a["b0"],
                                                    a["bn"], a["row"], a["first"], a["frames"], a["df"], a["dst"], a["ds"], a["gain"], a["c"],
                                                    a["coefs"], a["phases"], a["taps"], a["L"], a["H"], a["a"], a["block"], a["sin"], a["sout"],
                                                    a["red"], a["lim"], a["work"], a["wd"])
print("uninit", call())                                   # before init_ratelib
print("init", L.init_ratelib(cb))                         # no device: refuses
print("uninit", call(), call(frames=0, wd=L.RRX_tracks_limit_release_window_work_doubles(3, 0, 12, 64, 0, 1024)))
cases = [("a-0.1", dict(a=-0.1)), ("a1.0", dict(a=1.0)), ("a1.5", dict(a=1.5)), ("anan", dict(a=float("nan"))), ("ainf", dict(a=float("inf"))),
         ("block63", dict(block=63)), ("block65537", dict(block=65537)), ("block0", dict(block=0)), ("work", dict(work=None)),
         ("wd", dict(wd=need - 1)), ("wd-plain", dict(wd=L.RRX_tracks_limit_window_work_doubles(3, 1024, 12, 64, 0))), ("wd-for-block", dict(block=64)),
         ("state-null", dict(sin=None)), ("state-equal", dict(sout=s1)), ("state-overlap", dict(sout=s1 + 8)), ("state-overlap-end", dict(sout=s1 + 3 * 64 - 8)),
         ("state-overlap-front", dict(sin=s2 + 8)),
         ("c0", dict(c=0.0)), ("L0", dict(L=0)), ("L1025", dict(L=1025)), ("H4097", dict(H=4097)), ("coefs", dict(coefs=None)), ("dstfmt7", dict(df=7)),
         ("device-2", dict(device=-2)), ("inplace", dict(dst=p)), ("table", dict(table=None)), ("buf", dict(buf=None)), ("ntracks0", dict(ntracks=0)),
         ("coverage-front", dict(b0=927, bn=1171)), ("coverage-end", dict(bn=1171)), ("window", dict(first=4000)), ("ds", dict(ds=1023)),
         ("rows2^60", dict(row=2**58))]
for name, kw in cases:
    print("inv", name, call(**kw))
for name, kw in [("a0", dict(a=0.0)), ("block65536", dict(block=65536)), ("block1000", dict(block=1000)), ("no-state-out", dict(sout=None)),
                 ("state-adjacent", dict(sout=s1 + 3 * 64)), ("first-window", dict(first=0, b0=0, bn=1024 + 74, sin=None)),
                 ("double", dict(sf=1, df=1)), ("no-stats", dict(red=None, lim=None)), ("gain", dict(gain=p)), ("large-work", dict(wd=need + 1))]:
    print("ok", name, call(**kw))                         # nothing to refuse: answered RR_EXTUNINIT here
"""


def test_invalid_parameters_are_refused_without_a_device():
    out = subprocess.run([sys.executable, "-c", CHILD % ROOT], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))
    assert out.returncode == 0, out.stderr
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.split() and ln.split()[0] in ("uninit", "init", "inv", "ok")]
    assert ["init", "-1"] in lines
    uninit = [ln for ln in lines if ln[0] == "uninit"]
    assert len(uninit) == 2 and all(int(v) == RR_EXTUNINIT for ln in uninit for v in ln[1:])
    for kind, count, want in (("inv", 33, RR_INVPARAM), ("ok", 10, RR_EXTUNINIT)):
        got = [ln for ln in lines if ln[0] == kind]
        assert len(got) == count and all(int(ln[2]) == want for ln in got), got


def test_python_wrapper_checks_on_the_host():
    class Fake:  # stands in for a device tensor: the wrapper must refuse before any C call
        def __init__(self, shape, dtype="torch.float32", contiguous=True, cuda=True):
            self.shape, self.dtype, self._c, self.is_cuda = shape, dtype, contiguous, cuda

        def dim(self):
            return len(self.shape)

        def is_contiguous(self):
            return self._c

    for bad in (-0.1, 1.0, 1.5, float("nan")):  # _limit_release_params comes first
        with pytest.raises(ValueError):
            F.tracks_limit_release_window_device(Fake((2, 100, 2)), None, 100, 0, 0, 10, 0.5, bad)
    for bad in (63, 65537):
        with pytest.raises(ValueError):
            F.tracks_limit_release_window_device(Fake((2, 100, 2)), None, 100, 0, 0, 10, 0.5, 0.9, block=bad)
    with pytest.raises(TypeError):
        F.tracks_limit_release_window_device(Fake((2, 100, 2), "torch.int16"), None, 100, 0, 0, 10, 0.5, 0.9)
    with pytest.raises(TypeError):
        F.tracks_limit_release_window_device(Fake((2, 100, 2), contiguous=False), None, 100, 0, 0, 10, 0.5, 0.9)
    with pytest.raises(TypeError):
        F.tracks_limit_release_window_device(Fake((100, 2)), None, 100, 0, 0, 10, 0.5, 0.9)
    with pytest.raises(ValueError):
        F.tracks_limit_release_window_device(Fake((2, 100, 2)), None, 100, 0, 95, 10, 0.5, 0.9)  # the window leaves the rows
    assert F.tracks_limit_release_window_work_doubles(1, 10, block=63) == 0
