"""The limiter's host side (RRX_limit_device / RRX_tracks_limit_device / RRX_limit_work_doubles / RRX_debug_limit_host): the
symbols and the header's text, the refusals that need no device, the arithmetic -- the host twin is serial loops over the very
functions the kernels call -- against the numpy restatement in limit_model.py, bit for bit, and the properties of the limiter
that do not rest on that model.  CPU only."""
import os
import subprocess
import sys

import numpy as np
import pytest

import foo_dsp_resampler_amd as F
import limit_model as M
from test_loudness_api import gate_host
from test_loudness_api import host as loudness_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RR_OK, RR_EXTUNINIT, RR_INVPARAM = 0, 5, 6
SHAPES = [(1, 1, 1), (1, 2, 11), (1, 2, 12), (1, 2, 13), (3, 3, 4099), (2, 6, 1201)]  # (nstreams, nch, frames)
LH = [(1, 0), (2, 1), (64, 0), (72, 480), (1024, 4096)]
BS = np.ascontiguousarray(M.BS1770.reshape(-1))
GUARD = 777.25
NAMES = ("RRX_limit_work_doubles", "RRX_limit_device", "RRX_tracks_limit_device", "RRX_debug_limit_host")


def host(x, ceiling, L, H, coefs=M.BS1770, gain=None, dst=np.float64, stride=None, out=None, red=None, lim=None):
    """RRX_debug_limit_host on x [nstreams, frames, nch] (rows `stride` frames apart inside x's buffer when given): (rc, y, reduction
    bits, limited).  The work buffer is three doubles longer than needed, under guards."""
    ns, frames, nch = x.shape
    coefs = np.ascontiguousarray(coefs, dtype=np.float64)
    y = np.full((ns, frames, nch), GUARD, dtype=dst) if out is None else out
    red = np.full(ns, M.ONE) if red is None else red
    lim = np.zeros(ns, np.uint64) if lim is None else lim
    g = None if gain is None else np.ascontiguousarray(gain, dtype=np.float64)
    need = F.limit_work_doubles(ns, frames, coefs.shape[1], L)
    assert need == M.work_doubles(ns, frames, coefs.shape[1], L)
    work = np.full(need + 3, GUARD)
    rc = F.lib().RRX_debug_limit_host(int(x.dtype == np.float64), x.ctypes.data, frames if stride is None else stride, int(y.dtype == np.float64),
                                      y.ctypes.data, frames if stride is None or out is None else stride, ns, frames, nch,
                                      None if g is None else g.ctypes.data, float(ceiling), coefs.ctypes.data, coefs.shape[0], coefs.shape[1], L, H,
                                      red.ctypes.data, lim.ctypes.data, work.ctypes.data, need)
    assert np.all(work[need:] == GUARD)
    return rc, y, red, lim


def signal(rng, shape, dtype):
    ns, nch, frames = shape
    if frames >= 1000:
        return M.planted(rng, (ns, frames, nch), dtype)
    return (rng.standard_normal((ns, frames, nch)) * 0.5).astype(dtype)


def test_symbols_are_exported_listed_and_declared():
    header = open(os.path.join(ROOT, "include", "ratelib_amd.h")).read()
    for name in NAMES:
        assert name in F.EXPECTED_SYMBOLS and name in F.available_symbols()
        assert name + "(" in header
    assert "#define RRX_LIMIT_MAX_LOOKAHEAD 1024" in header and "#define RRX_LIMIT_MAX_HOLD      4096" in header
    assert (F.RRX_LIMIT_MAX_LOOKAHEAD, F.RRX_LIMIT_MAX_HOLD) == (1024, 4096) == (M.MAX_LOOKAHEAD, M.MAX_HOLD)
    for name in ("limit_device", "tracks_limit_device", "limit_work_doubles"):
        assert callable(getattr(F, name)) and name in F.__all__
    assert hasattr(F.Resampler, "convert_tracks_to_pcm_loudness_limited")
    # the arithmetic and its limits are stated
    assert "s[n]      = fmin(acc * invL, m[n])" in header and "m[k]      = min of r[F] over F in [k - H, k + L - 1 + D]" in header
    assert "|y| <= c * (1 + 2^-51)" in header and "NOT strictly bounded" in header
    assert "A NaN sample passes through as a NaN" in header
    makefile = open(os.path.join(ROOT, "foo_dsp_resampler_amd", "csrc", "Makefile")).read()
    assert "limit.hip" in makefile and "FP_limit         := -ffp-contract=off" in makefile


def test_work_doubles():
    w = F.lib().RRX_limit_work_doubles
    assert w(3, 1000, 12, 64) == 3 * 2 * (1000 + 12 + 64) == F.limit_work_doubles(3, 1000)
    assert w(1, 0, 1, 1) == 4
    for bad in ((0, 10, 12, 64), (-1, 10, 12, 64), (1, 10, 0, 64), (1, 10, 17, 64), (1, 10, 12, 0), (1, 10, 12, 1025)):
        assert w(*bad) == 0, bad
    assert w(1, 2 ** 59 - 76, 12, 64) == 0 and w(1, 2 ** 59 - 77, 12, 64) == 2 ** 60 - 2  # the product reaches 2^60 or not
    assert w(2 ** 31 - 1, 2 ** 29, 12, 64) == 0 and w(1, 2 ** 64 - 1, 12, 64) == 0 and w(3, 2 ** 63, 16, 1024) == 0


CHILD = r"""
import sys, ctypes as C
sys.path.insert(0, %r)
import foo_dsp_resampler_amd as F
L = F.lib()
cb = F.ratelib._ALLOC_CB(lambda: None)
p = 1 << 24  # never dereferenced: every call below is answered from its arguments, or from the library's state, alone
q = p + (1 << 24)
w = p + (1 << 26)
co = (C.c_double * 128)(*([0.25] * 128))
bad = (C.c_double * 48)(*([0.25] * 47 + [float("inf")]))
co_p = C.cast(co, C.c_void_p)
need = L.RRX_limit_work_doubles(2, 1024, 12, 64)
good = dict(device=-1, stream=None, sf=0, src=p, ss=4096, df=0, dst=q, ds=4096, nstreams=2, frames=1024, nch=2, gain=None, c=0.9, coefs=co_p, phases=4,
            taps=12, L=64, H=0, red=p, lim=p, work=w, wd=need)
def call(**kw):
    a = dict(good, **kw)
    return L.RRX_limit_device(a["device"], a["stream"], a["sf"], a["src"], a["ss"], a["df"], a["dst"], a["ds"], a["nstreams"], a["frames"], a["nch"],
                              a["gain"], a["c"], a["coefs"], a["phases"], a["taps"], a["L"], a["H"], a["red"], a["lim"], a["work"], a["wd"])
tneed = L.RRX_limit_work_doubles(3, 4096, 12, 64)
tgood = dict(device=-1, stream=None, table=p, ntracks=3, nch=2, sf=0, rows=p, df=0, dst=q, row_frames=4096, gain=None, c=0.9, coefs=co_p, phases=4,
             taps=12, L=64, H=0, red=p, lim=p, work=w, wd=tneed)
def tcall(**kw):
    a = dict(tgood, **kw)
    return L.RRX_tracks_limit_device(a["device"], a["stream"], a["table"], a["ntracks"], a["nch"], a["sf"], a["rows"], a["df"], a["dst"],
                                     a["row_frames"], a["gain"], a["c"], a["coefs"], a["phases"], a["taps"], a["L"], a["H"], a["red"], a["lim"],
                                     a["work"], a["wd"])
print("uninit", call(), tcall())                          # before init_ratelib
print("init", L.init_ratelib(cb))                         # no device: refuses
print("uninit", call(), call(frames=0, wd=2 * 2 * 76), tcall(), tcall(row_frames=0))
src_bytes = (4096 + 1024) * 2 * 4
for name, kw in [("null", dict(src=None)), ("nstreams0", dict(nstreams=0)), ("nstreams-1", dict(nstreams=-1)), ("nch0", dict(nch=0)),
                 ("nch-1", dict(nch=-1)), ("srcfmt16", dict(sf=16)), ("srcfmt7", dict(sf=7)), ("sstride", dict(ss=1023)), ("sstride0", dict(ss=0)),
                 ("samples2^60", dict(frames=2**59, ss=2**59, ds=2**59)), ("srcrows2^60", dict(ss=2**58)), ("device-2", dict(device=-2)),
                 ("coefs", dict(coefs=None)), ("phases0", dict(phases=0)), ("phases9", dict(phases=9)), ("taps0", dict(taps=0)),
                 ("taps17", dict(taps=17)), ("inf", dict(coefs=C.cast(bad, C.c_void_p))),
                 ("dst", dict(dst=None)), ("dstfmt16", dict(df=16)), ("dstfmt7", dict(df=7)), ("dstride", dict(ds=1023)), ("dstrows2^60", dict(ds=2**58)),
                 ("c0", dict(c=0.0)), ("c-1", dict(c=-1.0)), ("cinf", dict(c=float("inf"))), ("cnan", dict(c=float("nan"))),
                 ("L0", dict(L=0)), ("L1025", dict(L=1025)), ("H4097", dict(H=4097)), ("work", dict(work=None)), ("wd", dict(wd=need - 1)),
                 ("wd-for-L", dict(L=65)), ("inplace-formats", dict(dst=p, df=1)), ("inplace-strides", dict(dst=p, ds=4097)),
                 ("overlap-above", dict(dst=p + 4)), ("overlap-end", dict(dst=p + src_bytes - 4)), ("overlap-below", dict(dst=p - 4)),
                 ("overlap-double-dst", dict(dst=p - 2 * src_bytes + 8, df=1))]:
    print("inv", name, call(**kw))
for name, kw in [("one-stream", dict(nstreams=1, ss=0, ds=0)), ("tight", dict(ss=1024, ds=1024)), ("double", dict(sf=1)), ("to-double", dict(df=1)),
                 ("no-stats", dict(red=None, lim=None)), ("gain", dict(gain=p)), ("8x16", dict(phases=8, taps=16, wd=2 * 2 * (1024 + 16 + 64))),
                 ("1x1", dict(phases=1, taps=1)), ("L1", dict(L=1)), ("widest", dict(L=1024, H=4096, wd=2 * 2 * (1024 + 12 + 1024))),
                 ("inplace", dict(dst=p)), ("inplace-one-stream", dict(dst=p, nstreams=1, ds=7)), ("adjacent-above", dict(dst=p + src_bytes)),
                 ("adjacent-below", dict(dst=p - src_bytes)), ("large-work", dict(wd=need + 1))]:
    print("ok", name, call(**kw))                         # nothing to refuse: answered RR_EXTUNINIT here
rows_bytes = 3 * 4096 * 2 * 4
for name, kw in [("table", dict(table=None)), ("rows", dict(rows=None)), ("dst", dict(dst=None)), ("ntracks0", dict(ntracks=0)), ("nch0", dict(nch=0)),
                 ("srcfmt16", dict(sf=16)), ("dstfmt24", dict(df=24)), ("coefs", dict(coefs=None)), ("phases9", dict(phases=9)), ("taps17", dict(taps=17)),
                 ("inf", dict(coefs=C.cast(bad, C.c_void_p))), ("rows2^60", dict(row_frames=2**58)), ("device-2", dict(device=-2)),
                 ("c0", dict(c=0.0)), ("cnan", dict(c=float("nan"))), ("L0", dict(L=0)), ("L1025", dict(L=1025)), ("H4097", dict(H=4097)),
                 ("work", dict(work=None)), ("wd", dict(wd=tneed - 1)), ("inplace-formats", dict(dst=p, df=1)), ("overlap", dict(dst=p + rows_bytes - 4)),
                 ("overlap-below", dict(dst=p - 8))]:
    print("tinv", name, tcall(**kw))
for name, kw in [("double", dict(sf=1)), ("to-double", dict(df=1)), ("gain", dict(gain=p)), ("3x5", dict(phases=3, taps=5)), ("inplace", dict(dst=p)),
                 ("adjacent", dict(dst=p + rows_bytes)), ("no-stats", dict(red=None, lim=None))]:
    print("tok", name, tcall(**kw))
"""


def test_invalid_parameters_are_refused_without_a_device():
    out = subprocess.run([sys.executable, "-c", CHILD % ROOT], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))
    assert out.returncode == 0, out.stderr
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.split() and ln.split()[0] in ("uninit", "init", "inv", "ok", "tinv", "tok")]
    assert ["init", "-1"] in lines
    uninit = [ln for ln in lines if ln[0] == "uninit"]
    assert len(uninit) == 2 and all(int(v) == RR_EXTUNINIT for ln in uninit for v in ln[1:])
    for kind, count, want in (("inv", 39, RR_INVPARAM), ("ok", 15, RR_EXTUNINIT), ("tinv", 23, RR_INVPARAM), ("tok", 7, RR_EXTUNINIT)):
        got = [ln for ln in lines if ln[0] == kind]
        assert len(got) == count and all(int(ln[2]) == want for ln in got), got


def test_host_twin_refuses_as_the_device_call_does_and_leaves_the_results_alone():
    x = np.ones((2, 8, 2), np.float32)
    y = np.full((2, 8, 2), GUARD)
    red, lim = np.full(2, 5, np.uint64), np.full(2, 6, np.uint64)
    need = F.limit_work_doubles(2, 8, 12, 64)
    work = np.full(need, GUARD)
    fn = F.lib().RRX_debug_limit_host

    def call(**kw):
        co = kw.get("coefs", BS)
        return fn(kw.get("sf", 0), kw.get("src", x.ctypes.data), kw.get("ss", 8), kw.get("df", 1), kw.get("dst", y.ctypes.data), kw.get("ds", 8),
                  kw.get("ns", 2), kw.get("frames", 8), kw.get("nch", 2), None, kw.get("c", 0.5), None if co is None else co.ctypes.data,
                  kw.get("phases", 4), kw.get("taps", 12), kw.get("L", 64), kw.get("H", 0), red.ctypes.data, lim.ctypes.data,
                  kw.get("work", work.ctypes.data), kw.get("wd", need))

    inf = BS.copy()
    inf[17] = -np.inf
    for kw in (dict(src=None), dict(ns=0), dict(nch=0), dict(sf=16), dict(ss=7), dict(ss=2 ** 58), dict(coefs=None), dict(phases=9), dict(taps=0),
               dict(coefs=inf), dict(dst=None), dict(df=16), dict(ds=7), dict(c=0.0), dict(c=np.nan), dict(c=np.inf), dict(L=0), dict(L=1025),
               dict(H=4097), dict(work=None), dict(wd=need - 1), dict(dst=x.ctypes.data), dict(dst=x.ctypes.data + 4, df=0)):
        assert call(**kw) == RR_INVPARAM, kw
        assert np.all(y == GUARD) and np.all(red == 5) and np.all(lim == 6) and np.all(work == GUARD) and np.all(x == 1), kw
    assert call(frames=0) == RR_OK  # nothing to do: nothing is touched
    assert np.all(y == GUARD) and np.all(red == 5) and np.all(lim == 6) and np.all(work == GUARD)
    assert call() == RR_OK and np.all(y <= 0.5) and np.all(lim == 6 + 8)
    assert np.all(red == 5)  # a reduction already below what the call finds stays
    z = x.copy()
    assert call(src=z.ctypes.data, dst=z.ctypes.data, df=0) == RR_OK and np.array_equal(z, y.astype(np.float32))  # in place
    code = ("import sys; sys.path.insert(0, %r)\nimport foo_dsp_resampler_amd as F\n"
            "print(F.lib().RRX_debug_limit_host(0, None, 0, 0, None, 0, 1, 0, 1, None, 1.0, None, 4, 12, 1, 0, None, None, None, 0))\n" % ROOT)
    env = {k: v for k, v in os.environ.items() if k != "RSMP_TEST_HOOKS"}
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-1] == "-1"


def test_python_wrappers_check_on_the_host():
    class Fake:  # stands in for a device tensor: the wrapper must refuse before any C call
        def __init__(self, shape, dtype="torch.float32", contiguous=True):
            self.shape, self.dtype, self._c = shape, dtype, contiguous

        def is_contiguous(self):
            return self._c

        def data_ptr(self):
            raise AssertionError("the arguments are checked before the pointer is taken")

    with pytest.raises(ValueError):
        F.limit_device(Fake((100,)), 0.9)
    with pytest.raises(ValueError):
        F.limit_device(Fake((100, 2), contiguous=False), 0.9)
    with pytest.raises(TypeError):
        F.limit_device(Fake((100, 2), dtype="torch.int16"), 0.9)
    with pytest.raises(ValueError):
        F.limit_device(Fake((100, 2)), 0.9, filter="bs1771")
    for kw in (dict(ceiling=0.0), dict(ceiling=float("nan")), dict(ceiling=float("inf")), dict(ceiling=-1.0), dict(ceiling=0.9, lookahead=0),
               dict(ceiling=0.9, lookahead=1025), dict(ceiling=0.9, hold=-1), dict(ceiling=0.9, hold=4097)):
        with pytest.raises(ValueError):
            F.limit_device(Fake((100, 2)), **kw)
    with pytest.raises(TypeError):
        F.limit_device(Fake((100, 2)), 0.9)  # not a device tensor


@pytest.mark.parametrize("shape", SHAPES)
def test_host_twin_equals_the_model_bit_for_bit(shape):
    rng = np.random.default_rng(sum(shape))
    ns, nch, frames = shape
    for sdt in (np.float32, np.float64):
        x = signal(rng, shape, sdt)
        for ddt in (np.float32, np.float64):
            for (L, H), g in zip(LH, (None, 0.5, 1.7, 1.7, 0.5)):
                gain = None if g is None else np.full(ns, g)
                rc, y, red, lim = host(x, 0.9, L, H, gain=gain, dst=ddt)
                assert rc == RR_OK
                wy, _, wred, wlim = M.limit(x, M.BS1770, 0.9, L, H, gain, ddt)
                assert M.same_samples(y, wy), (sdt, ddt, L, H, g)
                assert np.array_equal(red, wred) and np.array_equal(lim, wlim), (sdt, ddt, L, H, g)
    x = signal(rng, shape, np.float32)
    for g in (None, 0.5, 1.7):
        gain = None if g is None else np.linspace(g, 1.0, ns)
        for L, H in LH:
            rc, y, red, lim = host(x, 0.7, L, H, gain=gain)
            wy, _, wred, wlim = M.limit(x, M.BS1770, 0.7, L, H, gain)
            assert rc == RR_OK and M.same_samples(y, wy) and np.array_equal(red, wred) and np.array_equal(lim, wlim), (g, L, H)


def test_the_model_window_minimum_is_the_plain_one():
    rng = np.random.default_rng(2)
    r = rng.random((2, 300))
    for width in (1, 2, 3, 7, 8, 83, 300):
        want = np.stack([r[:, i:i + width].min(axis=1) for i in range(300 - width + 1)], axis=1)
        assert np.array_equal(M.window_min(r, width), want), width


def test_a_random_filter_and_rows_at_a_pitch_above_their_length():
    rng = np.random.default_rng(11)
    coefs = rng.standard_normal((3, 5))
    buf = M.planted(rng, (3, 1300, 2), np.float32)
    obuf = np.full((3, 1300, 2), GUARD)
    x = np.ascontiguousarray(buf[:, :1201])  # rows of 1201 frames at a pitch of 1300
    for L, H in LH:
        obuf[:] = GUARD
        rc, _, red, lim = host(buf[:, :1201], 0.9, L, H, coefs=coefs, stride=1300, out=obuf[:, :1201], gain=np.array([0.5, 1.0, 1.7]))
        assert rc == RR_OK and np.all(obuf[:, 1201:] == GUARD)
        wy, _, wred, wlim = M.limit(x, coefs, 0.9, L, H, np.array([0.5, 1.0, 1.7]))
        assert M.same_samples(np.ascontiguousarray(obuf[:, :1201]), wy) and np.array_equal(red, wred) and np.array_equal(lim, wlim), (L, H)


def test_a_ceiling_above_every_level_returns_the_gained_frames():
    rng = np.random.default_rng(12)
    x = (rng.standard_normal((2, 3000, 3)) * 0.1).astype(np.float32)
    gain = np.array([0.5, 1.7])
    for ddt in (np.float32, np.float64):
        for L, H in LH:
            rc, y, red, lim = host(x, 50.0, L, H, gain=gain, dst=ddt)
            want = (x.astype(np.float64) * gain[:, None, None]).astype(ddt)
            assert rc == RR_OK and M.same_samples(y, want) and np.all(red == M.ONE) and not lim.any()


def test_finite_input_stays_under_the_ceiling():
    rng = np.random.default_rng(13)
    for sdt in (np.float32, np.float64):
        x = (rng.standard_normal((2, 5000, 2)) * 3.0).astype(sdt)
        x[0, 0] = 40.0     # a peak in the very first frame
        x[1, -1] = -40.0   # and in the very last
        for c in (0.9, 1.0, 1e-3, 0.3333333333333333):
            for L, H in LH:
                rc, y, red, lim = host(x, c, L, H)
                assert rc == RR_OK and np.abs(y).max() <= c * (1 + 2.0 ** -51), (c, L, H)
                assert abs(y[0, 0, 0]) <= c * (1 + 2.0 ** -51) and abs(y[0, 0, 0]) > 0.2 * c  # limited, not muted
                assert abs(y[1, -1, 0]) <= c * (1 + 2.0 ** -51) and abs(y[1, -1, 0]) > 0.2 * c
                assert np.all(red.view(np.float64) < 1.0) and np.all(lim > 0)


def test_a_peak_in_the_flushed_tail_lowers_the_last_samples():
    """A tone at fs/4 sampled at +-0.7071 that ends abruptly: no sample is above 0.9, the tone's true peak is 1.005, and the
    largest detector value lies behind the last frame, where the filter runs out of the tone (F >= N)."""
    n = np.arange(400)
    x = np.sin(2 * np.pi * n / 4 + np.pi / 4).reshape(1, -1, 1)
    lev = M.levels(x, M.BS1770).view(np.float64)[0]
    assert np.abs(x).max() < 0.75 and lev[:400].max() > 1.0 and lev[400:].max() > 0.9
    quiet = x * 0.85                      # inside the tone the level is 0.854: only onset and tail could cross 0.86
    lev = M.levels(quiet, M.BS1770).view(np.float64)[0]
    c = 0.5 * (lev[20:395].max() + lev[400:].max())
    assert lev[20:395].max() < c < lev[400:].max()
    rc, y, red, lim = host(quiet, c, 8, 0)
    assert rc == RR_OK
    assert np.array_equal(y[0, 100:380], quiet[0, 100:380])     # the middle is untouched
    assert np.all(np.abs(y[0, -5:]) < np.abs(quiet[0, -5:]))     # the last samples are lowered by the peak behind them
    assert red.view(np.float64)[0] == c / lev[400:].max() or red.view(np.float64)[0] == c / lev.max()


def test_lookahead_one_is_the_minimum_over_the_filter_window():
    rng = np.random.default_rng(14)
    x = rng.standard_normal((2, 700, 2))
    c = 1.1
    rc, y, red, lim = host(x, c, 1, 0)
    assert rc == RR_OK
    lev = M.levels(x, M.BS1770).view(np.float64)                 # [2, 700 + 11]
    r = np.where(lev > c, c / np.where(lev > c, lev, 1.0), 1.0)
    s = np.stack([r[:, n:n + 12].min(axis=1) for n in range(700)], axis=1)   # s[n] = min r[n .. n + D]
    assert np.array_equal(y, x * s[:, :, None])
    assert np.array_equal(lim, (s < 1).sum(axis=1)) and np.array_equal(red.view(np.float64), s.min(axis=1))


def test_non_finite_samples():
    rng = np.random.default_rng(15)
    x = (rng.standard_normal((2, 600, 3)) * 0.3).astype(np.float32)
    clean = x.copy()
    x[1, 300, 1] = np.nan
    x[1, 450, 2] = np.inf
    rc, y, red, lim = host(x, 0.9, 64, 0)
    rc2, y2, red2, lim2 = host(clean, 0.9, 64, 0)
    assert rc == RR_OK and rc2 == RR_OK
    assert np.array_equal(y[0], y2[0]) and red[0] == red2[0] and lim[0] == lim2[0]     # the other stream is exact
    assert np.isnan(y[1, 300, 1]) and np.isnan(y[1, 450, 2])
    assert np.isnan(y[1]).sum() == 2
    assert np.array_equal(y[1, 300, [0, 2]], y2[1, 300, [0, 2]])                          # a NaN level demands nothing
    assert not y[1, 440:450].any() and not y[1, 451:462].any()                            # +inf demands +0.0 around it
    assert red.view(np.float64)[1] == 0.0


def test_tracks_are_one_stream_calls_on_slices():
    """What RRX_tracks_limit_device promises per track, on the host: a slice of a row limited as its own stream, from +0.0 in
    front of it, into the same frames of the destination rows, nothing else written."""
    rng = np.random.default_rng(16)
    rows = (rng.standard_normal((3, 900, 2)) * 0.6).astype(np.float32)
    out = rows.copy()
    for t, (of, n) in enumerate([(0, 900), (100, 650), (899, 1)]):
        sl = rows[t:t + 1, of:of + n]
        rc, _, red, lim = host(sl, 0.9, 72, 480, stride=900, out=out[t:t + 1, of:of + n])
        assert rc == RR_OK
        wy, _, wred, wlim = M.limit(np.ascontiguousarray(sl), M.BS1770, 0.9, 72, 480, None, np.float32)
        assert M.same_samples(np.ascontiguousarray(out[t:t + 1, of:of + n]), wy) and np.array_equal(red, wred) and np.array_equal(lim, wlim)
        assert np.array_equal(out[t, :of], rows[t, :of]) and np.array_equal(out[t, of + n:], rows[t, of + n:])
    whole = M.limit(rows[1:2], M.BS1770, 0.9, 72, 480, None, np.float32)[0]
    assert not np.array_equal(whole[0, 100:750], out[1, 100:750])  # the row in front of a slice is not its history


def bed_with_bursts(rng, rate=48000, seconds=2.0, nch=2):
    n = int(rate * seconds)
    x = rng.standard_normal((1, n, nch)) * 10.0 ** (-30.0 / 20.0)
    burst = 0.9 * np.sin(2 * np.pi * np.arange(40) / 4 + np.pi / 4)
    for b in range(8):
        at = (b + 1) * n // 10
        x[0, at:at + 40] = burst[:, None]
    return x.astype(np.float32)


def lufs_of(x, gain=None):
    rc, energy, _, _ = loudness_host(x, 4800, coefs=np.array(F.k_weighting(48000)), gain=gain)
    assert rc == RR_OK
    res = gate_host(energy[:, :, :x.shape[1] // 4800], 4800)
    return -0.691 + 10 * np.log10(res[0, 0] / res[0, 1])


def test_the_limiter_brings_a_bed_with_bursts_closer_to_its_loudness_target():
    """Noise at -30 dBFS RMS with eight 40-frame fs/4 bursts at 0.9, target -14 LUFS under -1 dBTP, everything through the host
    twins: the peak-bound gain min(by loudness, by peak) against the limiter at (72, 480) followed by the static trim.  On this
    signal (measured at -19.7 LUFS: the bursts carry a large share of its K-weighted energy) the peak-bound gain leaves the track
    5.9 LU under the target and the limiter 2.8 LU, a margin of 3.1 LU -- half the 6 dB of the unweighted estimate, because
    what the limiter takes from the bursts it takes from the loudness too.  The gain is flat across a 40-frame burst, so the
    trim finds nothing left over here (DESIGN.md 10 has the residuals of signals where it does)."""
    target, ceiling = -14.0, 10.0 ** (-1.0 / 20.0)
    x = bed_with_bursts(np.random.default_rng(17))
    lufs = lufs_of(x)
    by_loudness = 10.0 ** ((target - lufs) / 20.0)
    tp, pk, _ = true_peak_of(x)
    by_peak = ceiling / max(tp, pk)
    normalized = lufs_of(x, np.array([min(by_loudness, by_peak)]))
    rc, y, red, lim = host(x, ceiling, 72, 480, gain=np.array([by_loudness]), dst=np.float32)
    assert rc == RR_OK and lim[0] > 0
    tp, pk, _ = true_peak_of(y)
    trim = min(1.0, ceiling / max(tp, pk))
    limited = lufs_of(y, np.array([trim]))
    tp2, pk2, _ = true_peak_of(y, np.array([trim]))
    d_lim, d_norm = abs(limited - target), abs(normalized - target)
    print("measured %.3f LUFS; by loudness %.4f, by peak %.4f; peak-bound gain leaves %.3f LUFS (%.3f LU off), limiter + trim %.3f LUFS "
          "(%.3f LU off): margin %.3f LU; overshoot after the limiter %.4f %%, trim %.6f, reduction %.4f, limited frames %d"
          % (lufs, by_loudness, by_peak, normalized, d_norm, limited, d_lim, d_norm - d_lim, 100 * (max(tp, pk) / ceiling - 1), trim,
             red.view(np.float64)[0], lim[0]))
    assert max(tp2, pk2) <= ceiling * (1 + 1e-12)
    assert d_lim < d_norm


def true_peak_of(x, gain=None):
    ns, frames, nch = x.shape
    tp, pk = np.zeros((ns, nch), np.uint64), np.zeros((ns, nch), np.uint64)
    rc = F.lib().RRX_debug_true_peak_host(int(x.dtype == np.float64), x.ctypes.data, frames, ns, frames, nch, None if gain is None else gain.ctypes.data,
                                          0, BS.ctypes.data, 4, 12, 1, None, None, tp.ctypes.data, pk.ctypes.data)
    assert rc == RR_OK
    return float(tp.view(np.float64).max()), float(pk.view(np.float64).max()), None
