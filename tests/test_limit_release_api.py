"""The host side of the limiter's release (RRX_limit_release_device / RRX_tracks_limit_release_device /
RRX_limit_release_work_doubles / RRX_debug_limit_release_host): the symbols and the header's text, the refusals that need no
device, the arithmetic -- the host twin is serial loops over the very functions the kernels call -- against the numpy restatement
in limit_release_model.py, bit for bit, the properties that do not rest on that model, and the distance of the blocked form to
the plain serial recursion.  CPU only."""
import os
import subprocess
import sys

import numpy as np
import pytest

import foo_dsp_resampler_amd as F
import limit_release_model as R
from test_limit_api import host as limit_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RR_OK, RR_EXTUNINIT, RR_INVPARAM = 0, 5, 6
SHAPES = [(1, 1, 1), (1, 2, 11), (3, 3, 4099), (2, 6, 1201)]  # (nstreams, nch, frames)
# J = frames + L - 1 at L = 64, block 64: one block, one block + 1, 256 blocks, 256 blocks + 1
SEAMS = [(1, 2, 1), (1, 2, 2), (1, 1, 256 * 64 - 63), (2, 1, 256 * 64 - 62)]
LH = [(1, 0), (64, 0), (72, 480), (1024, 4096)]
AB = [(R.coef(50, 44100), 64), (R.coef(200, 96000), 65), (R.coef(1000, 192000), 1024)]
BS = np.ascontiguousarray(R.BS1770.reshape(-1))
GUARD = 777.25
NAMES = ("RRX_limit_release_work_doubles", "RRX_limit_release_device", "RRX_tracks_limit_release_device", "RRX_debug_limit_release_host")
# The largest relative difference of q between the blocked form and the serial recursion over the cases of
# test_distance_to_the_serial_recursion, as measured, and the bound that test holds: the next power of ten above it.
SERIAL_DISTANCE_MEASURED, SERIAL_DISTANCE_BOUND = 6.8e-13, 1e-12


def host(x, ceiling, L, H, a, block, coefs=R.BS1770, gain=None, dst=np.float64, red=None, lim=None):
    """RRX_debug_limit_release_host on x [nstreams, frames, nch]: (rc, y, reduction bits, limited).  The work buffer is three doubles
    longer than needed, under guards."""
    ns, frames, nch = x.shape
    coefs = np.ascontiguousarray(coefs, dtype=np.float64)
    y = np.full((ns, frames, nch), GUARD, dtype=dst)
    red = np.full(ns, R.ONE) if red is None else red
    lim = np.zeros(ns, np.uint64) if lim is None else lim
    g = None if gain is None else np.ascontiguousarray(gain, dtype=np.float64)
    need = F.limit_release_work_doubles(ns, frames, coefs.shape[1], L, block)
    assert need == R.work_doubles(ns, frames, coefs.shape[1], L, block) and need > 0
    work = np.full(need + 3, GUARD)
    rc = F.lib().RRX_debug_limit_release_host(int(x.dtype == np.float64), x.ctypes.data, frames, int(y.dtype == np.float64), y.ctypes.data, frames,
                                              ns, frames, nch, None if g is None else g.ctypes.data, float(ceiling), coefs.ctypes.data,
                                              coefs.shape[0], coefs.shape[1], L, H, float(a), block, red.ctypes.data, lim.ctypes.data,
                                              work.ctypes.data, need)
    assert np.all(work[need:] == GUARD)
    return rc, y, red, lim


def signal(rng, shape, dtype):
    ns, nch, frames = shape
    if frames >= 1000:
        return R.planted(rng, (ns, frames, nch), dtype)
    return (rng.standard_normal((ns, frames, nch)) * 0.5).astype(dtype)


def test_symbols_are_exported_listed_and_declared():
    header = open(os.path.join(ROOT, "include", "ratelib_amd.h")).read()
    for name in NAMES:
        assert name in F.EXPECTED_SYMBOLS and name in F.available_symbols()
        assert name + "(" in header
    assert "#define RRX_LIMIT_RELEASE_MIN_BLOCK 64" in header and "#define RRX_LIMIT_RELEASE_MAX_BLOCK 65536" in header
    assert (F.RRX_LIMIT_RELEASE_MIN_BLOCK, F.RRX_LIMIT_RELEASE_MAX_BLOCK) == (64, 65536) == (R.MIN_BLOCK, R.MAX_BLOCK)
    for name in ("limit_release_coef", "limit_release_work_doubles", "limit_release_device", "tracks_limit_release_device"):
        assert callable(getattr(F, name)) and name in F.__all__
    # the three loops and what holds of them are stated
    assert "C = v_0;  A = a;  B = b * v_0" in header
    assert "for t = 1 .. n-1:  u = b * v_t;  C = fmin(v_t, a * C + u);  A = a * A;  B = a * B + u" in header
    assert "carry:  S_0 = 1.0;  S_{i+1} = fmin(C_i, A_i * S_i + B_i)" in header
    assert "run of block i:  p = S_i;  for t = 0 .. n-1:  u = b * v_t;  p = fmin(v_t, a * p + u);  q[i*block + t] = p" in header
    assert "q[j] <= v[j]" in header and "NOT bit-equal" in header
    assert ("%.1e" % SERIAL_DISTANCE_MEASURED) in header
    makefile = open(os.path.join(ROOT, "foo_dsp_resampler_amd", "csrc", "Makefile")).read()
    assert "limit_release.hip" in makefile and "FP_limit_release := -ffp-contract=off" in makefile
    import inspect
    sig = inspect.signature(F.Resampler.convert_tracks_to_pcm_loudness_limited)
    assert list(sig.parameters)[-2:] == ["release_ms", "release_block"]
    assert sig.parameters["release_ms"].default is None and sig.parameters["release_block"].default == 1024


def test_release_coef():
    import math
    assert F.limit_release_coef(50, 44100) == math.exp(-1 / (50 * 1e-3 * 44100)) == R.coef(50, 44100)
    assert isinstance(F.limit_release_coef(200, 96000), float) and 0 < F.limit_release_coef(0.001, 8000) < F.limit_release_coef(1000, 192000) < 1
    for bad in (0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            F.limit_release_coef(bad, 48000)


def test_work_doubles():
    w = F.lib().RRX_limit_release_work_doubles
    assert w(3, 1000, 12, 64, 1024) == 3 * (2 * (1000 + 12 + 64) + 4 * (2 + 1)) == F.limit_release_work_doubles(3, 1000)
    assert w(1, 0, 1, 1, 64) == 4 + 4 and w(1, 1, 12, 64, 64) == 2 * 77 + 8 and w(1, 2, 12, 64, 64) == 2 * 78 + 12
    assert w(2, 100, 12, 64, 65) == R.work_doubles(2, 100, 12, 64, 65) == 2 * (2 * 176 + 4 * 4)
    for bad in ((0, 10, 12, 64, 64), (-1, 10, 12, 64, 64), (1, 10, 0, 64, 64), (1, 10, 17, 64, 64), (1, 10, 12, 0, 64), (1, 10, 12, 1025, 64),
                (1, 10, 12, 64, 63), (1, 10, 12, 64, 65537), (1, 10, 12, 64, 0)):
        assert w(*bad) == 0, bad
    # the total reaches 2^60 or not: the first frame count at which it does, by bisection on the formula
    for ns, block in ((1, 65536), (1, 64), (3, 1000)):
        total = lambda f: ns * (2 * (f + 76) + 4 * (-(-(f + 63) // block) + 1))  # noqa: E731
        lo, hi = 0, 2 ** 60
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if total(mid) >= 2 ** 60 else (mid, hi)
        assert total(lo) < 2 ** 60 <= total(hi)
        assert w(ns, lo, 12, 64, block) == total(lo) == R.work_doubles(ns, lo, 12, 64, block) and w(ns, hi, 12, 64, block) == 0
    assert w(2 ** 31 - 1, 2 ** 29, 12, 64, 1024) == 0 and w(1, 2 ** 64 - 1, 12, 64, 1024) == 0 and w(3, 2 ** 63, 16, 1024, 64) == 0


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
co_p = C.cast(co, C.c_void_p)
need = L.RRX_limit_release_work_doubles(2, 1024, 12, 64, 1024)
good = dict(device=-1, stream=None, sf=0, src=p, ss=4096, df=0, dst=q, ds=4096, nstreams=2, frames=1024, nch=2, gain=None, c=0.9, coefs=co_p, phases=4,
            taps=12, L=64, H=0, a=0.999, block=1024, red=p, lim=p, work=w, wd=need)
def call(**kw):
    a = dict(good, **kw)
    return L.RRX_limit_release_device(a["device"], a["stream"], a["sf"], a["src"], a["ss"], a["df"], a["dst"], a["ds"], a["nstreams"], a["frames"],
                                      a["nch"], a["gain"], a["c"], a["coefs"], a["phases"], a["taps"], a["L"], a["H"], a["a"], a["block"], a["red"],
                                      a["lim"], a["work"], a["wd"])
tneed = L.RRX_limit_release_work_doubles(3, 4096, 12, 64, 1024)
tgood = dict(device=-1, stream=None, table=p, ntracks=3, nch=2, sf=0, rows=p, df=0, dst=q, row_frames=4096, gain=None, c=0.9, coefs=co_p, phases=4,
             taps=12, L=64, H=0, a=0.999, block=1024, red=p, lim=p, work=w, wd=tneed)
def tcall(**kw):
    a = dict(tgood, **kw)
    return L.RRX_tracks_limit_release_device(a["device"], a["stream"], a["table"], a["ntracks"], a["nch"], a["sf"], a["rows"], a["df"], a["dst"],
                                             a["row_frames"], a["gain"], a["c"], a["coefs"], a["phases"], a["taps"], a["L"], a["H"], a["a"],
                                             a["block"], a["red"], a["lim"], a["work"], a["wd"])
print("uninit", call(), tcall())                          # before init_ratelib
print("init", L.init_ratelib(cb))                         # no device: refuses
print("uninit", call(), call(frames=0, wd=L.RRX_limit_release_work_doubles(2, 0, 12, 64, 1024)), tcall(), tcall(row_frames=0))
cases = [("a-0.1", dict(a=-0.1)), ("a1.0", dict(a=1.0)), ("a1.5", dict(a=1.5)), ("anan", dict(a=float("nan"))), ("ainf", dict(a=float("inf"))),
         ("block63", dict(block=63)), ("block65537", dict(block=65537)), ("block0", dict(block=0)), ("work", dict(work=None)),
         ("c0", dict(c=0.0)), ("L0", dict(L=0)), ("L1025", dict(L=1025)), ("H4097", dict(H=4097)), ("coefs", dict(coefs=None)),
         ("dstfmt7", dict(df=7)), ("device-2", dict(device=-2)), ("inplace-formats", dict(dst=p, df=1)), ("overlap", dict(dst=p + 4))]
for name, kw in cases + [("wd", dict(wd=need - 1)), ("wd-plain", dict(wd=L.RRX_limit_work_doubles(2, 1024, 12, 64))), ("wd-for-block", dict(block=512)),
                         ("null", dict(src=None)), ("nstreams0", dict(nstreams=0)), ("sstride", dict(ss=1023)), ("dstride", dict(ds=1023))]:
    print("inv", name, call(**kw))
for name, kw in [("a0", dict(a=0.0)), ("block64", dict(block=64, wd=L.RRX_limit_release_work_doubles(2, 1024, 12, 64, 64))), ("block65536", dict(block=65536)),
                 ("block1000", dict(block=1000, wd=need + 4)), ("inplace", dict(dst=p)), ("double", dict(sf=1, df=1)), ("no-stats", dict(red=None, lim=None)),
                 ("gain", dict(gain=p)), ("large-work", dict(wd=need + 1))]:
    print("ok", name, call(**kw))                         # nothing to refuse: answered RR_EXTUNINIT here
for name, kw in cases + [("wd", dict(wd=tneed - 1)), ("table", dict(table=None)), ("rows", dict(rows=None)), ("ntracks0", dict(ntracks=0)),
                         ("rows2^60", dict(row_frames=2**58))]:
    print("tinv", name, tcall(**kw))
for name, kw in [("a0", dict(a=0.0)), ("block65536", dict(block=65536)), ("inplace", dict(dst=p)), ("to-double", dict(df=1)), ("gain", dict(gain=p))]:
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
    for kind, count, want in (("inv", 25, RR_INVPARAM), ("ok", 9, RR_EXTUNINIT), ("tinv", 23, RR_INVPARAM), ("tok", 5, RR_EXTUNINIT)):
        got = [ln for ln in lines if ln[0] == kind]
        assert len(got) == count and all(int(ln[2]) == want for ln in got), got


def test_host_twin_refuses_as_the_device_call_does_and_leaves_the_results_alone():
    x = np.ones((2, 8, 2), np.float32)
    y = np.full((2, 8, 2), GUARD)
    red, lim = np.full(2, 5, np.uint64), np.full(2, 6, np.uint64)
    need = F.limit_release_work_doubles(2, 8, 12, 64, 64)
    work = np.full(need, GUARD)
    fn = F.lib().RRX_debug_limit_release_host

    def call(**kw):
        return fn(0, kw.get("src", x.ctypes.data), 8, kw.get("df", 1), kw.get("dst", y.ctypes.data), 8, 2, kw.get("frames", 8), 2, None, kw.get("c", 0.5),
                  BS.ctypes.data, 4, 12, kw.get("L", 64), kw.get("H", 0), kw.get("a", 0.99), kw.get("block", 64), red.ctypes.data, lim.ctypes.data,
                  kw.get("work", work.ctypes.data), kw.get("wd", need))

    for kw in (dict(a=-0.1), dict(a=1.0), dict(a=1.5), dict(a=np.nan), dict(block=63), dict(block=65537), dict(wd=need - 1), dict(work=None),
               dict(src=None), dict(dst=None), dict(c=0.0), dict(L=0), dict(H=4097), dict(dst=x.ctypes.data), dict(df=16)):
        assert call(**kw) == RR_INVPARAM, kw
        assert np.all(y == GUARD) and np.all(red == 5) and np.all(lim == 6) and np.all(work == GUARD) and np.all(x == 1), kw
    assert call(frames=0) == RR_OK  # nothing to do: nothing is touched
    assert np.all(y == GUARD) and np.all(red == 5) and np.all(lim == 6) and np.all(work == GUARD)
    assert call() == RR_OK and np.all(y <= 0.5) and np.all(lim == 6 + 8) and np.all(red == 5)
    z = x.copy()
    assert call(src=z.ctypes.data, dst=z.ctypes.data, df=0) == RR_OK and np.array_equal(z, y.astype(np.float32))  # in place
    code = ("import sys; sys.path.insert(0, %r)\nimport foo_dsp_resampler_amd as F\n"
            "print(F.lib().RRX_debug_limit_release_host(0, None, 0, 0, None, 0, 1, 0, 1, None, 1.0, None, 4, 12, 1, 0, 0.5, 64, None, None, None, 0))\n"
            % ROOT)
    env = {k: v for k, v in os.environ.items() if k != "RSMP_TEST_HOOKS"}
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-1] == "-1"


def test_python_wrappers_check_on_the_host():
    class Fake:  # stands in for a device tensor: the wrapper must refuse before any C call
        def __init__(self, shape, dtype="torch.float32"):
            self.shape, self.dtype = shape, dtype

        def is_contiguous(self):
            return True

        def data_ptr(self):
            raise AssertionError("the arguments are checked before the pointer is taken")

    for kw in (dict(release=-0.1), dict(release=1.0), dict(release=1.5), dict(release=float("nan")), dict(release=0.5, block=63),
               dict(release=0.5, block=65537), dict(release=0.5, lookahead=0), dict(release=0.5, hold=4097)):
        with pytest.raises(ValueError):
            F.limit_release_device(Fake((100, 2)), 0.9, **kw)
    with pytest.raises(ValueError):
        F.limit_release_device(Fake((100,)), 0.9, 0.5)
    with pytest.raises(TypeError):
        F.limit_release_device(Fake((100, 2), dtype="torch.int16"), 0.9, 0.5)
    with pytest.raises(TypeError):
        F.limit_release_device(Fake((100, 2)), 0.9, 0.5)  # not a device tensor


def test_the_model_without_a_release_is_the_limiter_model():
    rng = np.random.default_rng(3)
    x = R.planted(rng, (2, 1500, 2), np.float32)
    for L, H in LH:
        g, m = R.window_minima(x, R.BS1770, 0.9, L, H, np.array([0.5, 1.7]))
        want = R.M.limit(x, R.BS1770, 0.9, L, H, np.array([0.5, 1.7]), np.float32)
        for got in (R.smooth(g, m, L, np.float32), R.limit_release(x, R.BS1770, 0.9, L, H, 0.0, 65, np.array([0.5, 1.7]), np.float32)):
            assert R.same_samples(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
            assert np.array_equal(got[3], want[3])


@pytest.mark.parametrize("shape", SHAPES + SEAMS)
def test_host_twin_equals_the_model_bit_for_bit(shape):
    rng = np.random.default_rng(sum(shape))
    ns, nch, frames = shape
    seam = shape in SEAMS
    for sdt in (np.float32, np.float64):
        x = signal(rng, shape, sdt)
        for ddt in (np.float32, np.float64):
            for (L, H), g in zip([(64, 0)] if seam else LH, (None, 0.5, 1.7, 1.7)):
                gain = None if g is None else np.linspace(g, 1.0, ns)
                for a, block in AB[:1] if seam else AB:
                    rc, y, red, lim = host(x, 0.9, L, H, a, block, gain=gain, dst=ddt)
                    assert rc == RR_OK
                    wy, _, wred, wlim = R.limit_release(x, R.BS1770, 0.9, L, H, a, block, gain, ddt)
                    assert R.same_samples(y, wy), (sdt, ddt, L, H, g, a, block)
                    assert np.array_equal(red, wred) and np.array_equal(lim, wlim), (sdt, ddt, L, H, g, a, block)
    x = signal(rng, shape, np.float32)
    for g in (None, 1.7):  # every (L, H) with and without a gain, at a lower ceiling
        gain = None if g is None else np.linspace(g, 1.0, ns)
        for L, H in [(64, 0)] if seam else LH:
            for a, block in AB[:1] if seam else AB:
                rc, y, red, lim = host(x, 0.3, L, H, a, block, gain=gain)
                wy, _, wred, wlim = R.limit_release(x, R.BS1770, 0.3, L, H, a, block, gain)
                assert rc == RR_OK and R.same_samples(y, wy) and np.array_equal(red, wred) and np.array_equal(lim, wlim), (g, L, H, a, block)


@pytest.mark.parametrize("shape", SHAPES)
def test_release_zero_is_the_limiter(shape):
    rng = np.random.default_rng(5 + sum(shape))
    ns = shape[0]
    for sdt, ddt in ((np.float32, np.float32), (np.float64, np.float32), (np.float32, np.float64)):
        x = signal(rng, shape, sdt)
        for (L, H), g in zip(LH, (None, 0.5, 1.7, 1.7)):
            gain = None if g is None else np.full(ns, g)
            for block in (64, 65, 1024):
                rc, y, red, lim = host(x, 0.9, L, H, 0.0, block, gain=gain, dst=ddt)
                rc2, y2, red2, lim2 = limit_host(x, 0.9, L, H, gain=gain, dst=ddt)
                assert rc == RR_OK and rc2 == RR_OK
                assert y.tobytes() == y2.tobytes() and np.array_equal(red, red2) and np.array_equal(lim, lim2), (sdt, ddt, L, H, block)


def test_the_gain_never_exceeds_the_window_minimum_and_finite_input_stays_under_the_ceiling():
    rng = np.random.default_rng(13)
    for sdt in (np.float32, np.float64):
        x = (rng.standard_normal((2, 5000, 2)) * 3.0).astype(sdt)
        x[0, 0] = 40.0     # a peak in the very first frame
        x[1, -1] = -40.0   # and in the very last
        for c in (0.9, 1e-3, 0.3333333333333333):
            for L, H in LH:
                for a, block in AB:
                    rc, y, red, lim = host(x, c, L, H, a, block)
                    assert rc == RR_OK and np.abs(y).max() <= c * (1 + 2.0 ** -51), (c, L, H, a)
                    assert abs(y[0, 0, 0]) > 0.2 * c and abs(y[1, -1, 0]) > 0.2 * c  # limited, not muted
                    rc2, _, red2, lim2 = limit_host(x, c, L, H)
                    assert rc2 == RR_OK and np.all(lim >= lim2) and np.all(red <= red2), (c, L, H, a)
    x = R.planted(rng, (2, 3000, 2), np.float32)
    for L, H in LH:
        g, m = R.window_minima(x, R.BS1770, 0.9, L, H)
        for a, block in AB:
            q = R.release(m, a, block)
            assert np.all(q <= m) and not np.isnan(q).any() and np.all(q >= 0)
            _, s, _, _ = R.smooth(g, q, L, np.float64)
            assert np.all(s <= m[:, L - 1:]), (L, H, a)


def test_the_gain_recovers_exponentially_behind_an_isolated_peak():
    """DC at 0.1 under a ceiling of 0.5 with one sample at 4.0: s = y / x.  From the end of the hold -- the last frame whose window
    minimum is the peak's -- the gain covers 1 - 1/e of its way back to 1.0 within round(release_ms * rate / 1000) frames, give or
    take `lookahead` frames for the box.  (Lookaheads of at least the filter's taps: the detector spreads the peak over `taps` frames,
    and their smaller demands follow the hold for up to taps - 1 frames, which a box of one frame would not cover.)"""
    rate, at = 48000, 3000
    for release_ms, (L, H), block in ((10.0, (64, 100), 64), (50.0, (72, 480), 1024), (100.0, (1024, 0), 65)):
        T = int(round(release_ms * rate / 1000))
        x = np.full((1, at + H + 8 * T, 1), 0.1)
        x[0, at, 0] = 4.0
        rc, y, red, lim = host(x, 0.5, L, H, F.limit_release_coef(release_ms, rate), block)
        assert rc == RR_OK
        s = y[0, :, 0] / x[0, :, 0]
        _, m = R.window_minima(x, R.BS1770, 0.5, L, H)
        m = m[0, L - 1:]
        end = int(np.flatnonzero(m == m.min())[-1])                  # the end of the hold
        low = s.min()
        assert low == red.view(np.float64)[0] and low < 0.2
        back = int(np.flatnonzero((1.0 - s[end:]) <= (1.0 - low) / np.e)[0])
        assert abs(back - T) <= L, (release_ms, L, H, back, T)
        assert np.all(np.diff(s[end + L + 12:]) >= 0) and 1.0 - s[-1] < 1e-3   # monotone behind the box and the filter; and back up
        # without a release the gain is back at 1.0 a box behind the hold
        _, y0, _, _ = limit_host(x, 0.5, L, H)
        assert np.all(y0[0, end + L + 12:, 0] == x[0, end + L + 12:, 0]) and lim[0] > T


def test_the_gain_recovers_from_an_infinite_sample():
    x = np.full((1, 6000, 1), 0.25)
    x[0, 500, 0] = np.inf
    rc, y, red, lim = host(x, 0.9, 64, 0, F.limit_release_coef(10, 48000), 64)
    assert rc == RR_OK and red.view(np.float64)[0] == 0.0 and not y[0, 500 - 11:500, 0].any()
    assert np.isnan(y[0, 500, 0]) and np.isnan(y).sum() == 1
    assert y[0, -1, 0] > 0.2499 and np.all(np.diff(y[0, 600:, 0]) >= 0)   # towards the target, from +0.0


def serial_distances():
    """the largest relative difference of q between the blocked form and the serial recursion, per (a, block), over the shapes, the
    seams and every (L, H) of this file: planted and sparse to dense reductions"""
    rng = np.random.default_rng(21)
    worst = {}
    for shape in SHAPES + SEAMS:
        ns, nch, frames = shape
        for c, scale in ((0.9, 1.0), (0.3, 1.0), (0.9, 0.35)):   # dense, denser, sparse attacks
            x = signal(rng, shape, np.float64) * scale
            for L, H in LH:
                _, m = R.window_minima(x, R.BS1770, c, L, H)
                for a, block in AB:
                    qb, qs = R.release(m, a, block), R.serial(m, a)
                    assert np.array_equal(qb == 0, qs == 0)
                    d = np.abs(qb - qs) / np.where(qs == 0, 1.0, qs)
                    worst[(a, block)] = max(worst.get((a, block), 0.0), float(d.max()) if d.size else 0.0)
    return worst


def test_distance_to_the_serial_recursion():
    worst = serial_distances()
    for (a, block), d in sorted(worst.items()):
        print("a = %.9f, block %5d: largest relative difference to the serial recursion %.3e" % (a, block, d))
    assert max(worst.values()) <= SERIAL_DISTANCE_BOUND
    assert "%.1e" % max(worst.values()) == "%.1e" % SERIAL_DISTANCE_MEASURED   # what the header and DESIGN.md quote
    assert max(worst.values()) > 0.0   # the two are not bit-equal: the decomposition is the ABI
