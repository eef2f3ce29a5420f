"""The shaped output stage's host side (RRX_finish_shaped_device / RRX_debug_finish_shaped_host / RRX_tracks_finish_shaped_device):
the symbols, the refusals that need no device, and the arithmetic -- the host twin is a serial loop over the very functions the
kernel calls -- against the numpy restatement in shaped_model.py, bit for bit; what the ABI promises about zero coefficients,
padding, chunks and non-finite samples; and what the segments cost in quality.  CPU only."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import foo_dsp_resampler_amd as F
import finish_model as M
import shaped_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RR_OK, RR_EXTUNINIT, RR_INVPARAM = 0, 5, 6
SEED = 0x1234567887654321
NEW = ("RRX_finish_shaped_device", "RRX_debug_finish_shaped_host", "RRX_tracks_finish_shaped_device")
ORDERS = (1, 5, 9, 16)
SEGMENTS = (0, 1, 7, 64, 5000)
FIRSTS = (0, 3, 2 ** 32 + 5)
TARGETS = [(f, True) for f in SM.FORMATS] + [(F.RRX_FMT_S16, False)]      # (format, write): the last is measure only


def test_symbols_are_exported_and_listed():
    header = open(os.path.join(ROOT, "include", "ratelib_amd.h")).read()
    for name in NEW:
        assert name in F.EXPECTED_SYMBOLS and name in F.available_symbols()
        assert name in header
    assert "#define RRX_SHAPE_MAX_ORDER 16" in header and F.RRX_SHAPE_MAX_ORDER == 16
    assert callable(F.finish_shaped_device) and callable(F.tracks_finish_shaped_device)
    assert F.NOISE_SHAPES["lipshitz5"] == (2.033, -2.165, 1.959, -1.590, 0.6149)
    assert F.NOISE_SHAPES["wannamaker3"] == (1.623, -0.982, 0.109)
    assert F.NOISE_SHAPES["wannamaker9"] == (2.412, -3.370, 3.937, -4.174, 3.353, -2.205, 1.281, -0.569, 0.0847)


CHILD = r"""
import sys, ctypes as C
sys.path.insert(0, %r)
import foo_dsp_resampler_amd as F
L = F.lib()
cb = F.ratelib._ALLOC_CB(lambda: None)
fn = L.RRX_finish_shaped_device
p = 0x10000  # never dereferenced: every call below is answered from its arguments, or from the library's state, alone
D = C.c_double
k3 = (D * 3)(1.623, -0.982, 0.109)
k16 = (D * 16)(*([0.5] * 16))
knan = (D * 3)(1.0, float("nan"), 0.0)
kinf = (D * 2)(1.0, float("-inf"))
kbeyond = (D * 3)(1.0, 0.5, float("nan"))       # order 2: the NaN is not part of the filter
adr = lambda a: C.cast(a, C.c_void_p)
STATE = 2 * 2 * 16 * 8                          # bytes of the state of 2 streams x 2 channels
good = dict(device=-1, stream=None, sf=0, src=p, ss=4096, df=16, dst=p, ds=4096, nstreams=2, frames=1024, nch=2, gain=None, dither=1,
            seed=7, first=0, coefs=adr(k3), order=3, segment=64, sin=None, sout=None, peak=p, clipped=p)
def call(**kw):
    a = dict(good, **kw)
    return fn(a["device"], a["stream"], a["sf"], a["src"], a["ss"], a["df"], a["dst"], a["ds"], a["nstreams"], a["frames"], a["nch"],
              a["gain"], a["dither"], a["seed"], a["first"], a["coefs"], a["order"], a["segment"], a["sin"], a["sout"], a["peak"], a["clipped"])
print("uninit", call())                                   # before init_ratelib
print("init", L.init_ratelib(cb))                         # no device: refuses
print("uninit", call(), call(frames=0))
for name, kw in [("null", dict(src=None)), ("nstreams0", dict(nstreams=0)), ("nstreams-1", dict(nstreams=-1)), ("nch0", dict(nch=0)),
                 ("nch-1", dict(nch=-1)), ("srcfmt16", dict(sf=16)), ("srcfmt7", dict(sf=7)), ("dstfmt0", dict(df=0)), ("dstfmt1", dict(df=1)),
                 ("dstfmt8", dict(df=8)), ("sstride", dict(ss=1023)), ("dstride", dict(ds=1023)), ("sstride0", dict(ss=0)),
                 ("nothing", dict(dst=None, peak=None, clipped=None)), ("wrap", dict(first=2**64 - 1024)),
                 ("wrap1", dict(first=2**64 - 1, frames=1, ss=1, ds=1, segment=1)),
                 ("samples2^60", dict(frames=2**59, ss=2**59, ds=2**59)), ("srcrows2^60", dict(ss=2**58)), ("dstrows2^60", dict(ds=2**58)),
                 ("device-2", dict(device=-2)),
                 # the shaped call's own
                 ("measure-dstfmt0", dict(dst=None, df=0)), ("measure-dstfmt8", dict(dst=None, df=8)),
                 ("coefs-null", dict(coefs=None)), ("order0", dict(order=0)), ("order-1", dict(order=-1)), ("order17", dict(coefs=adr(k16), order=17)),
                 ("coef-nan", dict(coefs=adr(knan))), ("coef-inf", dict(coefs=adr(kinf), order=2)),
                 ("inside-no-state", dict(first=3)), ("inside-no-state-0", dict(first=5, segment=0)),
                 ("inside-no-state-frames0", dict(first=65, frames=0)),
                 ("state-equal", dict(sin=p, sout=p)), ("state-overlap-above", dict(sin=p, sout=p + STATE - 8)),
                 ("state-overlap-below", dict(sin=p + 8, sout=p)), ("state-equal-at-a-start", dict(first=128, sin=p, sout=p))]:
    print("inv", name, call(**kw))
for name, kw in [("one-stream", dict(nstreams=1, ss=0, ds=0)), ("tight", dict(ss=1024, ds=1024)), ("s24", dict(df=24)), ("s32", dict(df=32)),
                 ("double", dict(sf=1)), ("measure", dict(dst=None, ds=0)), ("measure-s24", dict(dst=None, df=24, clipped=None)),
                 ("no-stats", dict(peak=None, clipped=None)), ("last-frame", dict(first=2**64 - 1025, segment=1)),
                 ("order16", dict(coefs=adr(k16), order=16)), ("order1", dict(order=1)), ("nan-beyond-the-order", dict(coefs=adr(kbeyond), order=2)),
                 ("segment0", dict(segment=0)), ("segment1", dict(segment=1, first=12345)), ("segment-huge", dict(segment=2**63)),
                 ("at-a-start", dict(first=128)), ("inside-with-state", dict(first=3, sin=p)), ("inside-0-with-state", dict(first=5, segment=0, sin=p)),
                 ("state-out", dict(sout=p)), ("states-adjacent", dict(sin=p, sout=p + STATE)), ("states-adjacent-below", dict(sin=p + STATE, sout=p))]:
    print("ok", name, call(**kw))                         # nothing to refuse: answered RR_EXTUNINIT here

tr = L.RRX_tracks_finish_shaped_device
tgood = dict(device=-1, stream=None, table=p, ntracks=3, nch=2, sf=0, rows=p, row_frames=4096, df=16, dst=p, dst_total=9000, gain=None, dither=1,
             seed=7, coefs=adr(k3), order=3, segment=64, peak=p, clipped=p)
def tcall(**kw):
    a = dict(tgood, **kw)
    return tr(a["device"], a["stream"], a["table"], a["ntracks"], a["nch"], a["sf"], a["rows"], a["row_frames"], a["df"], a["dst"], a["dst_total"],
              a["gain"], a["dither"], a["seed"], a["coefs"], a["order"], a["segment"], a["peak"], a["clipped"])
for name, kw in [("table", dict(table=None)), ("rows", dict(rows=None)), ("ntracks0", dict(ntracks=0)), ("nch0", dict(nch=0)), ("srcfmt16", dict(sf=16)),
                 ("dstfmt8", dict(df=8)), ("measure-dstfmt0", dict(dst=None, df=0)), ("nothing", dict(dst=None, peak=None, clipped=None)),
                 ("rows2^60", dict(row_frames=2**58)), ("dst2^60", dict(dst_total=2**59)), ("device-2", dict(device=-2)),
                 ("coefs-null", dict(coefs=None)), ("order0", dict(order=0)), ("order17", dict(coefs=adr(k16), order=17)), ("coef-nan", dict(coefs=adr(knan)))]:
    print("tinv", name, tcall(**kw))
for name, kw in [("good", dict()), ("measure", dict(dst=None)), ("segment0", dict(segment=0)), ("rows0", dict(row_frames=0)), ("double-s24", dict(sf=1, df=24))]:
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
    for tag, count, want in (("inv", 35, RR_INVPARAM), ("ok", 21, RR_EXTUNINIT), ("tinv", 15, RR_INVPARAM), ("tok", 5, RR_EXTUNINIT)):
        got = [ln for ln in lines if ln[0] == tag]
        assert len(got) == count and all(int(ln[2]) == want for ln in got), got


def test_host_twin_refuses_as_the_device_call_does_and_is_inert_without_test_hooks():
    x = np.zeros((2, 8, 2), np.float32)
    k = np.array([1.0, -0.5])
    for kw, rc in ((dict(), RR_OK), (dict(first_frame=3), RR_INVPARAM), (dict(first_frame=3, state=np.zeros((2, 2, 16))), RR_OK),
                   (dict(first_frame=64), RR_OK)):
        SM.host(x, F.RRX_FMT_S16, k, 64, rc=rc, **kw)
    SM.host(x, F.RRX_FMT_S16, np.array([1.0, np.inf]), 64, rc=RR_INVPARAM)
    fn = F.lib().RRX_debug_finish_shaped_host
    pk = np.zeros(4, np.uint64)
    st = np.zeros(2 * 2 * 16 + 1)
    args = lambda **kw: [0, kw.get("src", x.ctypes.data), 8, kw.get("df", 16), None, 8, 2, 8, 2, None, 0, 0, kw.get("first", 0),
                         kw.get("coefs", k.ctypes.data), kw.get("order", 2), 64, kw.get("sin"), kw.get("sout"), kw.get("peak", pk.ctypes.data), None]
    assert fn(*args()) == RR_OK
    for kw in (dict(src=None), dict(df=0), dict(df=8), dict(coefs=None), dict(order=0), dict(order=17), dict(peak=None), dict(first=2 ** 64 - 4),
               dict(first=1), dict(sin=st.ctypes.data, sout=st.ctypes.data), dict(sin=st.ctypes.data, sout=st.ctypes.data + 8)):
        assert fn(*args(**kw)) == RR_INVPARAM, kw
    code = ("import sys; sys.path.insert(0, %r)\nimport foo_dsp_resampler_amd as F\n"
            "print(F.lib().RRX_debug_finish_shaped_host(0, None, 0, 16, None, 0, 1, 0, 1, None, 0, 0, 0, None, 0, 0, None, None, None, None))\n" % ROOT)
    env = {k_: v for k_, v in os.environ.items() if k_ != "RSMP_TEST_HOOKS"}
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

    S16 = F.RRX_FMT_S16
    for bad in (dict(x=Fake((100,))), dict(x=Fake((100, 2), contiguous=False)), dict(fmt=8), dict(fmt=None), dict(shaping="nobody"),
                dict(shaping=[]), dict(shaping=[0.5] * 17), dict(shaping=[1.0, float("nan")]), dict(segment=-1), dict(first_frame=3),
                dict(first_frame=5, segment=0), dict(first_frame=2 ** 64 - 50, segment=1)):
        kw = dict(x=Fake((100, 2)), fmt=S16, shaping="wannamaker9", segment=64, first_frame=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            F.finish_shaped_device(kw["x"], kw["fmt"], kw["shaping"], kw["segment"], first_frame=kw["first_frame"])
    with pytest.raises(TypeError):
        F.finish_shaped_device(Fake((100, 2), dtype="torch.int16"), S16, "lipshitz5")
    with pytest.raises(TypeError):
        F.finish_shaped_device(Fake((100, 2)), S16, "lipshitz5")                  # not a device tensor
    import inspect
    sig = inspect.signature(F.finish_shaped_device)
    assert list(sig.parameters) == ["x", "dst_format", "shaping", "segment", "gain", "dither", "seed", "first_frame", "state", "out", "peak",
                                    "clipped", "stream"]
    assert sig.parameters["segment"].default == 65536 and sig.parameters["dither"].default is True
    for name in ("convert_track_to_pcm_device", "convert_tracks_to_pcm_device", "convert_tracks_to_pcm_streamed", "convert_library_to_pcm"):
        ps = inspect.signature(getattr(F.Resampler, name)).parameters
        assert ps["shaping"].default is None and ps["segment"].default == 65536, name


def run_both(x, fmt, write, coefs, segment, g, dith, first, what):
    st = None if SM.restarts(first, segment) else SM.random_state(x.shape[0], x.shape[2], len(coefs))
    want = SM.model(x, fmt, coefs, segment, g, dith, SEED, first, st, write=write)
    got = SM.host(x, fmt, coefs, segment, g, dith, SEED, first, st, write=write)
    SM.same(got, want, x, what)
    return got


@pytest.mark.parametrize("frames", M.FRAMES)
@pytest.mark.parametrize("nstreams,nch", M.SHAPES)
def test_host_twin_equals_the_model_bit_for_bit(nstreams, nch, frames):
    """formats and measure only x float32 / float64 x orders x segments x first frames in full for the short inputs, with the gains
    and the dither switch going round beside them; the long input, whose model takes a Python loop over a whole segment, takes
    every (order, segment) pair with the other axes going round, so that every value of every axis meets several of the others"""
    gains = lambda v: None if v is None else v * (1 + 0.25 * np.arange(nstreams))
    if frames < 100:
        for i, ((fmt, write), double, order, segment, first) in enumerate(itertools.product(TARGETS, (False, True), ORDERS, SEGMENTS, FIRSTS)):
            x = SM.make_input(nstreams, frames, nch, fmt, double)
            gain, dith = M.GAINS[i % 3], bool((i // 3) % 2)
            run_both(x, fmt, write, SM.coefs_of(order), segment, gains(gain), dith, first, (fmt, write, double, order, segment, first, gain, dith))
        return
    seen = set()
    for i, (order, segment) in enumerate(itertools.product(ORDERS, SEGMENTS)):
        (fmt, write), double, gain, dith, first = TARGETS[i % 4], bool((i // 4 + i) % 2), M.GAINS[i % 3], bool((i // 2) % 2), FIRSTS[(i // 5 + i) % 3]
        x = SM.make_input(nstreams, frames, nch, fmt, double)
        run_both(x, fmt, write, SM.coefs_of(order), segment, gains(gain), dith, first, (fmt, write, double, order, segment, first, gain, dith))
        seen |= {("t", fmt, write), ("d", double), ("g", gain), ("n", dith), ("f", first)}
    assert len(seen) == 4 + 2 + 3 + 2 + 3
    # the planted values did their work: a NaN peak in one channel, infinities, clipped samples
    x = SM.make_input(nstreams, frames, nch, F.RRX_FMT_S32, False)
    _, pk, cl, _ = SM.host(x, F.RRX_FMT_S32, SM.W9, 64, None, True, SEED)
    nanch = SM.nan_channels(x)
    assert nanch.sum() == 1 and np.isnan(pk.view(np.float64)[nanch]).all()
    assert cl.sum() >= 5 * nstreams


@pytest.mark.parametrize("segment", [0, 7, 5000])
def test_zero_coefficients_are_the_unshaped_call_bit_for_bit(segment):
    """order 1, coefficient 0.0: RRX_debug_finish_host's bytes, peaks and clip counts, with and without dither, for the planted NaN,
    +-inf, -0.0, ties and denormals alike -- and so for any number of zero coefficients"""
    for fmt, double, gain, dith in itertools.product(SM.FORMATS, (False, True), (None, 1.7), (False, True)):
        x = np.array(SM.make_input(3, 4099, 3, fmt, double))
        x[2, 17, 1] = -0.0
        x[1, 300:310, 2] = -0.0
        g = None if gain is None else gain * (1 + 0.25 * np.arange(3))
        want = M.host(x, fmt, g, dith, SEED, 11)
        st = None if SM.restarts(11, segment) else SM.random_state(3, 3, 1)
        for zeros in (1, 16):
            got = SM.host(x, fmt, np.zeros(zeros), segment, g, dith, SEED, 11, st)
            for k, what in enumerate(("output bytes", "peak bit patterns", "clip counts")):
                assert np.array_equal(got[k], want[k]), (what, fmt, double, gain, dith, zeros)


def test_padding_with_zero_coefficients_changes_no_bit():
    x = SM.make_input(2, 4099, 3, F.RRX_FMT_S16, False)
    for segment, first in ((64, 3), (0, 0), (5000, 2 ** 32 + 5)):
        st5 = None if SM.restarts(first, segment) else SM.random_state(2, 3, 5)
        a = SM.host(x, F.RRX_FMT_S16, SM.L5, segment, None, True, SEED, first, st5)
        for size in (8, 16):
            b = SM.host(x, F.RRX_FMT_S16, np.concatenate([SM.L5, np.zeros(size - 5)]), segment, None, True, SEED, first, st5)
            assert all(np.array_equal(p, q) for p, q in zip(a[:3], b[:3])), (segment, first, size)
            assert np.array_equal(a[3][:, :, :5], b[3][:, :, :5])      # (the padded filter's state goes on: the errors are the same)


CUTS = (1, 63, 64, 65, 4000)


@pytest.mark.parametrize("segment", [64, 0, 5000])
@pytest.mark.parametrize("first", [0, 3])
def test_chunked_calls_that_hand_the_state_on_give_one_call(segment, first):
    x = SM.make_input(2, 4099, 3, F.RRX_FMT_S24_3, False)
    g = np.array([0.5, 1.7])
    st = None if SM.restarts(first, segment) else SM.random_state(2, 3, 9)
    whole = SM.host(x, F.RRX_FMT_S24_3, SM.W9, segment, g, True, SEED, first, st)
    SM.same(whole, SM.model(x, F.RRX_FMT_S24_3, SM.W9, segment, g, True, SEED, first, st), x, ("one call", segment, first))
    parts, pk, cl = [], None, None
    for lo, hi in zip((0,) + CUTS, CUTS + (4099,)):
        o, pk, cl, st = SM.host(np.ascontiguousarray(x[:, lo:hi]), F.RRX_FMT_S24_3, SM.W9, segment, g, True, SEED, first + lo, st, pk, cl)
        parts.append(o)
    got = (np.concatenate(parts, axis=1), pk, cl, st)
    for k, what in enumerate(("output bytes", "peak bit patterns", "clip counts", "state")):
        assert np.array_equal(got[k].view(np.uint8), whole[k].view(np.uint8)), (what, segment, first)
    # no frames: nothing is touched, the state included
    o, pk2, cl2, st2 = SM.host(np.ascontiguousarray(x[:, :0]), F.RRX_FMT_S24_3, SM.W9, segment, g, True, SEED, first + 4099, st, pk, cl)
    assert np.array_equal(pk2, pk) and np.array_equal(cl2, cl) and (st2 == 77.0).all()


def test_a_non_finite_sample_leaves_no_trace_in_the_history():
    """the error of a NaN or infinite sample is stored as 0.0: with a one-tap filter the very next sample is the unshaped call's,
    every sample equals the model's, and no state ever holds anything but a finite number"""
    rng = np.random.default_rng(8)
    x = rng.uniform(-0.5, 0.5, (1, 600, 2))
    where = {100: np.nan, 200: np.inf, 300: -np.inf, 400: 1e300, 599: np.nan}
    for i, v in where.items():
        x[0, i, 0] = v
    plain = M.host(x, F.RRX_FMT_S16, None, True, SEED)[0].view("<i2").reshape(600, 2)
    for coefs in (np.array([0.9]), SM.W9):
        for segment in (0, 64):
            got = SM.host(x, F.RRX_FMT_S16, coefs, segment, None, True, SEED)
            SM.same(got, SM.model(x, F.RRX_FMT_S16, coefs, segment, None, True, SEED), x, (len(coefs), segment))
            assert np.isfinite(got[3]).all()
            q = got[0].view("<i2").reshape(600, 2)
            if len(coefs) == 1:
                for i in where:
                    if i + 1 < 600:
                        assert q[i + 1, 0] == plain[i + 1, 0], i
                assert (q[1:, 0] != plain[1:, 0]).mean() > 0.3      # (elsewhere the filter is at work)
            for cut in where:                                       # a state taken right behind the sample holds 0.0 for it
                st = SM.host(np.ascontiguousarray(x[:, :cut + 1]), F.RRX_FMT_S16, coefs, segment, None, True, SEED)[3]
                assert st[0, 0, 0] == 0.0 and np.isfinite(st).all()


def band_noise_db(segment, coefs, n=1 << 20):
    """the table of DESIGN.md 10: a 997 Hz sine at 0.25 of full scale, 2^20 mono frames at 44.1 kHz, S16, TPDF dither; Hann window,
    mean of |FFT|^2 over [2000, 5000) Hz of (output - input * 2^15), in dB"""
    x = (0.25 * np.sin(2 * np.pi * 997 / 44100 * np.arange(n))).reshape(1, n, 1)
    out = SM.host(x, F.RRX_FMT_S16, coefs, segment, None, True, SEED)[0].view("<i2").reshape(n).astype(np.float64)
    err = out - x.reshape(n) * 2.0 ** 15
    spec = np.abs(np.fft.rfft(err * np.hanning(n))) ** 2
    f = np.fft.rfftfreq(n, 1 / 44100)
    return 10 * np.log10(spec[(f >= 2000) & (f < 5000)].mean()), np.abs(err).max()


def test_what_the_segments_cost_in_quality():
    flat, _ = band_noise_db(0, np.zeros(1))
    never, worst = band_noise_db(0, SM.W9)
    default, _ = band_noise_db(65536, SM.W9)
    short, _ = band_noise_db(256, SM.W9)
    print("2-5 kHz noise against plain TPDF: never %.2f dB, 65536 %.2f dB, 256 %.2f dB; largest error %.1f LSB"
          % (never - flat, default - flat, short - flat, worst))
    assert never <= flat - 20
    assert abs(default - never) <= 0.5
    assert short >= never + 8          # the check can see a restart
