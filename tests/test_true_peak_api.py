"""The true-peak pass's host side (RRX_true_peak_device / RRX_tracks_true_peak_device / RRX_debug_true_peak_host): the symbols, the
refusals that need no device, and the arithmetic -- the host twin is a serial loop over the very function the kernels call --
against the numpy restatement in true_peak_model.py, bit for bit.  CPU only."""
import os
import subprocess
import sys

import numpy as np
import pytest

import foo_dsp_resampler_amd as F
import true_peak_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RR_OK, RR_EXTUNINIT, RR_INVPARAM = 0, 5, 6
SHAPES = [(1, 1, 1), (1, 2, 11), (1, 2, 12), (1, 2, 13), (3, 3, 4099), (2, 5, 1201)]
BS = np.ascontiguousarray(M.BS1770.reshape(-1))


def host(x, coefs=M.BS1770, gain=None, first_frame=0, flush=True, state=None, tp=None, pk=None, want_state=True, stride=None):
    """RRX_debug_true_peak_host on x [nstreams, frames, nch]: (rc, true peak bits, peak bits, state_out)"""
    ns, frames, nch = x.shape
    coefs = np.ascontiguousarray(coefs, dtype=np.float64)
    tp = np.zeros((ns, nch), np.uint64) if tp is None else tp
    pk = np.zeros((ns, nch), np.uint64) if pk is None else pk
    so = np.full((ns, nch, 16), 7.0) if want_state else None
    g = None if gain is None else np.ascontiguousarray(gain, dtype=np.float64)
    rc = F.lib().RRX_debug_true_peak_host(int(x.dtype == np.float64), x.ctypes.data, frames if stride is None else stride, ns, frames, nch,
                                          None if g is None else g.ctypes.data, first_frame, coefs.ctypes.data, coefs.shape[0], coefs.shape[1],
                                          1 if flush else 0, None if state is None else state.ctypes.data,
                                          None if so is None else so.ctypes.data, tp.ctypes.data, pk.ctypes.data)
    return rc, tp, pk, so


def test_symbols_are_exported_and_listed():
    header = open(os.path.join(ROOT, "include", "ratelib_amd.h")).read()
    for name in ("RRX_true_peak_device", "RRX_tracks_true_peak_device", "RRX_debug_true_peak_host"):
        assert name in F.EXPECTED_SYMBOLS and name in F.available_symbols()
        assert name in header
    assert "#define RRX_TP_MAX_PHASES 8" in header and "#define RRX_TP_MAX_TAPS 16" in header
    assert (F.RRX_TP_MAX_PHASES, F.RRX_TP_MAX_TAPS) == (8, 16) == (M.MAX_PHASES, M.MAX_TAPS)
    assert callable(F.true_peak_device) and callable(F.tracks_true_peak_device)
    assert hasattr(F.Resampler, "convert_tracks_to_pcm_normalized")


def test_the_bs1770_table():
    phases, taps, coefs = F.TRUE_PEAK_FILTERS["bs1770"]
    assert (phases, taps) == (4, 12) and len(coefs) == 48
    c = np.array(coefs).reshape(4, 12)
    num = c * 8192.0
    assert np.array_equal(num, np.rint(num))  # numerators over 8192, exactly
    assert tuple(num[0].astype(int)) == (14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68)
    assert tuple(num[1].astype(int)) == (-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155)
    assert np.array_equal(c[2], c[1][::-1]) and np.array_equal(c[3], c[0][::-1])
    assert [int(v) for v in num.sum(axis=1)] == [8205, 7971, 7971, 8205]
    proto = c.T.reshape(-1)  # h[4k + p] = coefs[p][k]
    assert np.array_equal(proto, proto[::-1])
    assert np.array_equal(c, M.BS1770)


CHILD = r"""
import sys, ctypes as C
sys.path.insert(0, %r)
import foo_dsp_resampler_amd as F
L = F.lib()
cb = F.ratelib._ALLOC_CB(lambda: None)
p = 0x10000  # never dereferenced: every call below is answered from its arguments, or from the library's state, alone
co = (C.c_double * 128)(*([0.25] * 128))
bad = (C.c_double * 48)(*([0.25] * 47 + [float("inf")]))
nan = (C.c_double * 48)(*([float("nan")] + [0.25] * 47))
co_p = C.cast(co, C.c_void_p)
good = dict(device=-1, stream=None, sf=0, src=p, ss=4096, nstreams=2, frames=1024, nch=2, gain=None, first=0, coefs=co_p, phases=4, taps=12,
            flush=1, sin=None, sout=p + (1 << 20), tp=p, pk=p)
def call(**kw):
    a = dict(good, **kw)
    return L.RRX_true_peak_device(a["device"], a["stream"], a["sf"], a["src"], a["ss"], a["nstreams"], a["frames"], a["nch"], a["gain"],
                                  a["first"], a["coefs"], a["phases"], a["taps"], a["flush"], a["sin"], a["sout"], a["tp"], a["pk"])
tgood = dict(device=-1, stream=None, table=p, ntracks=3, nch=2, sf=0, rows=p, row_frames=4096, gain=None, coefs=co_p, phases=4, taps=12, tp=p, pk=p)
def tcall(**kw):
    a = dict(tgood, **kw)
    return L.RRX_tracks_true_peak_device(a["device"], a["stream"], a["table"], a["ntracks"], a["nch"], a["sf"], a["rows"], a["row_frames"],
                                         a["gain"], a["coefs"], a["phases"], a["taps"], a["tp"], a["pk"])
print("uninit", call(), tcall())                          # before init_ratelib
print("init", L.init_ratelib(cb))                         # no device: refuses
print("uninit", call(), call(frames=0), tcall(), tcall(row_frames=0))
for name, kw in [("null", dict(src=None)), ("nstreams0", dict(nstreams=0)), ("nstreams-1", dict(nstreams=-1)), ("nch0", dict(nch=0)),
                 ("nch-1", dict(nch=-1)), ("srcfmt16", dict(sf=16)), ("srcfmt7", dict(sf=7)), ("sstride", dict(ss=1023)), ("sstride0", dict(ss=0)),
                 ("nothing", dict(tp=None, pk=None)), ("wrap", dict(first=2**64 - 1024, sin=p + (2 << 20))),
                 ("samples2^60", dict(frames=2**59, ss=2**59)), ("srcrows2^60", dict(ss=2**58)), ("device-2", dict(device=-2)),
                 ("coefs", dict(coefs=None)), ("phases0", dict(phases=0)), ("phases9", dict(phases=9)), ("taps0", dict(taps=0)),
                 ("taps17", dict(taps=17)), ("inf", dict(coefs=C.cast(bad, C.c_void_p))), ("nan", dict(coefs=C.cast(nan, C.c_void_p))),
                 ("first-without-state", dict(first=1)), ("same-state", dict(first=5, sin=p + (1 << 20))),
                 ("overlapping-state", dict(first=5, sin=p + (1 << 20) + 8)), ("same-state-at-0", dict(sin=p + (1 << 20))),
                 ("overlap-below", dict(first=5, sin=p + (1 << 20) - 2 * 2 * 16 * 8 + 8))]:
    print("inv", name, call(**kw))
for name, kw in [("one-stream", dict(nstreams=1, ss=0)), ("tight", dict(ss=1024)), ("double", dict(sf=1)), ("tp-only", dict(pk=None)),
                 ("pk-only", dict(tp=None)), ("no-state-out", dict(sout=None)), ("state", dict(first=5, sin=p + (2 << 20))),
                 ("adjacent-state", dict(first=5, sin=p + (1 << 20) - 2 * 2 * 16 * 8)), ("state-unread-at-0", dict(sin=p + (2 << 20))),
                 ("8x16", dict(phases=8, taps=16)), ("1x1", dict(phases=1, taps=1)), ("no-flush", dict(flush=0)),
                 ("last-frame", dict(first=2**64 - 1025, sin=p + (2 << 20))), ("rows-below-2^60", dict(ss=2**58 - 1))]:
    print("ok", name, call(**kw))                         # nothing to refuse: answered RR_EXTUNINIT here
for name, kw in [("table", dict(table=None)), ("rows", dict(rows=None)), ("ntracks0", dict(ntracks=0)), ("nch0", dict(nch=0)), ("srcfmt16", dict(sf=16)),
                 ("nothing", dict(tp=None, pk=None)), ("coefs", dict(coefs=None)), ("phases9", dict(phases=9)), ("taps17", dict(taps=17)),
                 ("inf", dict(coefs=C.cast(bad, C.c_void_p))), ("rows2^60", dict(row_frames=2**58)), ("device-2", dict(device=-2))]:
    print("tinv", name, tcall(**kw))
for name, kw in [("double", dict(sf=1)), ("tp-only", dict(pk=None)), ("pk-only", dict(tp=None)), ("gain", dict(gain=p)), ("3x5", dict(phases=3, taps=5))]:
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
    for kind, count, want in (("inv", 26, RR_INVPARAM), ("ok", 14, RR_EXTUNINIT), ("tinv", 12, RR_INVPARAM), ("tok", 5, RR_EXTUNINIT)):
        got = [ln for ln in lines if ln[0] == kind]
        assert len(got) == count and all(int(ln[2]) == want for ln in got), got


def test_host_twin_refuses_as_the_device_call_does_and_leaves_the_results_alone():
    x = np.ones((2, 8, 2), np.float32)
    tp, pk = np.full((2, 2), 5, np.uint64), np.full((2, 2), 6, np.uint64)
    state = np.zeros((2, 2, 16))
    fn = F.lib().RRX_debug_true_peak_host

    def call(**kw):
        so = np.full((2, 2, 16), 7.0)
        co = kw.get("coefs", BS)
        rc = fn(kw.get("sf", 0), kw.get("src", x.ctypes.data), kw.get("ss", 8), kw.get("ns", 2), kw.get("frames", 8), kw.get("nch", 2), None,
                kw.get("first", 0), None if co is None else co.ctypes.data, kw.get("phases", 4), kw.get("taps", 12), 1,
                kw.get("sin", None), so.ctypes.data if kw.get("sout", True) is True else kw["sout"],
                tp.ctypes.data if kw.get("tp", True) else None, pk.ctypes.data if kw.get("pk", True) else None)
        return rc, so

    inf = BS.copy()
    inf[17] = -np.inf
    nan = BS.copy()
    nan[47] = np.nan
    for kw in (dict(src=None), dict(ns=0), dict(nch=0), dict(sf=16), dict(ss=7), dict(tp=False, pk=False), dict(first=2 ** 64 - 4, sin=state.ctypes.data),
               dict(ss=2 ** 58), dict(coefs=None), dict(phases=0), dict(phases=9), dict(taps=0), dict(taps=17), dict(coefs=inf), dict(coefs=nan),
               dict(first=3), dict(first=3, sin=state.ctypes.data, sout=state.ctypes.data), dict(sin=state.ctypes.data, sout=state.ctypes.data + 64)):
        rc, so = call(**kw)
        assert rc == RR_INVPARAM, kw
        assert np.all(tp == 5) and np.all(pk == 6) and np.all(so == 7.0) and not state.any(), kw
    rc, so = call(frames=0)  # nothing to do, even with flush: nothing is touched
    assert rc == RR_OK and np.all(tp == 5) and np.all(pk == 6) and np.all(so == 7.0)
    rc, so = call()
    assert rc == RR_OK and not np.all(so == 7.0) and np.all(pk == np.float64(1.0).view(np.uint64))
    code = ("import sys; sys.path.insert(0, %r)\nimport foo_dsp_resampler_amd as F\n"
            "print(F.lib().RRX_debug_true_peak_host(0, None, 0, 1, 0, 1, None, 0, None, 4, 12, 1, None, None, None, None))\n" % ROOT)
    env = {k: v for k, v in os.environ.items() if k != "RSMP_TEST_HOOKS"}
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-1] == "-1"


def test_python_wrapper_checks_on_the_host():
    class Fake:  # stands in for a device tensor: the wrapper must refuse before any C call
        def __init__(self, shape, dtype="torch.float32", contiguous=True):
            self.shape, self.dtype, self._c = shape, dtype, contiguous

        def is_contiguous(self):
            return self._c

        def data_ptr(self):
            raise AssertionError("the arguments are checked before the pointer is taken")

    with pytest.raises(ValueError):
        F.true_peak_device(Fake((100,)))
    with pytest.raises(ValueError):
        F.true_peak_device(Fake((100, 2), contiguous=False))
    with pytest.raises(TypeError):
        F.true_peak_device(Fake((100, 2), dtype="torch.int16"))
    with pytest.raises(ValueError):
        F.true_peak_device(Fake((100, 2)), filter="bs1771")
    with pytest.raises(ValueError):
        F.true_peak_device(Fake((100, 2)), filter=(4, 12, [0.0] * 47))
    with pytest.raises(ValueError):
        F.true_peak_device(Fake((100, 2)), filter=(9, 1, [0.0] * 9))
    with pytest.raises(ValueError):
        F.true_peak_device(Fake((100, 2)), filter=(1, 2, [0.0, float("inf")]))
    with pytest.raises(ValueError):
        F.true_peak_device(Fake((100, 2)), first_frame=5)  # no state
    with pytest.raises(ValueError):
        F.true_peak_device(Fake((100, 2)), first_frame=2 ** 64 - 50)
    with pytest.raises(TypeError):
        F.true_peak_device(Fake((100, 2)))  # not a device tensor


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", SHAPES)
def test_host_twin_equals_the_model_bit_for_bit(shape, dtype):
    rng = np.random.default_rng(hash((shape, np.dtype(dtype).name)) & 0xffff)
    ns, frames, nch = shape
    for g in (None, 0.5, 1.7):
        for flush in (False, True):
            x = M.planted(rng, shape, dtype)
            gain = None if g is None else np.full(ns, g)
            rc, tp, pk, so = host(x, gain=gain, flush=flush)
            assert rc == RR_OK
            mt, mp, ms = M.true_peak(x, M.BS1770, gain, flush)
            assert np.array_equal(tp, mt) and np.array_equal(pk, mp), (g, flush)
            assert np.array_equal(so.view(np.uint64), ms.view(np.uint64)), (g, flush)
            assert not so[:, :, 11:].any()  # entries at taps - 1 and beyond are 0


def test_other_filter_shapes_and_strides():
    rng = np.random.default_rng(11)
    for phases, taps in ((3, 5), (8, 16), (1, 1), (2, 2)):
        coefs = rng.standard_normal((phases, taps))
        buf = M.planted(rng, (3, 700, 2), np.float32)
        x = buf[:, :601]  # rows of 601 frames at a pitch of 700
        tp = np.zeros((3, 2), np.uint64)
        pk = np.zeros((3, 2), np.uint64)
        so = np.zeros((3, 2, 16))
        rc = F.lib().RRX_debug_true_peak_host(0, buf.ctypes.data, 700, 3, 601, 2, None, 0, np.ascontiguousarray(coefs).ctypes.data, phases, taps, 1,
                                              None, so.ctypes.data, tp.ctypes.data, pk.ctypes.data)
        assert rc == RR_OK
        mt, mp, ms = M.true_peak(np.ascontiguousarray(x), coefs)
        assert np.array_equal(tp, mt) and np.array_equal(pk, mp) and np.array_equal(so.view(np.uint64), ms.view(np.uint64)), (phases, taps)


def test_a_nan_channel_leaves_a_nan_and_its_neighbours_are_exact():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((2, 300, 3)) * 0.5).astype(np.float32)
    clean = x.copy()
    x[1, 150, 1] = np.nan
    rc, tp, pk, _ = host(x, gain=np.array([0.5, 1.7]))
    rc2, tp2, pk2, _ = host(clean, gain=np.array([0.5, 1.7]))
    assert rc == RR_OK and rc2 == RR_OK
    assert np.isnan(M.as_double(tp)[1, 1]) and np.isnan(M.as_double(pk)[1, 1])
    mask = np.ones((2, 3), bool)
    mask[1, 1] = False
    assert np.array_equal(tp[mask], tp2[mask]) and np.array_equal(pk[mask], pk2[mask])
    assert not np.isnan(M.as_double(tp)[mask]).any()


def test_peak_is_the_output_stage_measure_only_peak():
    rng = np.random.default_rng(6)
    for dtype in (np.float32, np.float64):
        x = M.planted(rng, (3, 1201, 2), dtype)
        gain = np.array([0.5, 1.7, 1.0])
        rc, _, pk, _ = host(x, gain=gain)
        ref = np.zeros((3, 2), np.uint64)
        rc2 = F.lib().RRX_debug_finish_host(int(dtype == np.float64), x.ctypes.data, 1201, 0, None, 0, 3, 1201, 2, gain.ctypes.data, 0, 0, 0,
                                            ref.ctypes.data, None)
        assert rc == RR_OK and rc2 == RR_OK
        assert np.array_equal(pk, ref)


@pytest.mark.parametrize("coefs", [M.BS1770, np.random.default_rng(3).standard_normal((3, 5))], ids=["bs1770", "3x5"])
def test_chunked_calls_that_hand_the_state_on_equal_one_call(coefs):
    rng = np.random.default_rng(7)
    taps = coefs.shape[1]
    x = M.planted(rng, (2, 997, 3), np.float32)
    gain = np.array([0.5, 1.7])
    rc, tp1, pk1, so1 = host(x, coefs, gain=gain)
    assert rc == RR_OK
    _, _, _, so_noflush = host(x, coefs, gain=gain, flush=False)
    assert np.array_equal(so1.view(np.uint64), so_noflush.view(np.uint64))  # the flushed frames do not enter the state
    for cuts in ([1], [max(taps - 2, 1)], [taps - 1], [taps], [int(rng.integers(taps + 1, 990))], [1, 2, 3, 5, taps + 7, 500], [3, 4]):
        edges = [0] + sorted(set(cuts)) + [997]
        tp, pk = np.zeros((2, 3), np.uint64), np.zeros((2, 3), np.uint64)
        state = None
        for a, b in zip(edges, edges[1:]):
            rc, tp, pk, state = host(np.ascontiguousarray(x[:, a:b]), coefs, gain=gain, first_frame=a, flush=b == 997, state=state, tp=tp, pk=pk)
            assert rc == RR_OK
        assert np.array_equal(tp, tp1) and np.array_equal(pk, pk1), cuts
        assert np.array_equal(state.view(np.uint64), so1.view(np.uint64)), cuts
    # the model cuts the same way
    mt, mp, ms = M.true_peak(x[:, :400], coefs, gain, flush=False)
    mt2, mp2, ms2 = M.true_peak(x[:, 400:], coefs, gain, flush=True, state=ms)
    assert np.array_equal(np.maximum(mt, mt2), tp1) and np.array_equal(np.maximum(mp, mp2), pk1) and np.array_equal(ms2.view(np.uint64), so1.view(np.uint64))


def test_a_state_is_not_read_at_frame_zero():
    rng = np.random.default_rng(8)
    x = M.planted(rng, (1, 50, 2), np.float32)
    junk = np.full((1, 2, 16), 123.0)
    rc, tp, pk, so = host(x, state=junk)
    rc2, tp2, pk2, so2 = host(x)
    assert rc == RR_OK and rc2 == RR_OK and np.array_equal(tp, tp2) and np.array_equal(pk, pk2) and np.array_equal(so, so2)


def tone(phase):
    n = np.arange(4000)
    return np.sin(2 * np.pi * n / 4 + phase).reshape(1, -1, 1)


def steady(x):
    """the tone's true peak where the filter lies wholly inside it: the first taps - 1 frames only prime the history"""
    rc, _, _, state = host(np.ascontiguousarray(x[:, :11]), flush=False)
    assert rc == RR_OK
    rc, tp, pk, _ = host(np.ascontiguousarray(x[:, 11:]), first_frame=11, flush=False, state=state)
    assert rc == RR_OK
    return float(M.as_double(tp)[0, 0]), float(M.as_double(pk)[0, 0])


def test_the_fs4_tone_between_the_samples():
    """sin(2 pi n / 4 + pi / 4), amplitude 1: every sample is +-0.7071, the peaks of the wave lie between them.  As one whole
    track (from +0.0, flushed) the true peak is 1.0095607: the largest value is at the onset, where the older taps still see
    zeros.  Inside the tone it is 1.0051585, the figure of a tone that has always been there; both lie in (1.0, 1.01)."""
    x = tone(np.pi / 4)
    rc, tp, pk, _ = host(x)
    assert rc == RR_OK
    tp, pk = float(M.as_double(tp)[0, 0]), float(M.as_double(pk)[0, 0])
    print("whole track: true peak %.10f sample peak %.10f" % (tp, pk))
    assert abs(pk - np.sqrt(0.5)) < 1e-9
    assert 1.0 < tp < 1.01
    mt, mp, _ = M.true_peak(x, M.BS1770)
    assert M.as_double(mt)[0, 0] == tp and M.as_double(mp)[0, 0] == pk
    stp, spk = steady(x)
    print("inside the tone: true peak %.10f sample peak %.10f" % (stp, spk))
    assert abs(stp - 1.0051585) < 1e-7 and abs(spk - np.sqrt(0.5)) < 1e-9
    assert 20 * np.log10(stp / spk) > 3.05  # the error of a gain derived from the sample peak, in dB


def test_the_fs4_tone_on_the_samples():
    """The same tone at phase 0: the samples are 0, 1, 0, -1 and the sample peak is 1.0.  Inside the tone the true peak is
    8008 / 8192 = 0.9775390625, BELOW the sample peak -- the centre tap of phase 0 is 7964 / 8192 -- which is why a caller needs
    both numbers.  (As one whole track from +0.0 the onset gives (7964 + 487 - 161 - 14) / 8192 = 1.0102539: the taps that would
    subtract 390 - 122 still see zeros.  That is the arithmetic of the interface applied to a tone that begins abruptly, not a
    property of the tone.)"""
    x = tone(0.0)
    stp, spk = steady(x)
    print("inside the tone: true peak %.10f sample peak %.10f" % (stp, spk))
    assert spk == 1.0
    assert stp < spk
    assert abs(stp - 8008.0 / 8192.0) < 1e-12
    rc, tp, pk, _ = host(x)
    assert rc == RR_OK
    print("whole track: true peak %.10f" % float(M.as_double(tp)[0, 0]))
    assert abs(float(M.as_double(tp)[0, 0]) - 8276.0 / 8192.0) < 1e-12 and float(M.as_double(pk)[0, 0]) == 1.0
