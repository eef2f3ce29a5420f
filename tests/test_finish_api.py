"""The output stage's host side (RRX_finish_device / RRX_debug_finish_host): the symbols, the refusals that need no device, and
the per-sample arithmetic -- the host twin is a serial loop over the very function the kernel calls -- against the numpy
restatement in finish_model.py, bit for bit.  CPU only."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import foo_dsp_resampler_amd as F
import finish_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RR_OK, RR_EXTUNINIT, RR_INVPARAM = 0, 5, 6
SEED = 0x1234567887654321


def test_symbols_are_exported_and_listed():
    header = open(os.path.join(ROOT, "include", "ratelib_amd.h")).read()
    for name in ("RRX_finish_device", "RRX_debug_finish_host"):
        assert name in F.EXPECTED_SYMBOLS and name in F.available_symbols()
        assert name in header
    assert "#define RRX_FMT_S24_3 24" in header and F.RRX_FMT_S24_3 == 24
    assert callable(F.finish_device) and hasattr(F.Resampler, "convert_track_to_pcm_device")


def test_packed_24_bit_is_no_handle_format():
    cfg = F.RRConfig(44100, 48000, 50.0, 95.0, 0, F.RR_BEST)
    h = C.c_void_p()
    assert F.lib().RRX_open_batch_fmt(C.byref(cfg), 2, 1, -1, F.RRX_FMT_S24_3, C.byref(h)) == RR_INVPARAM
    assert not h


CHILD = r"""
import sys, ctypes as C
sys.path.insert(0, %r)
import foo_dsp_resampler_amd as F
L = F.lib()
cb = F.ratelib._ALLOC_CB(lambda: None)
fn = L.RRX_finish_device
p = 0x10000  # never dereferenced: every call below is answered from its arguments, or from the library's state, alone
good = dict(device=-1, stream=None, sf=0, src=p, ss=4096, df=16, dst=p, ds=4096, nstreams=2, frames=1024, nch=2, gain=None, dither=1,
            seed=7, first=0, peak=p, clipped=p)
def call(**kw):
    a = dict(good, **kw)
    return fn(a["device"], a["stream"], a["sf"], a["src"], a["ss"], a["df"], a["dst"], a["ds"], a["nstreams"], a["frames"], a["nch"],
              a["gain"], a["dither"], a["seed"], a["first"], a["peak"], a["clipped"])
print("uninit", call())                                   # before init_ratelib
print("init", L.init_ratelib(cb))                         # no device: refuses
print("uninit", call(), call(frames=0))
for name, kw in [("null", dict(src=None)), ("nstreams0", dict(nstreams=0)), ("nstreams-1", dict(nstreams=-1)), ("nch0", dict(nch=0)),
                 ("nch-1", dict(nch=-1)), ("srcfmt16", dict(sf=16)), ("srcfmt7", dict(sf=7)), ("dstfmt0", dict(df=0)), ("dstfmt1", dict(df=1)),
                 ("dstfmt8", dict(df=8)), ("sstride", dict(ss=1023)), ("dstride", dict(ds=1023)), ("sstride0", dict(ss=0)),
                 ("nothing", dict(dst=None, peak=None, clipped=None)), ("wrap", dict(first=2**64 - 1024)),
                 ("wrap1", dict(first=2**64 - 1, frames=1, ss=1, ds=1)),
                 ("samples2^60", dict(frames=2**59, ss=2**59, ds=2**59)), ("srcrows2^60", dict(ss=2**58)), ("dstrows2^60", dict(ds=2**58)),
                 ("device-2", dict(device=-2))]:
    print("inv", name, call(**kw))
for name, kw in [("one-stream", dict(nstreams=1, ss=0, ds=0)), ("tight", dict(ss=1024, ds=1024)), ("s24", dict(df=24)), ("s32", dict(df=32)),
                 ("double", dict(sf=1)), ("measure", dict(dst=None, df=0, ds=0)), ("peak-only", dict(dst=None, clipped=None)),
                 ("no-stats", dict(peak=None, clipped=None)), ("last-frame", dict(first=2**64 - 1025)),
                 ("rows-below-2^60", dict(ss=2**58 - 1, ds=2**58 - 1)), ("dstride-unused", dict(dst=None, ds=2**63))]:
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
    inv = [ln for ln in lines if ln[0] == "inv"]
    assert len(inv) == 20 and all(int(ln[2]) == RR_INVPARAM for ln in inv), inv
    ok = [ln for ln in lines if ln[0] == "ok"]
    assert len(ok) == 11 and all(int(ln[2]) == RR_EXTUNINIT for ln in ok), ok


def test_host_twin_refuses_as_the_device_call_does_and_is_inert_without_test_hooks():
    x = np.zeros((2, 8, 2), np.float32)
    fn = F.lib().RRX_debug_finish_host
    pk = np.zeros(4, np.uint64)
    args = lambda **kw: [kw.get("sf", 0), kw.get("src", x.ctypes.data), kw.get("ss", 8), 16, None, 8, kw.get("ns", 2), 8, kw.get("nch", 2), None, 0,
                         0, kw.get("first", 0), kw.get("peak", pk.ctypes.data), None]
    assert fn(*args()) == RR_OK
    for kw in (dict(src=None), dict(ns=0), dict(nch=0), dict(sf=16), dict(ss=7), dict(peak=None), dict(first=2 ** 64 - 4), dict(ss=2 ** 58)):
        assert fn(*args(**kw)) == RR_INVPARAM, kw
    code = ("import sys; sys.path.insert(0, %r)\nimport foo_dsp_resampler_amd as F\n"
            "print(F.lib().RRX_debug_finish_host(0, None, 0, 16, None, 0, 1, 0, 1, None, 0, 0, 0, None, None))\n" % ROOT)
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
        F.finish_device(Fake((100,)), F.RRX_FMT_S16)
    with pytest.raises(ValueError):
        F.finish_device(Fake((100, 2), contiguous=False), F.RRX_FMT_S16)
    with pytest.raises(TypeError):
        F.finish_device(Fake((100, 2), dtype="torch.int16"), F.RRX_FMT_S16)
    with pytest.raises(ValueError):
        F.finish_device(Fake((100, 2)), 8)
    with pytest.raises(ValueError):
        F.finish_device(Fake((100, 2)), F.RRX_FMT_S16, first_frame=2 ** 64 - 50)
    with pytest.raises(TypeError):
        F.finish_device(Fake((100, 2)), F.RRX_FMT_S16)                  # not a device tensor


@pytest.mark.parametrize("frames", M.FRAMES)
@pytest.mark.parametrize("nstreams,nch", M.SHAPES)
def test_host_twin_equals_the_model_bit_for_bit(nstreams, nch, frames):
    for fmt in M.FORMATS:
        for double in (False, True):
            for gain in M.GAINS:
                for dith in (False, True):
                    x, g, want = M.case(nstreams, frames, nch, fmt, double, gain, dith, SEED)
                    got = M.host(x, fmt, g, dith, SEED)
                    for k, what in enumerate(("output bytes", "peak bit patterns", "clip counts")):
                        assert np.array_equal(got[k], want[k]), (what, fmt, double, gain, dith)
    x = M.make_input(nstreams, frames, nch, F.RRX_FMT_S32, False)
    if frames == 4099:  # the planted values did their work
        _, pk, cl = M.case(nstreams, frames, nch, F.RRX_FMT_S32, False, None, False, SEED)[2]
        nanch = M.nan_channels(x)
        assert nanch.sum() == 1 and np.isnan(pk.view(np.float64)[nanch]).all()
        assert nstreams * nch == 1 or pk.view(np.float64)[~nanch].max() == np.inf
        assert cl.sum() >= 5 * nstreams           # +1.0, +-3.0, +-inf at the least


@pytest.mark.parametrize("fmt,dtype", [(F.RRX_FMT_S16, "<i2"), (F.RRX_FMT_S32, "<i4")])
def test_without_gain_and_dither_it_is_the_integer_handles_rule(fmt, dtype):
    """round half to even, saturate in fp64, narrow: ratelib_amd.h's rule for RRX_FMT_S16 / RRX_FMT_S32 handles, stated on its own"""
    bits = M.BITS[fmt]
    for double in (False, True):
        x = M.make_input(2, 4099, 3, fmt, double)
        with np.errstate(invalid="ignore"):
            q = np.clip(np.rint(x.astype(np.float64) * 2.0 ** bits), -2.0 ** bits, 2.0 ** bits - 1)
        q[np.isnan(q)] = -2.0 ** bits
        want = q.astype(np.int64).astype(dtype)
        got = M.host(x, fmt)[0].view(dtype)
        assert np.array_equal(got, want)


@pytest.mark.parametrize("fmt", M.FORMATS)
def test_dither_is_deterministic_and_chunk_invariant(fmt):
    x = M.make_input(3, 4099, 3, fmt, False)
    g = np.array([0.5, 1.0, 1.7])
    whole = M.host(x, fmt, g, True, SEED, 0)
    again = M.host(x, fmt, g, True, SEED, 0)
    assert all(np.array_equal(a, b) for a, b in zip(whole, again))
    o1, pk, cl = M.host(np.ascontiguousarray(x[:, :1001]), fmt, g, True, SEED, 0)
    o2, pk, cl = M.host(np.ascontiguousarray(x[:, 1001:]), fmt, g, True, SEED, 1001, peak=pk, clipped=cl)
    assert np.array_equal(np.concatenate([o1, o2], axis=1), whole[0])
    assert np.array_equal(pk, whole[1]) and np.array_equal(cl, whole[2])
    # measure only: no destination, the same peak; the clip count is the S32 quantiser's
    measured = M.host(x, fmt, g, True, SEED, 0, write=False)
    assert measured[0] is None and np.array_equal(measured[1], whole[1])
    if fmt == F.RRX_FMT_S32:
        assert np.array_equal(measured[2], whole[2])
    assert not np.array_equal(M.host(x, fmt, g, True, SEED, 1)[0], whole[0])


def test_seeds_and_channels_get_different_noise():
    x = np.full((2, 4096, 2), 0.25 + 2.0 ** -17, np.float32)     # identical input in every stream and channel, a quarter of an S16 LSB off the grid
    a = M.host(x, F.RRX_FMT_S16, None, True, 1)[0].view("<i2")
    b = M.host(x, F.RRX_FMT_S16, None, True, 2)[0].view("<i2")
    assert not np.array_equal(a, b)
    chans = a.reshape(2, 4096, 2)
    seqs = [chans[s, :, c] for s in range(2) for c in range(2)]
    for i in range(4):
        for j in range(i + 1, 4):
            assert np.mean(seqs[i] != seqs[j]) > 0.3, (i, j)
    assert set(np.unique(a)) <= {8191, 8192, 8193}


def test_dither_statistics():
    """mean 0 and variance 1/6 LSB^2 of a triangular density on (-1, 1); its kurtosis is 2.4, so the variance of 2^20 samples has a
    standard error of sqrt(1.4 / 2^20) = 0.12 % and 1 % is eight of them; the mean's is sqrt(1 / (6 * 2^20)), of which 5 are allowed"""
    n = 1 << 20
    d = M.dither(SEED, 1000, n, 2, 3)[1, :, 2]
    assert d.min() > -1 and d.max() < 1
    assert abs(d.mean()) <= 5 / np.sqrt(6 * n)
    assert abs(d.var() - 1 / 6) <= 0.01 / 6
    # the host twin adds exactly these values: silence * 2^bits + d, rounded
    q = M.host(np.zeros((2, 4096, 3), np.float32), F.RRX_FMT_S32, None, True, SEED, 1000)[0].view("<i4").reshape(2, 4096, 3)
    assert np.array_equal(q[1, :, 2], np.rint(d[:4096]).astype(np.int32))


@pytest.mark.parametrize("fmt", M.FORMATS)
def test_dithered_silence_is_minus_one_zero_plus_one(fmt):
    out, pk, cl = M.host(np.zeros((1, 20000, 2), np.float32), fmt, np.array([1.7]), True, SEED)
    b = out.reshape(1, 20000, 2, M.NBYTES[fmt]).astype(np.int64)
    q = sum(b[..., k] << (8 * k) for k in range(M.NBYTES[fmt]))
    q = np.where(q >= 1 << (8 * M.NBYTES[fmt] - 1), q - (1 << (8 * M.NBYTES[fmt])), q)
    assert set(np.unique(q)) == {-1, 0, 1}
    assert not pk.any() and not cl.any()
