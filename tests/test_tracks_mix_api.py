"""Channel mixing, host side (RRX_mix_device, RRX_tracks_stage_mix_device and its window form, RRX_debug_mix_host,
RRX_debug_tracks_mix_host; DESIGN.md 11, "Channel mixing"): the two hooks -- serial loops over the very per-frame function the
kernels call -- against the numpy model of tests/mix_model.py, bit for bit, the consequences of "zero means not connected", and
every refusal that needs no device.  CPU only."""
import os
import subprocess
import sys

import numpy as np
import pytest

import foo_dsp_resampler_amd as F
import mix_cases as MC
import mix_model as MM

ROOT = MC.ROOT
RR_OK, RR_EXTUNINIT, RR_INVPARAM = 0, 5, 6
NEW = ("RRX_mix_device", "RRX_debug_mix_host", "RRX_tracks_stage_mix_device", "RRX_tracks_stage_mix_window_device",
       "RRX_debug_tracks_mix_host")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def tracks_mix_host(fmt, raw, nch_src, first, count, M):
    M = np.ascontiguousarray(M, np.float64)
    out = np.full((count, M.shape[0]), np.nan, np.float32)
    rc = F.lib().RRX_debug_tracks_mix_host(fmt, raw.ctypes.data, nch_src, first, count, M.shape[0], M.ctypes.data, out.ctypes.data)
    assert rc == RR_OK, rc
    return out


def mix_host(src, M, frames=None, dst_stride=None, fill=0.0):
    """RRX_debug_mix_host on [nstreams, stride, nch_src] rows: the destination rows, pitch dst_stride"""
    M = np.ascontiguousarray(M, np.float64)
    n, stride, nch_src = src.shape
    frames = stride if frames is None else frames
    dst = np.full((n, dst_stride or stride, M.shape[0]), fill, src.dtype)
    fmt = F.RRX_FMT_DOUBLE if src.dtype == np.float64 else F.RRX_FMT_FLOAT
    rc = F.lib().RRX_debug_mix_host(fmt, src.ctypes.data, stride, n, frames, nch_src, dst.ctypes.data, dst.shape[1], M.shape[0], M.ctypes.data)
    assert rc == RR_OK, rc
    return dst


def test_symbols_are_exported_and_listed():
    header = open(os.path.join(ROOT, "include", "ratelib_amd.h")).read()
    for name in NEW:
        assert name in F.EXPECTED_SYMBOLS and name in F.available_symbols()
        assert name in header
    assert "#define RRX_MIX_MAX_CH 16" in header and F.RRX_MIX_MAX_CH == 16
    assert "rounded ONCE, from the exact sum" in header                       # the S32 statement


@pytest.mark.parametrize("pair", MC.PAIRS)
@pytest.mark.parametrize("fmt", MC.FMTS, ids=[MC.FMT_IDS[f] for f in MC.FMTS])
def test_tracks_hook_equals_the_model_bit_for_bit(fmt, pair):
    M = MC.MATRICES[pair]
    nch_src = M.shape[1]
    raw = np.concatenate(MC.tracks(fmt, nch_src, (40, 2300, 3001)))
    want = MM.mix_raw(raw, fmt, M)
    assert np.isfinite(want).all() and np.abs(want).max() > 0.05
    for first in (0, 1, 2, 3):
        got = tracks_mix_host(fmt, raw, nch_src, first, raw.shape[0] - first, M)
        assert np.array_equal(bits(got), bits(want[first:])), (fmt, pair, first)


@pytest.mark.parametrize("pair", MC.PAIRS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_rows_hook_equals_the_model_bit_for_bit(dtype, pair):
    M = MC.MATRICES[pair]
    nch_src = M.shape[1]
    rng = np.random.default_rng(5)
    src = rng.standard_normal((3, 70, nch_src)).astype(dtype)
    src[1, 3, 0] = -0.0
    got = mix_host(src, M, frames=63, dst_stride=75, fill=123.0)
    assert (got[:, 63:] == 123.0).all(), "frames outside [0, frames) were written"
    for s in range(3):
        want = MM.mix(src[s, :63].astype(np.float64), M, dtype)
        assert np.array_equal(bits(got[s, :63]), bits(want)), (pair, s)


@pytest.mark.parametrize("fmt", [F.RRX_FMT_S16, F.RRX_FMT_S24_3, F.RRX_FMT_S32], ids=["s16", "s24", "s32"])
def test_the_identity_gives_the_bits_of_the_load_hook(fmt):
    nch = 3
    raw = np.concatenate(MC.tracks(fmt, nch, (40, 2300, 3001)))
    got = tracks_mix_host(fmt, raw, nch, 0, raw.shape[0], np.eye(nch))
    want = np.full(raw.shape[0] * nch, np.nan, np.float32)
    assert F.lib().RRX_debug_tracks_load_host(fmt, raw.ctypes.data, 0, want.size, want.ctypes.data) == RR_OK
    assert np.array_equal(bits(got).reshape(-1), bits(want))


def test_s32_is_rounded_once_from_the_exact_sum():
    """2^24 + 1 and 1 in two S32 channels at 0.5 each: the exact sum (2^24 + 2) * 2^-32 is a float32; converting to float32 first
    rounds 2^24 + 1 to 2^24 and gives another value"""
    raw = np.array([[2 ** 24 + 1, 1]], np.int32)
    got = tracks_mix_host(F.RRX_FMT_S32, raw, 2, 0, 1, [[0.5, 0.5]])
    assert got[0, 0] == np.float32((2 ** 24 + 2) * 2.0 ** -32)
    first = raw.astype(np.float64) * 2.0 ** -31
    assert np.float32(0.5 * np.float32(first[0, 0]) + 0.5 * np.float32(first[0, 1])) != got[0, 0]


def test_zero_means_not_connected():
    perm = MC.MATRICES["3to3"]
    x = np.array([[-0.0, 0.25, -0.0], [0.0, -0.0, 1.0]], np.float32)
    got = tracks_mix_host(F.RRX_FMT_FLOAT, x, 3, 0, 2, perm)
    assert np.array_equal(bits(got), bits(x[:, [2, 0, 1]]))                   # -0.0 survives a permutation
    assert np.array_equal(bits(mix_host(x[None].astype(np.float64), perm)[0]), bits(x[:, [2, 0, 1]].astype(np.float64)))
    # a NaN and an infinity in the unconnected LFE leave the output finite
    M = F.mix_matrix("5.1_to_stereo")
    src = np.full((2, 6), 0.125, np.float32)
    src[0, 3], src[1, 3] = np.nan, np.inf
    got = tracks_mix_host(F.RRX_FMT_FLOAT, src, 6, 0, 2, M)
    assert np.isfinite(got).all()
    assert np.array_equal(bits(got), bits(MM.mix(src.astype(np.float64), M)))
    assert np.isfinite(mix_host(src[None], M)).all()
    # and reach it when the channel is connected
    M[0, 3] = 0.25
    got = tracks_mix_host(F.RRX_FMT_FLOAT, src, 6, 0, 2, M)
    assert np.isnan(got[0, 0]) and np.isinf(got[1, 0]) and np.isfinite(got[:, 1]).all()
    got = mix_host(src[None], M)[0]
    assert np.isnan(got[0, 0]) and np.isinf(got[1, 0]) and np.isfinite(got[:, 1]).all()
    # a row of zeros gives +0.0, whatever the source holds, and a negative zero is a zero
    M = np.array([[0.0, -0.0], [1.0, 0.0]])
    src = np.array([[-1.0, np.nan], [-0.0, -3.0]], np.float32)
    got = tracks_mix_host(F.RRX_FMT_FLOAT, src, 2, 0, 2, M)
    assert np.array_equal(bits(got[:, 0]), np.zeros(2, np.uint32))
    assert np.array_equal(bits(got[:, 1]), bits(src[:, 0]))
    got = mix_host(src[None].astype(np.float64), M, fill=7.0)[0]
    assert np.array_equal(bits(got[:, 0]), np.zeros(2, np.uint64))


def test_mix_matrices_and_normalize():
    shapes = {"stereo_to_mono": (1, 2), "mono_to_stereo": (2, 1), "swap": (2, 2), "mid_side": (2, 2), "5.1_to_stereo": (2, 6),
              "7.1_to_stereo": (2, 8)}
    assert set(F.MIX_MATRICES) == set(shapes)
    for name, shape in shapes.items():
        m = F.MIX_MATRICES[name]
        assert m.dtype == np.float64 and m.shape == shape and not m.flags.writeable
        assert F.mix_matrix(name).flags.writeable and np.array_equal(F.mix_matrix(name), m)
    assert np.array_equal(F.MIX_MATRICES["stereo_to_mono"], [[0.5, 0.5]])
    h = 0.5 ** 0.5
    assert np.array_equal(F.MIX_MATRICES["5.1_to_stereo"], [[1, 0, h, 0, h, 0], [0, 1, h, 0, 0, h]])   # the LFE is not connected
    assert np.array_equal(F.MIX_MATRICES["7.1_to_stereo"], [[1, 0, h, 0, h, 0, h, 0], [0, 1, h, 0, 0, h, 0, h]])
    for name in ("5.1_to_stereo", "7.1_to_stereo", "mid_side"):
        n = F.mix_matrix(name, normalize=True)
        worst = np.abs(F.MIX_MATRICES[name]).sum(axis=1).max()
        assert np.array_equal(n, F.MIX_MATRICES[name] / max(worst, 1.0))
        assert np.abs(n).sum(axis=1).max() <= 1.0 + 1e-15
    assert np.array_equal(F.mix_matrix([[2.0, -2.0]], normalize=True), [[0.5, -0.5]])
    with pytest.raises(KeyError):
        F.mix_matrix("quad_to_stereo")


def test_hook_refusals_and_inert_without_test_hooks():
    L = F.lib()
    x, out, M = np.zeros((8, 2), np.float32), np.zeros((8, 1), np.float32), np.array([[0.5, 0.5]])
    good = dict(fmt=F.RRX_FMT_FLOAT, src=x.ctypes.data, nch_src=2, first=0, count=8, nch=1, mix=M.ctypes.data, out=out.ctypes.data)

    def tracks_call(**kw):
        a = dict(good, **kw)
        return L.RRX_debug_tracks_mix_host(a["fmt"], a["src"], a["nch_src"], a["first"], a["count"], a["nch"], a["mix"], a["out"])

    assert tracks_call() == RR_OK and tracks_call(count=0) == RR_OK
    bad = np.array([[0.5, np.nan]])
    inf = np.array([[np.inf, 0.5]])
    for kw in (dict(fmt=F.RRX_FMT_DOUBLE), dict(fmt=8), dict(fmt=-1), dict(src=None), dict(out=None), dict(mix=None), dict(nch_src=0),
               dict(nch_src=17), dict(nch=0), dict(nch=17), dict(mix=bad.ctypes.data), dict(mix=inf.ctypes.data)):
        assert tracks_call(**kw) == RR_INVPARAM, kw

    dst = np.zeros((8, 1), np.float32)
    rows = dict(fmt=F.RRX_FMT_FLOAT, src=x.ctypes.data, src_stride=8, nstreams=1, frames=8, nch_src=2, dst=dst.ctypes.data, dst_stride=8,
                nch_dst=1, mix=M.ctypes.data)

    def rows_call(**kw):
        a = dict(rows, **kw)
        return L.RRX_debug_mix_host(a["fmt"], a["src"], a["src_stride"], a["nstreams"], a["frames"], a["nch_src"], a["dst"], a["dst_stride"],
                                    a["nch_dst"], a["mix"])

    assert rows_call() == RR_OK and rows_call(frames=0) == RR_OK
    for kw in (dict(fmt=F.RRX_FMT_S16), dict(fmt=F.RRX_FMT_S24_3), dict(fmt=-1), dict(src=None), dict(dst=None), dict(mix=None),
               dict(nch_src=0), dict(nch_src=17), dict(nch_dst=0), dict(nch_dst=17), dict(mix=bad.ctypes.data), dict(mix=inf.ctypes.data),
               dict(nstreams=0), dict(dst=x.ctypes.data),                                   # d_dst == d_src
               dict(dst=x.ctypes.data + 16), dict(dst=x.ctypes.data - 16),                  # any other overlap
               dict(nstreams=2, src_stride=7), dict(nstreams=2, dst_stride=7), dict(frames=2 ** 60), dict(nstreams=2, src_stride=2 ** 59)):
        assert rows_call(**kw) == RR_INVPARAM, kw
    code = ("import sys; sys.path.insert(0, %r)\nimport foo_dsp_resampler_amd as F\n"
            "print(F.lib().RRX_debug_tracks_mix_host(0, None, 2, 0, 0, 1, None, None), F.lib().RRX_debug_mix_host(0, None, 0, 1, 0, 2, None, 0, 1, None))\n"
            % ROOT)
    env = {k: v for k, v in os.environ.items() if k != "RSMP_TEST_HOOKS"}
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-2:] == ["-1", "-1"]


CHILD = r"""
import sys, ctypes as C
import numpy as np
sys.path.insert(0, %r)
import foo_dsp_resampler_amd as F
L = F.lib()
p = 0x10000  # never dereferenced: every call below is answered from its arguments, or from the library's state, alone
M = np.array([[1.0, 0.0, 0.7, 0.0, 0.7, 0.0], [0.0, 1.0, 0.7, 0.0, 0.0, 0.7]])
nan = M.copy(); nan[1, 3] = np.nan
inf = M.copy(); inf[0, 0] = -np.inf
good = dict(device=-1, stream=None, fs=44100, fo=48000, table=p, ntracks=3, fmt=24, nch_src=6, packed=p, src_total=1000, nch=2,
            mix=M.ctypes.data, rows=p, row_frames=4096, win_first=0, win_frames=100, win_stride=100)
def stage(**kw):
    a = dict(good, **kw)
    return L.RRX_tracks_stage_mix_device(a["device"], a["stream"], a["fs"], a["fo"], a["table"], a["ntracks"], a["fmt"], a["nch_src"],
                                         a["packed"], a["src_total"], a["nch"], a["mix"], a["rows"], a["row_frames"])
def window(**kw):
    a = dict(good, **kw)
    return L.RRX_tracks_stage_mix_window_device(a["device"], a["stream"], a["fs"], a["fo"], a["table"], a["ntracks"], a["fmt"], a["nch_src"],
                                                a["packed"], a["src_total"], a["nch"], a["mix"], a["row_frames"], a["win_first"],
                                                a["win_frames"], a["rows"], a["win_stride"])
shared = [("mix", dict(mix=None)), ("nan", dict(mix=nan.ctypes.data)), ("inf", dict(mix=inf.ctypes.data)), ("nch_src0", dict(nch_src=0)),
          ("nch_src17", dict(nch_src=17)), ("nch0", dict(nch=0)), ("nch17", dict(nch=17)), ("double", dict(fmt=1)), ("fmt8", dict(fmt=8)),
          ("fmt-1", dict(fmt=-1)), ("table", dict(table=None)), ("packed", dict(packed=None)), ("rows", dict(rows=None)),
          ("ntracks0", dict(ntracks=0)), ("fs0", dict(fs=0)), ("fo0", dict(fo=0)), ("row_frames0", dict(row_frames=0)),
          ("device-2", dict(device=-2)), ("channels2^30", dict(ntracks=2**29)), ("src2^60", dict(src_total=2**58)),
          ("rows2^60", dict(row_frames=2**58))]
for name, kw in shared:
    print("inv", "stage-" + name, stage(**kw))
    print("inv", "window-" + name, window(**kw))
for name, kw in [("past", dict(win_first=4000, win_frames=97)), ("wrap", dict(win_first=2**64 - 1, win_frames=2)), ("stride", dict(win_stride=99)),
                 ("stride2^60", dict(win_stride=2**59))]:
    print("inv", "window-" + name, window(**kw))
for fmt in (0, 16, 24, 32):
    print("ok", "stage", fmt, stage(fmt=fmt))
    print("ok", "window", fmt, window(fmt=fmt))
print("ok", "src-below-2^60", stage(src_total=(2**60 - 1) // 6, ntracks=1))  # (the bound counts nch_src channels)
rows = dict(device=-1, stream=None, fmt=0, src=p, src_stride=100, nstreams=2, frames=100, nch_src=6, dst=p + 2**20, dst_stride=100, nch_dst=2,
            mix=M.ctypes.data)
def mix(**kw):
    a = dict(rows, **kw)
    return L.RRX_mix_device(a["device"], a["stream"], a["fmt"], a["src"], a["src_stride"], a["nstreams"], a["frames"], a["nch_src"], a["dst"],
                            a["dst_stride"], a["nch_dst"], a["mix"])
for name, kw in [("mix", dict(mix=None)), ("nan", dict(mix=nan.ctypes.data)), ("inf", dict(mix=inf.ctypes.data)), ("nch_src0", dict(nch_src=0)),
                 ("nch_src17", dict(nch_src=17)), ("nch_dst0", dict(nch_dst=0)), ("nch_dst17", dict(nch_dst=17)), ("s16", dict(fmt=16)),
                 ("s24", dict(fmt=24)), ("s32", dict(fmt=32)), ("fmt-1", dict(fmt=-1)), ("src", dict(src=None)), ("dst", dict(dst=None)),
                 ("same", dict(dst=p)), ("overlap", dict(dst=p + 4000)), ("overlap-below", dict(dst=p - 1000)), ("nstreams0", dict(nstreams=0)),
                 ("src_stride", dict(src_stride=99)), ("dst_stride", dict(dst_stride=99)), ("frames2^60", dict(frames=2**60, nstreams=1)),
                 ("device-2", dict(device=-2))]:
    print("inv", "rows-" + name, mix(**kw))
for name, kw in [("float", dict()), ("double", dict(fmt=1)), ("adjacent", dict(dst=p + 199 * 6 * 4 + 6 * 4)), ("empty", dict(frames=0))]:
    print("ok", "rows", name, mix(**kw))
"""


def test_device_calls_refuse_from_their_arguments_alone():
    """RR_INVPARAM comes before RR_EXTUNINIT: in a process that never called init_ratelib (and sees no device) every refusal is
    answered from the arguments, and only a call with nothing to refuse gets as far as RR_EXTUNINIT -- an empty call included."""
    out = subprocess.run([sys.executable, "-c", CHILD % ROOT], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))
    assert out.returncode == 0, out.stderr
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.split() and ln.split()[0] in ("inv", "ok")]
    inv = [ln for ln in lines if ln[0] == "inv"]
    assert len(inv) == 2 * 21 + 4 + 21 and all(int(ln[-1]) == RR_INVPARAM for ln in inv), [ln for ln in inv if int(ln[-1]) != RR_INVPARAM]
    ok = [ln for ln in lines if ln[0] == "ok"]
    assert len(ok) == 8 + 1 + 4 and all(int(ln[-1]) == RR_EXTUNINIT for ln in ok), ok


def test_python_refusals_that_need_no_device():
    with pytest.raises(ValueError):
        F.ratelib._mix_checked("quad_to_stereo")
    with pytest.raises(ValueError):
        F.ratelib._mix_checked(np.zeros((2, 17)))
    with pytest.raises(ValueError):
        F.ratelib._mix_checked(np.zeros((0, 2)))
    with pytest.raises(ValueError):
        F.ratelib._mix_checked([[0.5, np.inf]])
    with pytest.raises(ValueError):
        F.ratelib._mix_checked("5.1_to_stereo", nch_src=2)
    with pytest.raises(ValueError):
        F.ratelib._mix_checked("5.1_to_stereo", nch_dst=1)
    m = F.ratelib._mix_checked("5.1_to_stereo", nch_src=6, nch_dst=2)
    assert m.dtype == np.float64 and m.flags.c_contiguous and m.shape == (2, 6)
