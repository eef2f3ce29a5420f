"""Integer PCM sources of the ragged stage pass, host side (RRX_tracks_stage_device_samples / RRX_debug_tracks_load_host;
DESIGN.md 11, "Integer sources"): the conversion -- the host hook is a serial loop over the very per-sample function the kernels
call -- against numpy, bit for bit, and every refusal that needs no device.  CPU only.

The model is numpy's alone: (s.astype(float64) * 2.0 ** -bits).astype(float32), one rounding to nearest even, with packed S24
unpacked and sign-extended in numpy."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import foo_dsp_resampler_amd as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RR_OK, RR_EXTUNINIT, RR_INVPARAM = 0, 5, 6
BITS = {F.RRX_FMT_S16: 15, F.RRX_FMT_S24_3: 23, F.RRX_FMT_S32: 31}
NEW = ("RRX_tracks_stage_device_samples", "RRX_debug_tracks_load_host")


def lcg(n, seed):
    """n 32-bit words of the LCG of tests/oracle_binding.py (s = s * 1664525 + 1013904223 mod 2^32)"""
    out, s = np.empty(n, np.uint32), seed & 0xffffffff
    for i in range(n):
        s = (s * 1664525 + 1013904223) & 0xffffffff
        out[i] = s
    return out


def s24_bytes(v):
    """int values in [-2^23, 2^23) -> packed little-endian three-byte samples (uint8 [n * 3])"""
    u = (np.asarray(v, np.int64) & 0xffffff).astype(np.uint32)
    return np.stack([u & 0xff, (u >> 8) & 0xff, u >> 16], axis=-1).astype(np.uint8).reshape(-1)


def s24_values(raw):
    """packed three-byte samples -> int32, sign-extended"""
    b = raw.reshape(-1, 3).astype(np.int32)
    v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
    return np.where(v >= 1 << 23, v - (1 << 24), v).astype(np.int32)


def source(fmt):
    """(raw host buffer as the call takes it, the integer value of every sample): 4096 LCG samples with the extremes planted"""
    w = lcg(4096, 1000 + fmt)
    if fmt == F.RRX_FMT_S16:
        v = (w >> 16).astype(np.uint16).view(np.int16).copy()
        v[[5, 6, 4095]] = [-2 ** 15, 2 ** 15 - 1, -2 ** 15]
        return v, v.astype(np.int64)
    if fmt == F.RRX_FMT_S24_3:
        raw = s24_bytes((w >> 8).astype(np.int64) - (1 << 23))
        raw[15:18] = (0x00, 0x00, 0x80)                      # -2^23
        raw[18:21] = (0xff, 0xff, 0x7f)                      # 2^23 - 1
        raw[21:24] = (0xff, 0xff, 0xff)                      # -1
        raw[-3:] = (0x00, 0x00, 0x80)
        return raw, s24_values(raw).astype(np.int64)
    v = w.view(np.int32).copy()
    v[[5, 6, 7, 8, 9, 4095]] = [-2 ** 31, 2 ** 31 - 1, 2 ** 24 + 1, 2 ** 24 + 3, 2 ** 25 + 2, -2 ** 31]
    return v, v.astype(np.int64)


def model(values, fmt):
    return (values.astype(np.float64) * 2.0 ** -BITS[fmt]).astype(np.float32)


def load_host(fmt, raw, first, count):
    out = np.full(count, np.nan, np.float32)
    rc = F.lib().RRX_debug_tracks_load_host(fmt, raw.ctypes.data, first, count, out.ctypes.data)
    assert rc == RR_OK, rc
    return out


def test_symbols_are_exported_and_listed():
    header = open(os.path.join(ROOT, "include", "ratelib_amd.h")).read()
    for name in NEW:
        assert name in F.EXPECTED_SYMBOLS and name in F.available_symbols()
        assert name in header
    assert "a source format of RRX_tracks_stage_device_samples" in header


@pytest.mark.parametrize("fmt", sorted(BITS), ids=["s16", "s24", "s32"])
def test_load_hook_equals_numpy_bit_for_bit(fmt):
    raw, values = source(fmt)
    want = model(values, fmt)
    for first in (0, 1, 2, 3):
        got = load_host(fmt, raw, first, 4096 - first)
        assert np.array_equal(got.view(np.uint32), want[first:].view(np.uint32)), (fmt, first)
    assert np.abs(want).max() <= 1.0


def test_planted_values_are_what_the_abi_says():
    raw, _ = source(F.RRX_FMT_S16)
    assert list(load_host(F.RRX_FMT_S16, raw, 5, 2)) == [-1.0, np.float32(32767 / 32768)]
    raw, _ = source(F.RRX_FMT_S24_3)
    assert list(load_host(F.RRX_FMT_S24_3, raw, 5, 3)) == [-1.0, np.float32((2 ** 23 - 1) / 2 ** 23), np.float32(-2.0 ** -23)]
    raw, _ = source(F.RRX_FMT_S32)
    got = load_host(F.RRX_FMT_S32, raw, 5, 5)
    # INT32_MAX rounds up to 1.0f; 2^24 + 1 and 2^24 + 3 are ties between neighbours 2 apart and go to the even one; 2^25 + 2 is a tie too
    assert list(got) == [-1.0, 1.0, np.float32(2.0 ** -7), np.float32((2 ** 24 + 4) * 2.0 ** -31), np.float32(2.0 ** -6)]
    # the float source passes through untouched, NaN payloads included
    x = np.array([0.25, -0.0, np.inf], np.float32)
    x = np.concatenate([x, np.array([0x7fc01234], np.uint32).view(np.float32)])
    assert np.array_equal(load_host(F.RRX_FMT_FLOAT, x, 0, 4).view(np.uint32), x.view(np.uint32))


def test_load_hook_refusals_and_inert_without_test_hooks():
    fn = F.lib().RRX_debug_tracks_load_host
    x, out = np.zeros(8, np.int16), np.zeros(8, np.float32)
    assert fn(F.RRX_FMT_S16, x.ctypes.data, 0, 8, out.ctypes.data) == RR_OK
    assert fn(F.RRX_FMT_S16, x.ctypes.data, 0, 0, out.ctypes.data) == RR_OK
    for fmt in (F.RRX_FMT_DOUBLE, 8, 7, -1, 48):
        assert fn(fmt, x.ctypes.data, 0, 8, out.ctypes.data) == RR_INVPARAM, fmt
    assert fn(F.RRX_FMT_S16, None, 0, 8, out.ctypes.data) == RR_INVPARAM
    assert fn(F.RRX_FMT_S16, x.ctypes.data, 0, 8, None) == RR_INVPARAM
    code = ("import sys; sys.path.insert(0, %r)\nimport foo_dsp_resampler_amd as F\n"
            "print(F.lib().RRX_debug_tracks_load_host(16, None, 0, 0, None))\n" % ROOT)
    env = {k: v for k, v in os.environ.items() if k != "RSMP_TEST_HOOKS"}
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-1] == "-1"


CHILD = r"""
import sys, ctypes as C
sys.path.insert(0, %r)
import foo_dsp_resampler_amd as F
L = F.lib()
fn = L.RRX_tracks_stage_device_samples
p = 0x10000  # never dereferenced: every call below is answered from its arguments, or from the library's state, alone
good = dict(device=-1, stream=None, fs=44100, fo=48000, table=p, ntracks=3, nch=2, fmt=16, packed=p, src_total=1000, rows=p, row_frames=4096)
def call(**kw):
    a = dict(good, **kw)
    return fn(a["device"], a["stream"], a["fs"], a["fo"], a["table"], a["ntracks"], a["nch"], a["fmt"], a["packed"], a["src_total"],
              a["rows"], a["row_frames"])
for name, kw in [("fmt8", dict(fmt=8)), ("fmt7", dict(fmt=7)), ("fmt-1", dict(fmt=-1)), ("fmt48", dict(fmt=48)), ("double", dict(fmt=1)),
                 ("table", dict(table=None)), ("packed", dict(packed=None)), ("rows", dict(rows=None)), ("ntracks0", dict(ntracks=0)),
                 ("ntracks-1", dict(ntracks=-1)), ("nch0", dict(nch=0)), ("fs0", dict(fs=0)), ("fo0", dict(fo=0)),
                 ("row_frames0", dict(row_frames=0)), ("device-2", dict(device=-2)), ("channels2^30", dict(ntracks=2**29, nch=2)),
                 ("src2^60", dict(src_total=2**59)), ("rows2^60", dict(row_frames=2**58)),
                 ("s24-src2^60", dict(fmt=24, src_total=2**59)), ("s32-rows2^60", dict(fmt=32, row_frames=2**58))]:
    print("inv", name, call(**kw))
for name, kw in [("s16", dict()), ("s24", dict(fmt=24)), ("s32", dict(fmt=32)), ("float", dict(fmt=0)),
                 ("below-2^60", dict(src_total=2**59 - 1, ntracks=1, row_frames=2**59 - 1))]:
    print("ok", name, call(**kw))                          # nothing to refuse: answered RR_EXTUNINIT before init_ratelib
print("float-call", L.RRX_tracks_stage_device(-1, None, 44100, 48000, p, 3, 2, p, 1000, p, 4096))
"""


def test_stage_samples_refuses_from_its_arguments_alone():
    """RR_INVPARAM comes before RR_EXTUNINIT: in a process that never called init_ratelib (and sees no device) every refusal is
    answered from the arguments, and only a call with nothing to refuse gets as far as RR_EXTUNINIT."""
    out = subprocess.run([sys.executable, "-c", CHILD % ROOT], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))
    assert out.returncode == 0, out.stderr
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.split() and ln.split()[0] in ("inv", "ok", "float-call")]
    inv = [ln for ln in lines if ln[0] == "inv"]
    assert len(inv) == 20 and all(int(ln[2]) == RR_INVPARAM for ln in inv), inv
    ok = [ln for ln in lines if ln[0] == "ok"]
    assert len(ok) == 5 and all(int(ln[2]) == RR_EXTUNINIT for ln in ok), ok
    assert ["float-call", str(RR_EXTUNINIT)] in lines


def test_packed_24_bit_is_still_no_handle_format():
    cfg = F.RRConfig(44100, 48000, 50.0, 95.0, 0, F.RR_BEST)
    h = C.c_void_p()
    assert F.lib().RRX_open_batch_fmt(C.byref(cfg), 2, 1, -1, F.RRX_FMT_S24_3, C.byref(h)) == RR_INVPARAM
    assert not h
