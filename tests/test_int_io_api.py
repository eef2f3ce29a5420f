"""Integer PCM sample formats of the C ABI (RRX_FMT_S16 / RRX_FMT_S32, RRX_*_samples): what can be checked without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import foo_dsp_resampler_amd as F
from foo_dsp_resampler_amd import ratelib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RR_NULLHANDLE, RR_INVPARAM = 3, 6
NEW = ["RRX_push_samples", "RRX_pull_samples", "RRX_flow_samples", "RRX_push_device_samples", "RRX_pull_device_samples",
       "RRX_flow_device_samples"]


def test_new_symbols_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "ratelib_amd.h")).read()
    declared = set(re.findall(r"\b(RRX_[A-Za-z_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, name
        assert name in F.EXPECTED_SYMBOLS, name
        assert hasattr(F.lib(), name), name
    assert re.search(r"#define RRX_FMT_S16 16\b", hdr) and re.search(r"#define RRX_FMT_S32 32\b", hdr)
    assert (F.RRX_FMT_S16, F.RRX_FMT_S32) == (16, 32)


@pytest.mark.parametrize("fmt", [3, 8, 15, 17, 24, 31, 33, 64])
def test_unknown_format_is_invparam_before_any_device(fmt):
    L = F.lib()
    cfg = ratelib._config(44100, 48000)
    for device in (-1, 0):
        h = C.c_void_p(1234)
        assert L.RRX_open_batch_fmt(C.byref(cfg), 2, 1, device, fmt, C.byref(h)) == RR_INVPARAM
        assert not h.value


@pytest.mark.parametrize("fmt", [F.RRX_FMT_FLOAT, F.RRX_FMT_DOUBLE, 16, 32])
def test_samples_calls_on_null_handle(fmt):
    L = F.lib()
    n, m = C.c_size_t(0), C.c_size_t(0)
    buf = (C.c_double * 16)()
    assert L.RRX_push_samples(None, fmt, buf, 4, 4) == RR_NULLHANDLE
    assert L.RRX_pull_samples(None, fmt, buf, 4, 4, C.byref(n)) == RR_NULLHANDLE
    assert L.RRX_flow_samples(None, fmt, buf, 4, buf, 4, 4, 4, C.byref(n), C.byref(m)) == RR_NULLHANDLE
    assert L.RRX_push_device_samples(None, fmt, buf, 4, 4) == RR_NULLHANDLE
    assert L.RRX_pull_device_samples(None, fmt, buf, 4, 4, C.byref(n)) == RR_NULLHANDLE
    assert L.RRX_flow_device_samples(None, fmt, buf, 4, buf, 4, 4, 4, C.byref(n), C.byref(m)) == RR_NULLHANDLE


class _NoC:
    """Stands in for the library: any call into C fails the test."""
    def __getattr__(self, name):
        raise AssertionError("C entry %s called" % name)


def _offline(dtype, nch=2):
    r = object.__new__(F.Resampler)  # no handle, no device: only the Python-side checks run
    r.L, r.h, r.nch, r.nstreams, r.dtype = _NoC(), None, nch, 1, np.dtype(dtype)
    return r


def test_binding_rejects_other_dtype_before_c():
    r16 = _offline(np.int16)
    assert r16.integer and r16.sample_format == F.RRX_FMT_S16
    with pytest.raises(TypeError):
        r16.push(np.zeros((64, 2), np.int32))
    with pytest.raises(TypeError):
        r16.push(np.zeros((64, 2), np.float32))
    with pytest.raises(TypeError):
        r16.flow(np.zeros((64, 2), np.float32), 64)
    rf = _offline(np.float32)
    with pytest.raises(TypeError):
        rf.push(np.zeros((64, 2), np.int16))
    with pytest.raises(TypeError):
        rf.process(np.zeros((64, 2), np.int16))


def test_binding_rejects_tensor_of_other_dtype_before_c():
    torch = pytest.importorskip("torch")
    r32 = _offline(np.int32)
    assert r32.integer and r32.sample_format == F.RRX_FMT_S32
    with pytest.raises(TypeError):
        r32.push_device(torch.zeros(64, 2, dtype=torch.int16), 64)
    with pytest.raises(TypeError):
        r32.pull_device(torch.zeros(64, 2, dtype=torch.int16), 64)
    with pytest.raises(TypeError):
        r32.flow_device(torch.zeros(64, 2, dtype=torch.int32), 64, torch.zeros(64, 2, dtype=torch.int16), 64)


def test_float_dtype_with_integer_format_is_refused():
    with pytest.raises(TypeError):
        F.Resampler(44100, 48000, dtype=np.float64, sample_format=F.RRX_FMT_S16)
    with pytest.raises(TypeError):
        F.Resampler(44100, 48000, dtype=np.float32, sample_format=F.RRX_FMT_S32)
