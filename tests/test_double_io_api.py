"""Float64 sample format of the C ABI (RRX_open_batch_fmt, RRX_*_double): what can be checked without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import foo_dsp_resampler_amd as F
from foo_dsp_resampler_amd import ratelib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RR_NULLHANDLE, RR_INVPARAM = 3, 6
NEW = ["RRX_open_batch_fmt", "RRX_format", "RRX_push_double", "RRX_pull_double", "RRX_flow_double", "RRX_push_device_double",
       "RRX_pull_device_double", "RRX_flow_device_double"]


def test_new_symbols_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "ratelib_amd.h")).read()
    declared = set(re.findall(r"\b(RRX_[A-Za-z_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, name
        assert name in F.EXPECTED_SYMBOLS, name
        assert hasattr(F.lib(), name), name
    assert "#define RRX_FMT_FLOAT  0" in hdr and "#define RRX_FMT_DOUBLE 1" in hdr
    assert (F.RRX_FMT_FLOAT, F.RRX_FMT_DOUBLE) == (0, 1)


@pytest.mark.parametrize("fmt", [2, -1, 7])
def test_unknown_format_is_invparam_before_any_device(fmt):
    L = F.lib()
    cfg = ratelib._config(44100, 48000)
    h = C.c_void_p(1234)
    assert L.RRX_open_batch_fmt(C.byref(cfg), 2, 1, -1, fmt, C.byref(h)) == RR_INVPARAM
    assert not h.value
    assert L.RRX_open_batch_fmt(C.byref(cfg), 2, 1, 0, fmt, C.byref(h)) == RR_INVPARAM


def test_double_calls_on_null_handle():
    L = F.lib()
    n, m = C.c_size_t(0), C.c_size_t(0)
    buf = (C.c_double * 16)()
    assert L.RRX_format(None) == -1
    assert L.RRX_push_double(None, buf, 4, 4) == RR_NULLHANDLE
    assert L.RRX_pull_double(None, buf, 4, 4, C.byref(n)) == RR_NULLHANDLE
    assert L.RRX_flow_double(None, buf, 4, buf, 4, 4, 4, C.byref(n), C.byref(m)) == RR_NULLHANDLE
    assert L.RRX_push_device_double(None, buf, 4, 4) == RR_NULLHANDLE
    assert L.RRX_pull_device_double(None, buf, 4, 4, C.byref(n)) == RR_NULLHANDLE
    assert L.RRX_flow_device_double(None, buf, 4, buf, 4, 4, 4, C.byref(n), C.byref(m)) == RR_NULLHANDLE


class _NoC:
    """Stands in for the library: any call into C fails the test."""
    def __getattr__(self, name):
        raise AssertionError("C entry %s called" % name)


def _offline(dtype, nch=2):
    r = object.__new__(F.Resampler)  # no handle, no device: only the Python-side checks run
    r.L, r.h, r.nch, r.nstreams, r.dtype = _NoC(), None, nch, 1, np.dtype(dtype)
    return r


def test_binding_rejects_other_precision_before_c():
    rf = _offline(np.float32)
    with pytest.raises(TypeError):
        rf.push(np.zeros((64, 2), np.float64))
    with pytest.raises(TypeError):
        rf.flow(np.zeros((64, 2), np.float64), 64)
    rd = _offline(np.float64)
    with pytest.raises(TypeError):
        rd.push(np.zeros((64, 2), np.float32))


def test_binding_rejects_tensor_of_other_precision_before_c():
    torch = pytest.importorskip("torch")
    rf, rd = _offline(np.float32), _offline(np.float64)
    with pytest.raises(TypeError):
        rf.push_device(torch.zeros(64, 2, dtype=torch.float64), 64)
    with pytest.raises(TypeError):
        rd.pull_device(torch.zeros(64, 2, dtype=torch.float32), 64)
    with pytest.raises(TypeError):
        rd.flow_device(torch.zeros(64, 2, dtype=torch.float64), 64, torch.zeros(64, 2, dtype=torch.float32), 64)


def test_resampler_refuses_other_dtypes():
    with pytest.raises(TypeError):
        F.Resampler(44100, 48000, dtype=np.int32)
