"""The device LPC edge extrapolator's host side: RRX_lpc_extrapolate_device / RRX_edge_geometry are exported, the edge geometry
is the plugin's (dsp_rate::reinit, foo_dsp_rate.cpp:96-101 with samples_len of util.h:38-48), and everything that can be refused
from the arguments alone is refused without a device.  CPU only."""
import ctypes as C
import math
import os
import subprocess
import sys

import pytest

import foo_dsp_resampler_amd as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RR_OK, RR_EXTUNINIT, RR_INVPARAM = 0, 5, 6


def test_symbols_are_exported_and_listed():
    for name in ("RRX_lpc_extrapolate_device", "RRX_edge_geometry"):
        assert name in F.EXPECTED_SYMBOLS and name in F.available_symbols()
        assert name in open(os.path.join(ROOT, "include", "ratelib_amd.h")).read()
    assert callable(F.lpc_extrapolate_device) and callable(F.edge_geometry)
    assert hasattr(F.Resampler, "convert_track_device")


def samples_len(r1, r2, N=20, M=8192):
    """util.h:38-48"""
    v = math.gcd(r1, r2)
    r1, r2 = r1 // v, r2 // v
    n = (v + N - 1) // N
    z = max(r1, r2)
    if z * n > M:
        n = M // z
    n = max(n, 1)
    return r1 * n, r2 * n


def test_edge_geometry_of_the_plugin_example():
    assert F.edge_geometry(44100, 48000) == (2205, 2400, 2205, 4410)   # util.h:38 walks through this pair


@pytest.mark.parametrize("fs,fo", [(44100, 48000), (44100, 96000), (96000, 44100), (8000, 192000), (192000, 8000)])
def test_edge_geometry_matches_samples_len(fs, fo):
    n_add, n_drop, prime, inbuf = F.edge_geometry(fs, fo)
    assert (n_add, n_drop) == samples_len(fs, fo)
    assert n_add * fo == n_drop * fs                                   # the same duration at both rates
    assert prime == max(min(max(fs // 20, 1024), 16384), 65)
    assert inbuf == min(max(fs // 10, 2048), 65536)


def test_edge_geometry_refuses_zero_rates_and_null_outputs():
    L = F.lib()
    v = [C.c_size_t(7) for _ in range(4)]
    refs = [C.byref(x) for x in v]
    assert L.RRX_edge_geometry(44100, 48000, *refs) == RR_OK
    assert L.RRX_edge_geometry(0, 48000, *refs) == RR_INVPARAM
    assert L.RRX_edge_geometry(44100, 0, *refs) == RR_INVPARAM
    for k in range(4):
        args = list(refs)
        args[k] = None
        assert L.RRX_edge_geometry(44100, 48000, *args) == RR_INVPARAM
    with pytest.raises(F.RRError):
        F.edge_geometry(0, 48000)


CHILD = r"""
import sys, ctypes as C
sys.path.insert(0, %r)
import foo_dsp_resampler_amd as F
L = F.lib()
cb = F.ratelib._ALLOC_CB(lambda: None)
fn = L.RRX_lpc_extrapolate_device
p = 0x10000  # never dereferenced: every call below is answered from its arguments, or from the library's state, alone
#            device stream data stride nstreams data_len nch order bkwd fwd
good = dict(device=-1, stream=None, data=p, stride=4096, nstreams=2, data_len=1024, nch=2, order=32, bk=512, fw=512)
def call(**kw):
    a = dict(good, **kw)
    return fn(a["device"], a["stream"], a["data"], a["stride"], a["nstreams"], a["data_len"], a["nch"], a["order"], a["bk"], a["fw"])
print("uninit", call())                                   # before init_ratelib
print("init", L.init_ratelib(cb))                         # no device: refuses
print("uninit", call(), call(bk=0, fw=0))
for name, kw in [("null", dict(data=None)), ("nstreams0", dict(nstreams=0)), ("nstreams-1", dict(nstreams=-1)), ("nch0", dict(nch=0)),
                 ("order0", dict(order=0)), ("order33", dict(order=33)), ("order-1", dict(order=-1)),
                 ("len=order", dict(data_len=32)), ("len<order", dict(data_len=5)), ("len0", dict(data_len=0)),
                 ("stride", dict(stride=2047)), ("stride0", dict(stride=0))]:
    print("inv", name, call(**kw))
print("ok1", call(nstreams=1, stride=0))                  # one stream: the stride is not looked at (answered RR_EXTUNINIT here)
print("ok2", call(stride=2048))
"""


def test_invalid_parameters_are_refused_without_a_device():
    out = subprocess.run([sys.executable, "-c", CHILD % ROOT], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))
    assert out.returncode == 0, out.stderr
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.split() and ln.split()[0] in ("uninit", "init", "inv", "ok1", "ok2")]
    assert ["init", "-1"] in lines
    uninit = [ln for ln in lines if ln[0] == "uninit"]
    assert len(uninit) == 2 and all(int(v) == RR_EXTUNINIT for ln in uninit for v in ln[1:])
    inv = [ln for ln in lines if ln[0] == "inv"]
    assert len(inv) == 12 and all(int(ln[2]) == RR_INVPARAM for ln in inv), inv
    assert [int(ln[1]) for ln in lines if ln[0] in ("ok1", "ok2")] == [RR_EXTUNINIT, RR_EXTUNINIT]


def test_python_wrapper_checks_bounds_on_the_host():
    class Fake:  # stands in for a device tensor: the wrapper must refuse before any C call
        def __init__(self, shape, dtype="torch.float32", contiguous=True):
            self.shape, self.dtype, self._c = shape, dtype, contiguous

        def is_contiguous(self):
            return self._c

        def data_ptr(self):
            raise AssertionError("the bounds are checked before the pointer is taken")

    with pytest.raises(ValueError):
        F.lpc_extrapolate_device(Fake((3, 100, 2)), 10, 80, 11, 0)     # first < extra_bkwd
    with pytest.raises(ValueError):
        F.lpc_extrapolate_device(Fake((3, 100, 2)), 10, 80, 0, 11)     # runs past the last frame
    with pytest.raises(ValueError):
        F.lpc_extrapolate_device(Fake((100,)), 0, 80, 0, 0)
    with pytest.raises(ValueError):
        F.lpc_extrapolate_device(Fake((100, 2), contiguous=False), 0, 80, 0, 0)
    with pytest.raises(TypeError):
        F.lpc_extrapolate_device(Fake((100, 2), dtype="torch.float64"), 0, 80, 0, 0)
