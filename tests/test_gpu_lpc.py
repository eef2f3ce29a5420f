"""The LPC edge extrapolator on the device (csrc/lpc.hip, RRX_lpc_extrapolate_device) and the whole-track conversion built on it.

The bar is EQUALITY of bits: the kernel keeps the reference's operations and their order, so its output is
compared as uint32 against (a) the reference's own vectors, tests/golden/lpc_reference_vectors.npz (lpc/lpc.cpp compiled as it
lies, on the seeded inputs of tests/lpc_cases.py) and (b) the harness's restatement, orc_lpc_extrapolate, which
tests/test_lpc_reference.py pins on those vectors.  The end-to-end test compares Resampler.convert_track_device with the plugin
harness over the CPU resampler under the parity bar of tests/test_plugin_layer.py, unchanged.

NaN samples.  A NaN in the base frames must come out as a NaN, in its own channel only, and every sample that is not a NaN must
still have the host's bits; the sign and payload of the NaN itself are not compared.  IEEE 754 leaves them open, and the host's
are no property of lpc.cpp: x86 SSE returns the FIRST NaN operand of an operation, and which operand of a commutative operation
comes first is the register allocation of the compiler that built the host code.  Measured on an MI355X: every extrapolated
sample of the NaN channel is 0x7fc00000 where this tree's x86-64 build of orc_lpc_extrapolate gives 0xffc00000, in all five
shapes; every other sample of those cases, and every sample of the finite cases, is bit-identical.  (A kernel variant that
replaced each NaN result by SSE's first-operand choice in source order did not reproduce that host build either: on the CPU it
differed from it in the NaN samples of 4 of 7 cases.)"""
import ctypes as C
import os

import numpy as np
import pytest

import foo_dsp_resampler_amd as F
from lpc_cases import CASES, make_input
from oracle_binding import OracleDsp, lcg_noise, lib as oracle_lib
from test_plugin_layer import music_like, run_track

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "lpc_reference_vectors.npz"), allow_pickle=False)
SENTINEL = 123.0
RR_INVPARAM = 6


def host_lpc(x, order, bk, fw):
    """orc_lpc_extrapolate on a host copy: (backward frames, forward frames)"""
    fn = oracle_lib().orc_lpc_extrapolate
    fn.argtypes, fn.restype = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_size_t, C.c_size_t], None
    n, nch = x.shape
    buf = np.zeros((bk + n + fw, nch), np.float32)
    buf[bk:bk + n] = x
    fn(buf.ctypes.data + bk * nch * 4, n, nch, order, bk, fw)
    assert np.array_equal(buf[bk:bk + n].view(np.uint32), x.view(np.uint32))
    return buf[:bk], buf[bk + n:]


def device_lpc(x, order, bk, fw, stream=None):
    """The device call on [bk + n + fw, nch] frames: (backward frames, forward frames); the base frames must be unchanged."""
    import torch
    n, nch = x.shape
    buf = np.full((bk + n + fw, nch), SENTINEL, np.float32)
    buf[bk:bk + n] = x
    t = torch.from_numpy(buf).cuda()
    F.lpc_extrapolate_device(t, bk, n, bk, fw, order=order, stream=stream)
    if stream is not None:
        stream.synchronize()
    got = t.cpu().numpy()
    assert np.array_equal(got[bk:bk + n].view(np.uint32), x.view(np.uint32))
    return got[:bk], got[bk + n:]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(got, want):
    """Bit for bit; where the host has a NaN, a NaN (module docstring)."""
    g, w = bits(got).copy(), bits(want).copy()
    g[np.isnan(got)] = w[np.isnan(want)] = 0x7fc00000
    return np.array_equal(g, w)


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_device_lpc_matches_reference_vectors(idx):
    case = CASES[idx]
    b, f = device_lpc(make_input(case), case["order"], case["bk"], case["fw"])
    for got, want in ((b, GOLD["case%d_bkwd" % idx]), (f, GOLD["case%d_fwd" % idx])):
        print(case, "differing samples:", int((bits(got) != bits(want)).sum()), "of", got.size)
        assert np.array_equal(bits(got), bits(want)), case


def with_nan(n, nch, order):
    x = music_like(n, nch, 44100, 11)
    x[n - 1 - order // 2, 0] = np.nan          # inside the last `order` frames of channel 0; the other channels stay finite
    return x


INPUTS = {"music": lambda n, nch, order: music_like(n, nch, 44100, 5), "noise": lambda n, nch, order: lcg_noise(n, nch, 99),
          "nan": with_nan}
# (n, nch, order, bk, fw); the last one is past what the kernel keeps in LDS (16384 frames): the window is recomputed on the fly
SHAPES = [(16384, 2, 32, 8192, 8192), (65, 3, 32, 5, 0), (1024, 1, 1, 0, 7), (4097, 5, 17, 33, 1), (16385, 1, 32, 3, 3)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", sorted(INPUTS))
def test_device_lpc_matches_live_oracle(kind, shape):
    n, nch, order, bk, fw = shape
    x = INPUTS[kind](n, nch, order)
    wb, wf = host_lpc(x, order, bk, fw)
    gb, gf = device_lpc(x, order, bk, fw)
    for got, want in ((gb, wb), (gf, wf)):
        diff = bits(got) != bits(want)
        print(kind, shape, "differing samples:", int(diff.sum()), "of", got.size,
              [(hex(a), hex(b)) for a, b in zip(bits(got)[diff][:4], bits(want)[diff][:4])])
        assert same_bits(got, want) if kind == "nan" else np.array_equal(bits(got), bits(want))
    if kind == "nan":
        assert np.isnan(np.concatenate([gb, gf])[:, 0]).all()     # the NaN passes through the clamp ...
        assert np.isfinite(np.concatenate([gb, gf])[:, 1:]).all()  # ... and stays in its channel


def test_device_lpc_batch_equals_single_streams_and_keeps_its_range():
    import torch
    S, nch, n, order, bk, fw = 3, 2, 300, 32, 40, 50
    first = bk + 7
    frames = first + n + fw + 64
    x = np.stack([music_like(n, nch, 44100, 20 + s) for s in range(S)])
    buf = np.full((S, frames, nch), SENTINEL, np.float32)
    buf[:, first:first + n] = x
    t = torch.from_numpy(buf).cuda()
    F.lpc_extrapolate_device(t, first, n, bk, fw, order=order)
    got = t.cpu().numpy()
    assert (got[:, :first - bk] == SENTINEL).all() and (got[:, first + n + fw:] == SENTINEL).all()
    assert np.array_equal(bits(got[:, first:first + n]), bits(x))
    for s in range(S):
        one = torch.from_numpy(buf[s]).cuda()                      # [frames, nch]: the one-stream form
        F.lpc_extrapolate_device(one, first, n, bk, fw, order=order)
        assert np.array_equal(bits(one.cpu().numpy()), bits(got[s])), s
        b, f = host_lpc(x[s], order, bk, fw)
        assert np.array_equal(bits(got[s, first - bk:first]), bits(b)) and np.array_equal(bits(got[s, first + n:first + n + fw]), bits(f))


def test_device_lpc_stream_and_device_contract():
    import torch
    n, nch, order, bk, fw = 1000, 2, 32, 100, 100
    x = music_like(n, nch, 44100, 31)
    want = device_lpc(x, order, bk, fw)
    dev = torch.cuda.current_device()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                                  # the tensor is filled on the side stream
        got = device_lpc(x, order, bk, fw, stream=side)
    assert torch.cuda.current_device() == dev
    for g, w in zip(got, want):
        assert np.array_equal(bits(g), bits(w))
    t = torch.zeros((bk + n + fw, nch), dtype=torch.float32, device="cuda")
    rc = F.lib().RRX_lpc_extrapolate_device(torch.cuda.device_count(), None, C.c_void_p(t.data_ptr() + bk * nch * 4), 0, 1, n, nch,
                                            order, bk, fw)
    assert rc == RR_INVPARAM
    assert torch.cuda.current_device() == dev
    torch.cuda.synchronize()
    assert not t.any()                                             # a refused call writes nothing


@pytest.mark.parametrize("frames", [1500, 40, 30000])
def test_convert_track_device_matches_plugin_harness(frames):
    """Two streams with different tracks: one short buffer (both edges from the same frames), too short to extrapolate, and a
    track longer than the plugin's staging buffer."""
    import torch
    from parity import assert_parity
    fs, fo, nch, S = 44100, 48000, 2, 2
    x = np.stack([music_like(frames, nch, fs, 40 + s) for s in range(S)])
    r = F.Resampler(fs, fo, nch=nch, nstreams=S)
    y = r.convert_track_device(torch.from_numpy(x).cuda()).cpu().numpy()
    r.close()
    for s in range(S):
        outs, _ = run_track(OracleDsp(fo), x[s], fs, [4096])
        ref = np.concatenate([c for c, _ in outs])
        assert y[s].shape == ref.shape, (y.shape, ref.shape)
        print(frames, s, assert_parity(y[s], ref))
