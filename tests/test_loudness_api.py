"""The loudness measurement's host side (RRX_loudness_device / RRX_tracks_loudness_device / RRX_loudness_gate_device and their
host twins): the symbols, the refusals that need no device, and the arithmetic -- the host twins are serial loops over the very
functions the kernels call -- against the numpy restatement in loudness_model.py, bit for bit; the block decomposition against the
serial filter; and known answers (BS.1770, EBU Tech 3341).  CPU only."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import foo_dsp_resampler_amd as F
import loudness_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RR_OK, RR_EXTUNINIT, RR_INVPARAM = 0, 5, 6
GUARD = 777.25
NAMES = ("RRX_loudness_device", "RRX_loudness_work_doubles", "RRX_debug_loudness_host", "RRX_tracks_loudness_device",
         "RRX_loudness_gate_device", "RRX_debug_loudness_gate_host")


def host(x, hop, coefs=M.K48, gain=None, first_frame=0, state=None, energy=None, stride=None, extra_work=3):
    """RRX_debug_loudness_host on x [nstreams, frames, nch] (rows `stride` frames apart inside x's buffer when given): (rc, energy
    [nstreams, nch, first_hop + n], state_out, work).  The work buffer is `extra_work` doubles longer than needed, under guards."""
    ns, frames, nch = x.shape
    n, first_hop = frames // hop, first_frame // hop
    need = F.lib().RRX_loudness_work_doubles(ns, nch, frames, hop)
    assert need == ns * nch * n * 4
    work = np.full(need + extra_work, GUARD)
    if energy is None:
        energy = np.full((ns, nch, first_hop + n + 2), GUARD)
    so = np.full((ns, nch, 4), GUARD)
    co = np.ascontiguousarray(coefs, dtype=np.float64)
    g = None if gain is None else np.ascontiguousarray(gain, dtype=np.float64)
    rc = F.lib().RRX_debug_loudness_host(int(x.dtype == np.float64), x.ctypes.data, frames if stride is None else stride, ns, frames, nch,
                                         None if g is None else g.ctypes.data, first_frame, co.ctypes.data, hop,
                                         None if state is None else state.ctypes.data, so.ctypes.data, energy.ctypes.data, energy.shape[2],
                                         work.ctypes.data, need)
    assert np.all(work[need:] == GUARD)
    return rc, energy, so, work


def gate_host(energy, hop, hops=None, weights=None, nhops=None, abs_lufs=-70.0, rel_lu=-10.0):
    ns, nch, stride = energy.shape
    energy = np.ascontiguousarray(energy)
    nhops = stride if nhops is None else nhops
    res = np.full((ns, 4), GUARD)
    h = None if hops is None else np.ascontiguousarray(hops, dtype=np.uint64)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    a, r = F.loudness_gate(abs_lufs, rel_lu)
    rc = F.lib().RRX_debug_loudness_gate_host(energy.ctypes.data, stride, ns, nch, nhops, None if h is None else h.ctypes.data,
                                              None if w is None else w.ctypes.data, hop, a, r, res.ctypes.data)
    assert rc == RR_OK
    return res


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_symbols_are_exported_listed_and_declared():
    header = open(os.path.join(ROOT, "include", "ratelib_amd.h")).read()
    for name in NAMES:
        assert name in F.EXPECTED_SYMBOLS and name in F.available_symbols()
        assert name + "(" in header
    for name in ("k_weighting", "loudness_device", "tracks_loudness_device", "loudness_gate_device", "integrated_lufs"):
        assert callable(getattr(F, name))
    assert hasattr(F.Resampler, "convert_tracks_to_pcm_loudness_normalized")
    assert "S_{k+1}[i] = (((M[i][0]*S_k[0] + M[i][1]*S_k[1]) + M[i][2]*S_k[2]) + M[i][3]*S_k[3]) + z_k[i]" in header
    assert F.lib().RRX_loudness_work_doubles(3, 2, 1000, 48) == 3 * 2 * 20 * 4
    assert F.lib().RRX_loudness_work_doubles(3, 2, 1000, 0) == 0 and F.lib().RRX_loudness_work_doubles(0, 2, 1000, 48) == 0


def test_k_weighting_reproduces_the_published_table():
    assert tuple(F.K_WEIGHTING_48K) == tuple(M.K48)
    got = np.array(F.k_weighting(48000))
    print("largest difference to the table of BS.1770-4: %.3g" % np.abs(got - M.K48).max())
    assert np.abs(got - M.K48).max() <= 1e-14
    assert tuple(got[5:8]) == (1.0, -2.0, 1.0)
    for rate in (8000, 44100, 96000, 192000):  # stable poles, unity at high frequencies for the high-pass, +4 dB for the shelf
        c = np.array(F.k_weighting(rate))
        for a1, a2 in ((c[3], c[4]), (c[8], c[9])):
            assert abs(a2) < 1 and abs(a1) < 1 + a2
        assert abs(20 * np.log10((c[0] - c[1] + c[2]) / (1 - c[3] + c[4])) - 3.999843853973347) < 1e-9  # the shelf at Nyquist


CHILD = r"""
import sys, ctypes as C
sys.path.insert(0, %r)
import foo_dsp_resampler_amd as F
L = F.lib()
cb = F.ratelib._ALLOC_CB(lambda: None)
p = 0x10000  # never dereferenced: every call below is answered from its arguments, or from the library's state, alone
co = (C.c_double * 10)(*F.K_WEIGHTING_48K)
bad = (C.c_double * 10)(*(list(F.K_WEIGHTING_48K[:9]) + [float("inf")]))
nan = (C.c_double * 10)(*([float("nan")] + list(F.K_WEIGHTING_48K[1:])))
co_p = C.cast(co, C.c_void_p)
# 2 streams x 2 channels x 1024 frames in hops of 100: n = 10, 160 doubles of work
good = dict(device=-1, stream=None, sf=0, src=p, ss=4096, nstreams=2, frames=1024, nch=2, gain=None, first=0, coefs=co_p, hop=100,
            sin=None, sout=p + (1 << 20), energy=p, es=10, work=p, wd=160)
def call(**kw):
    a = dict(good, **kw)
    return L.RRX_loudness_device(a["device"], a["stream"], a["sf"], a["src"], a["ss"], a["nstreams"], a["frames"], a["nch"], a["gain"],
                                 a["first"], a["coefs"], a["hop"], a["sin"], a["sout"], a["energy"], a["es"], a["work"], a["wd"])
tgood = dict(device=-1, stream=None, table=p, ntracks=3, nch=2, sf=0, rows=p, row_frames=4096, gain=None, coefs=co_p, hop=100, energy=p, es=40,
             hops=p, work=p, wd=3 * 2 * 40 * 4)
def tcall(**kw):
    a = dict(tgood, **kw)
    return L.RRX_tracks_loudness_device(a["device"], a["stream"], a["table"], a["ntracks"], a["nch"], a["sf"], a["rows"], a["row_frames"],
                                        a["gain"], a["coefs"], a["hop"], a["energy"], a["es"], a["hops"], a["work"], a["wd"])
ggood = dict(device=-1, stream=None, energy=p, es=40, nstreams=3, nch=2, nhops=40, hops=None, weights=None, hop=100, abs=1e-7, rel=0.1, result=p)
def gcall(**kw):
    a = dict(ggood, **kw)
    return L.RRX_loudness_gate_device(a["device"], a["stream"], a["energy"], a["es"], a["nstreams"], a["nch"], a["nhops"], a["hops"],
                                      a["weights"], a["hop"], a["abs"], a["rel"], a["result"])
print("uninit", call(), tcall(), gcall())                 # before init_ratelib
print("init", L.init_ratelib(cb))                         # no device: refuses
print("uninit", call(), call(frames=0), tcall(), tcall(row_frames=0), gcall())
for name, kw in [("null", dict(src=None)), ("nstreams0", dict(nstreams=0)), ("nstreams-1", dict(nstreams=-1)), ("nch0", dict(nch=0)),
                 ("nch-1", dict(nch=-1)), ("srcfmt16", dict(sf=16)), ("srcfmt7", dict(sf=7)), ("sstride", dict(ss=1023)), ("sstride0", dict(ss=0)),
                 ("wrap", dict(first=2**64 - 1000, sin=p + (2 << 20), es=2**62)),
                 ("samples2^60", dict(frames=2**59, ss=2**59, es=2**56, wd=2**62)), ("srcrows2^60", dict(ss=2**58)), ("device-2", dict(device=-2)),
                 ("coefs", dict(coefs=None)), ("inf", dict(coefs=C.cast(bad, C.c_void_p))), ("nan", dict(coefs=C.cast(nan, C.c_void_p))),
                 ("hop0", dict(hop=0)), ("energy", dict(energy=None)), ("energy-stride", dict(es=9)), ("energy-stride-first", dict(first=100, sin=p + (2 << 20))),
                 ("energy2^60", dict(es=2**58)), ("work-short", dict(wd=159)), ("work-null", dict(work=None)),
                 ("first-off-the-grid", dict(first=150, sin=p + (2 << 20), es=20)), ("first-without-state", dict(first=100, es=11)),
                 ("same-state", dict(first=100, es=11, sin=p + (1 << 20))), ("overlapping-state", dict(first=100, es=11, sin=p + (1 << 20) + 8)),
                 ("same-state-at-0", dict(sin=p + (1 << 20))), ("overlap-below", dict(first=100, es=11, sin=p + (1 << 20) - 2 * 2 * 4 * 8 + 8))]:
    print("inv", name, call(**kw))
for name, kw in [("one-stream", dict(nstreams=1, ss=0)), ("tight", dict(ss=1024)), ("double", dict(sf=1)), ("gain", dict(gain=p)),
                 ("no-state-out", dict(sout=None)), ("state", dict(first=100, es=11, sin=p + (2 << 20))),
                 ("adjacent-state", dict(first=100, es=11, sin=p + (1 << 20) - 2 * 2 * 4 * 8)), ("state-unread-at-0", dict(sin=p + (2 << 20))),
                 ("hop1", dict(hop=1, es=1024, wd=2 * 2 * 1024 * 4)), ("no-whole-hop", dict(hop=2000, es=0, work=None, wd=0)),
                 ("more-work", dict(wd=1000)), ("rows-below-2^60", dict(ss=2**58 - 1))]:
    print("ok", name, call(**kw))                         # nothing to refuse: answered RR_EXTUNINIT here
for name, kw in [("table", dict(table=None)), ("rows", dict(rows=None)), ("ntracks0", dict(ntracks=0)), ("nch0", dict(nch=0)), ("srcfmt16", dict(sf=16)),
                 ("energy", dict(energy=None)), ("hops", dict(hops=None)), ("coefs", dict(coefs=None)), ("inf", dict(coefs=C.cast(bad, C.c_void_p))),
                 ("hop0", dict(hop=0)), ("rows2^60", dict(row_frames=2**58, wd=2**62)), ("energy2^60", dict(es=2**58)), ("work-short", dict(wd=959)),
                 ("work-null", dict(work=None)), ("device-2", dict(device=-2))]:
    print("tinv", name, tcall(**kw))
for name, kw in [("double", dict(sf=1)), ("gain", dict(gain=p)), ("short-energy", dict(es=1)), ("hop1", dict(hop=1, wd=3 * 2 * 4096 * 4))]:
    print("tok", name, tcall(**kw))
for name, kw in [("energy", dict(energy=None)), ("result", dict(result=None)), ("nstreams0", dict(nstreams=0)), ("nch0", dict(nch=0)), ("hop0", dict(hop=0)),
                 ("nhops", dict(nhops=41)), ("energy2^60", dict(es=2**58, nhops=0)), ("nan-abs", dict(abs=float("nan"))),
                 ("nan-rel", dict(rel=float("nan"))), ("device-2", dict(device=-2))]:
    print("ginv", name, gcall(**kw))
for name, kw in [("hops", dict(hops=p)), ("weights", dict(weights=p)), ("nhops0", dict(nhops=0)), ("no-abs-gate", dict(abs=float("-inf")))]:
    print("gok", name, gcall(**kw))
"""


def test_invalid_parameters_are_refused_without_a_device():
    out = subprocess.run([sys.executable, "-c", CHILD % ROOT], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))
    assert out.returncode == 0, out.stderr
    kinds = ("uninit", "init", "inv", "ok", "tinv", "tok", "ginv", "gok")
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.split() and ln.split()[0] in kinds]
    assert ["init", "-1"] in lines
    uninit = [ln for ln in lines if ln[0] == "uninit"]
    assert len(uninit) == 2 and all(int(v) == RR_EXTUNINIT for ln in uninit for v in ln[1:])
    for kind, count, want in (("inv", 29, RR_INVPARAM), ("ok", 12, RR_EXTUNINIT), ("tinv", 15, RR_INVPARAM), ("tok", 4, RR_EXTUNINIT),
                              ("ginv", 10, RR_INVPARAM), ("gok", 4, RR_EXTUNINIT)):
        got = [ln for ln in lines if ln[0] == kind]
        assert len(got) == count and all(int(ln[2]) == want for ln in got), got


def test_host_twins_refuse_as_the_device_calls_do_and_leave_the_results_alone():
    x = np.ones((2, 64, 2), np.float32)
    energy, work, state = np.full((2, 2, 8), 5.0), np.full(2 * 2 * 8 * 4, 6.0), np.zeros((2, 2, 4))
    co = M.K48.copy()
    fn = F.lib().RRX_debug_loudness_host

    def call(**kw):
        so = np.full((2, 2, 4), 7.0)
        c = kw.get("coefs", co)
        rc = fn(kw.get("sf", 0), kw.get("src", x.ctypes.data), kw.get("ss", 64), kw.get("ns", 2), kw.get("frames", 64), kw.get("nch", 2), None,
                kw.get("first", 0), None if c is None else c.ctypes.data, kw.get("hop", 8), kw.get("sin", None),
                so.ctypes.data if kw.get("sout", True) is True else kw["sout"], energy.ctypes.data if kw.get("energy", True) else None,
                kw.get("es", 8), work.ctypes.data, kw.get("wd", work.size))
        return rc, so

    inf = co.copy()
    inf[3] = -np.inf
    for kw in (dict(src=None), dict(ns=0), dict(nch=0), dict(sf=16), dict(ss=63), dict(energy=False), dict(coefs=None), dict(coefs=inf), dict(hop=0),
               dict(es=7), dict(wd=127), dict(first=4, sin=state.ctypes.data), dict(first=8), dict(first=8, es=16, sin=state.ctypes.data, sout=state.ctypes.data),
               dict(sin=state.ctypes.data, sout=state.ctypes.data + 32), dict(first=2 ** 64 - 64, sin=state.ctypes.data, es=2 ** 62)):
        rc, so = call(**kw)
        assert rc == RR_INVPARAM, kw
        assert np.all(energy == 5.0) and np.all(work == 6.0) and np.all(so == 7.0) and not state.any(), kw
    rc, so = call(frames=0)  # nothing to do: nothing is touched, the state included
    assert rc == RR_OK and np.all(energy == 5.0) and np.all(work == 6.0) and np.all(so == 7.0)
    rc, so = call()
    assert rc == RR_OK and not np.any(energy == 5.0) and not np.all(so == 7.0)
    res = np.full((2, 4), 7.0)
    g = F.lib().RRX_debug_loudness_gate_host
    for args in ((None, 8, 2, 2, 8, None, None, 8, 0.0, 0.1, res.ctypes.data), (energy.ctypes.data, 8, 2, 2, 9, None, None, 8, 0.0, 0.1, res.ctypes.data),
                 (energy.ctypes.data, 8, 2, 2, 8, None, None, 0, 0.0, 0.1, res.ctypes.data), (energy.ctypes.data, 8, 2, 2, 8, None, None, 8, 0.0, 0.1, None),
                 (energy.ctypes.data, 8, 2, 2, 8, None, None, 8, float("nan"), 0.1, res.ctypes.data)):
        assert g(*args) == RR_INVPARAM and np.all(res == 7.0)
    code = ("import sys; sys.path.insert(0, %r)\nimport foo_dsp_resampler_amd as F\n"
            "print(F.lib().RRX_debug_loudness_host(0, None, 0, 1, 0, 1, None, 0, None, 1, None, None, None, 0, None, 0))\n"
            "print(F.lib().RRX_debug_loudness_gate_host(None, 0, 1, 1, 0, None, None, 1, 0.0, 0.1, None))\n" % ROOT)
    env = {k: v for k, v in os.environ.items() if k != "RSMP_TEST_HOOKS"}
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-2:] == ["-1", "-1"]


def test_python_wrappers_check_on_the_host():
    class Fake:  # stands in for a device tensor: the wrapper must refuse before any C call
        def __init__(self, shape, dtype="torch.float32", contiguous=True):
            self.shape, self.dtype, self._c = shape, dtype, contiguous

        def is_contiguous(self):
            return self._c

        def data_ptr(self):
            raise AssertionError("the arguments are checked before the pointer is taken")

    with pytest.raises(ValueError):
        F.loudness_device(Fake((100,)), 48000)
    with pytest.raises(ValueError):
        F.loudness_device(Fake((100, 2), contiguous=False), 48000)
    with pytest.raises(TypeError):
        F.loudness_device(Fake((100, 2), dtype="torch.int16"), 48000)
    with pytest.raises(ValueError):
        F.loudness_device(Fake((100, 2)))  # neither a rate nor coefficients
    with pytest.raises(ValueError):
        F.loudness_device(Fake((100, 2)), coefs=[1.0] * 9, hop=10)
    with pytest.raises(ValueError):
        F.loudness_device(Fake((100, 2)), coefs=[1.0] * 9 + [float("nan")], hop=10)
    with pytest.raises(ValueError):
        F.loudness_device(Fake((100, 2)), 48000, hop=0)
    with pytest.raises(ValueError):
        F.loudness_device(Fake((100, 2)), 48000, first_frame=100)  # not a multiple of 4800
    with pytest.raises(ValueError):
        F.loudness_device(Fake((100, 2)), 48000, first_frame=4800)  # no state
    with pytest.raises(TypeError):
        F.loudness_device(Fake((100, 2)), 48000)  # not a device tensor
    with pytest.raises(TypeError):
        F.loudness_gate_device(torch.zeros((2, 2, 8), dtype=torch.float64), 4800)  # not on the device


CASES = [(ns, nch, hop, f) for (ns, nch) in ((1, 1), (1, 2), (3, 3), (2, 6)) for hop in (1, 7, 48, 4410) for f in range(6)]


@pytest.mark.parametrize("ns,nch,hop,f", CASES)
def test_host_twin_equals_the_model_bit_for_bit(ns, nch, hop, f):
    frames = (0, hop - 1, hop, 4 * hop - 1, 4 * hop, 37 * hop + 5)[f]
    rng = np.random.default_rng(ns * 1000 + nch * 100 + hop + f)
    base = rng.standard_normal((ns, frames + 3, nch)) * 0.3
    gain = np.linspace(0.5, 1.7, ns)
    variants = [(dt, g) for dt in (np.float32, np.float64) for g in (None, gain)]
    bufs = [np.ascontiguousarray(base.astype(dt)) for dt, _ in variants]  # rows of `frames` at a pitch of frames + 3: the rest is a guard
    for b in bufs:
        b[:, frames:] = GUARD
    stacked = np.concatenate([M.gained(b[:, :frames], g) for b, (_, g) in zip(bufs, variants)])
    want_e, want_s = M.hop_energies(stacked, M.K48, hop)
    n = frames // hop
    for v, (b, (dt, g)) in enumerate(zip(bufs, variants)):
        rc, e, so, _ = host(b[:, :frames], hop, gain=g, stride=frames + 3)
        assert rc == RR_OK
        if not frames:
            assert np.all(e == GUARD) and np.all(so == GUARD)  # frames == 0 touches nothing
            continue
        assert np.array_equal(bits(e[:, :, :n]), bits(want_e[v * ns:(v + 1) * ns])), (dt, g is not None)
        assert np.all(e[:, :, n:] == GUARD)
        assert np.array_equal(bits(so), bits(want_s[v * ns:(v + 1) * ns])), (dt, g is not None)
        assert np.all(b[:, frames:] == GUARD)


@pytest.mark.parametrize("hop", [7, 48])
def test_chunked_calls_cut_at_hop_multiples_equal_one_call(hop):
    rng = np.random.default_rng(hop)
    nh = 29
    x = (rng.standard_normal((2, nh * hop + 3, 3)) * 0.3).astype(np.float32)
    gain = np.array([0.5, 1.7])
    rc, e1, s1, _ = host(x, hop, gain=gain)
    assert rc == RR_OK
    for cuts in ([1], [0], [nh], [5, 5, 6], [1, 2, 3, 17, 28], [14]):  # equal edges: a call without a whole hop (n == 0) in between
        edges = [0] + [c * hop for c in cuts] + [x.shape[1]]
        energy = np.full((2, 3, nh + 2), GUARD)
        state = None
        for a, b in zip(edges, edges[1:]):
            chunk = np.ascontiguousarray(x[:, a:b] if b - a else x[:, a:a + hop - 1])  # n == 0 with frames: hop - 1 of them (hop 7, 48 > 1)
            rc, energy, state, _ = host(chunk, hop, gain=gain, first_frame=a, state=state, energy=energy)
            assert rc == RR_OK
        assert np.array_equal(bits(energy), bits(e1)), cuts
        assert np.array_equal(bits(state), bits(s1)), cuts
    # the model cuts the same way, and a state is not read at frame 0
    g = M.gained(x, gain)
    ea, sa = M.hop_energies(g[:, :10 * hop], M.K48, hop)
    eb, sb = M.hop_energies(g[:, 10 * hop:], M.K48, hop, state=sa)
    assert np.array_equal(bits(np.concatenate([ea, eb], axis=2)), bits(e1[:, :, :nh])) and np.array_equal(bits(sb), bits(s1))
    rc, e2, s2, _ = host(x, hop, gain=gain, state=np.full((2, 3, 4), 123.0))
    assert rc == RR_OK and np.array_equal(bits(e2), bits(e1)) and np.array_equal(bits(s2), bits(s1))


@pytest.mark.parametrize("hop,measured", [(480, 2.73e-13), (4800, 5.5e-15)])
def test_the_decomposition_agrees_with_the_serial_filter(hop, measured):
    """White noise at 48 kHz, 24000 frames per channel: the hop energies of the decomposition against those of the serial
    recursion (scipy.signal.lfilter).  Measured with the host twin: the largest relative difference is 2.73e-13 at hop 480 (50
    carries: the rounding of every M S_k enters the hops behind it) and 5.5e-15 at hop 4800 (5 carries); the bound is 16 times
    the measured value.  Anything above 1e-9 would be a bug, not a tolerance."""
    rng = np.random.default_rng(1770)
    x = rng.standard_normal((2, 24000, 2)) * 0.25
    rc, e, _, _ = host(x, hop)
    assert rc == RR_OK
    n = 24000 // hop
    ref = M.serial_energies(x, M.K48, hop)
    rel = np.abs(e[:, :, :n] - ref) / ref
    print("hop %d: largest relative hop-energy difference to the serial filter %.3g" % (hop, rel.max()))
    assert rel.max() <= 16 * measured < 1e-9


def measure(x, rate, weights=None):
    """integrated loudness of x [frames, nch] through the two host twins and integrated_lufs"""
    hop = rate // 10
    rc, e, _, _ = host(np.ascontiguousarray(x[None]), hop, coefs=np.array(F.k_weighting(rate)))
    assert rc == RR_OK
    n = x.shape[0] // hop
    res = gate_host(e[:, :, :n], hop, weights=weights)
    model = M.gate(np.ascontiguousarray(e[:, :, :n]), hop, weights=weights)
    assert np.array_equal(bits(res), bits(model))
    return float(F.integrated_lufs(torch.from_numpy(res))[0])


def tone(rate, freq, nch, pieces):
    """pieces of (dBFS, seconds) of one phase-continuous sine, the same on every channel"""
    amp = np.concatenate([np.full(int(round(sec * rate)), 10.0 ** (db / 20.0)) for db, sec in pieces])
    t = np.arange(amp.size) / rate
    return np.repeat((amp * np.sin(2 * np.pi * freq * t))[:, None], nch, axis=1)


def test_a_full_scale_997_hz_sine_is_minus_3_01_lufs():
    got = measure(tone(48000, 997.0, 1, [(0.0, 5.0)]), 48000)
    print("997 Hz, 0 dBFS, mono, 48 kHz: %.4f LUFS" % got)
    assert abs(got - -3.01) <= 0.1


@pytest.mark.parametrize("want,pieces", [(-23.0, [(-23.0, 20.0)]), (-33.0, [(-33.0, 20.0)]), (-23.0, [(-36.0, 10.0), (-23.0, 60.0), (-36.0, 10.0)]),
                                         (-23.0, [(-72.0, 10.0), (-36.0, 10.0), (-23.0, 60.0), (-36.0, 10.0), (-72.0, 10.0)]),
                                         (-23.0, [(-26.0, 20.0), (-20.0, 20.1), (-26.0, 20.0)])], ids=["1", "2", "3", "4", "5"])
def test_ebu_tech_3341_sequences(want, pieces):
    """EBU Tech 3341 test cases 1 to 5 with a 1 kHz stereo tone, at a rate of 8000 to keep them small"""
    got = measure(tone(8000, 1000.0, 2, pieces), 8000)
    print("%r: %.4f LUFS" % (pieces, got))
    assert abs(got - want) <= 0.1


def test_gate_edge_cases():
    rng = np.random.default_rng(3)
    hop = 4800
    e = rng.uniform(1.0, 50.0, (2, 3, 40))
    for n in (0, 1, 3):  # fewer than four hops: no block
        assert not gate_host(e, hop, nhops=n).any()
    res = gate_host(e, hop, nhops=4)
    assert np.all(res[:, 1] == 1.0) and np.all(res[:, 3] == 1.0) and np.array_equal(bits(res), bits(M.gate(e[:, :, :4], hop)))
    quiet = e * 1e-12  # everything under the absolute gate
    res = gate_host(quiet, hop)
    assert not res.any() and np.array_equal(res, M.gate(quiet, hop))
    assert F.integrated_lufs(torch.from_numpy(res)).tolist() == [float("-inf")] * 2
    holed = e.copy()
    holed[1, 2, 17] = np.nan  # poisons the four blocks it enters, which are skipped
    res = gate_host(holed, hop)
    want = M.gate(holed, hop)
    assert np.array_equal(bits(res), bits(want)) and res[1, 3] == 37 - 4 and res[0, 3] == 37 and np.isfinite(res).all()
    six = rng.uniform(1.0, 50.0, (2, 6, 40))
    six[:, :, 20:] *= 0.01  # a quiet half the relative gate removes
    w = [1.0, 1.0, 1.0, 0.0, 1.41, 1.41]
    res = gate_host(six, hop, weights=w)
    assert np.array_equal(bits(res), bits(M.gate(six, hop, weights=w))) and np.all(res[:, 1] < res[:, 3]) and np.all(res[:, 1] > 0)
    assert not np.array_equal(res, gate_host(six, hop))
    lfe = six.copy()
    lfe[:, 3] *= 1000.0  # weight 0: the LFE channel does not count
    assert np.array_equal(bits(gate_host(lfe, hop, weights=w)), bits(res))
    hops = [9, 100]  # d_hops shorter than nhops for stream 0, beyond it (clamped) for stream 1
    res = gate_host(e, hop, hops=hops)
    assert np.array_equal(bits(res), bits(M.gate(e, hop, hops=hops))) and res[0, 3] == 6 and res[1, 3] == 37
    assert np.array_equal(bits(res[:1]), bits(M.gate(e[:1, :, :9], hop)))
