"""The packed meter calls' host side (RRX_tracks_true_peak_packed_device / RRX_tracks_loudness_packed_device and their host
twins): the symbols, the refusals that need no device, and the arithmetic -- the twins are loops over the clamp, the one-sample
load and the per-frame functions the kernels call -- against one-stream RRX_debug_true_peak_host / RRX_debug_loudness_host calls
per track on float64 arrays of the exact conversion, bit for bit.  CPU only."""
import os
import subprocess
import sys

import numpy as np
import pytest

import foo_dsp_resampler_amd as F
import scan_cases as S
from scan_cases import RR_EXTUNINIT, RR_INVPARAM, RR_OK

ROOT = S.ROOT
NAMES = ("RRX_tracks_true_peak_packed_device", "RRX_debug_tracks_true_peak_packed_host", "RRX_tracks_loudness_packed_device",
         "RRX_debug_tracks_loudness_packed_host")


def as_double(b):
    return np.asarray(b, dtype=np.uint64).view(np.float64)


def test_symbols_are_exported_and_listed():
    header = open(os.path.join(ROOT, "include", "ratelib_amd.h")).read()
    for name in NAMES:
        assert name in F.EXPECTED_SYMBOLS and name in F.available_symbols()
        assert name + "(" in header
    for words in ("first  = min(src_first, src_total)", "frames = min(frames, src_total - first, max_frames)", "1 - 2^-31"):
        assert words in header
    for fn in (F.packed_plan, F.tracks_true_peak_packed_device, F.tracks_loudness_packed_device, F.scan_tracks_pcm):
        assert callable(fn)
    L = F.lib()
    assert len(L.RRX_tracks_true_peak_packed_device.argtypes) == 15 and len(L.RRX_debug_tracks_true_peak_packed_host.argtypes) == 13
    assert len(L.RRX_tracks_loudness_packed_device.argtypes) == 17 and len(L.RRX_debug_tracks_loudness_packed_host.argtypes) == 15


def test_the_tile_seams_come_from_the_kernel_constant():
    assert S.lds_doubles() == 4096 and S.tile_frames(2, 12) == 2037
    assert S.lengths(12) == [0, 1, 10, 2037, 2038, 4075, 5003]


CHILD = r"""
import sys, ctypes as C
sys.path.insert(0, %r)
import foo_dsp_resampler_amd as F
L = F.lib()
cb = F.ratelib._ALLOC_CB(lambda: None)
p = 0x10000  # never dereferenced: every call below is answered from its arguments, or from the library's state, alone
co = (C.c_double * 128)(*([0.25] * 128))
bad = (C.c_double * 48)(*([0.25] * 47 + [float("inf")]))
kw = (C.c_double * 10)(*F.k_weighting(48000))
kbad = (C.c_double * 10)(*([float("nan")] + [0.5] * 9))
vp = lambda a: C.cast(a, C.c_void_p)
tgood = dict(device=-1, stream=None, table=p, ntracks=3, nch=2, sf=16, src=p, total=9000, most=4096, gain=None, coefs=vp(co), phases=4, taps=12, tp=p, pk=p)
def tcall(**k):
    a = dict(tgood, **k)
    return L.RRX_tracks_true_peak_packed_device(a["device"], a["stream"], a["table"], a["ntracks"], a["nch"], a["sf"], a["src"], a["total"], a["most"],
                                                a["gain"], a["coefs"], a["phases"], a["taps"], a["tp"], a["pk"])
lgood = dict(device=-1, stream=None, table=p, ntracks=3, nch=2, sf=16, src=p, total=9000, most=4096, gain=None, coefs=vp(kw), hop=100, e=p, es=40, hops=p,
             work=p, wd=3 * 2 * 40 * 4)
def lcall(**k):
    a = dict(lgood, **k)
    return L.RRX_tracks_loudness_packed_device(a["device"], a["stream"], a["table"], a["ntracks"], a["nch"], a["sf"], a["src"], a["total"], a["most"],
                                               a["gain"], a["coefs"], a["hop"], a["e"], a["es"], a["hops"], a["work"], a["wd"])
print("uninit", tcall(), lcall())                          # before init_ratelib
print("init", L.init_ratelib(cb))                          # no device: refuses
print("uninit", tcall(), tcall(most=0), tcall(total=0), lcall(), lcall(most=0, wd=0, work=None), lcall(total=0))
for name, k in [("table", dict(table=None)), ("src", dict(src=None)), ("ntracks0", dict(ntracks=0)), ("ntracks-1", dict(ntracks=-1)), ("nch0", dict(nch=0)),
                ("nch-1", dict(nch=-1)), ("double", dict(sf=1)), ("fmt7", dict(sf=7)), ("fmt8", dict(sf=8)), ("nothing", dict(tp=None, pk=None)),
                ("coefs", dict(coefs=None)), ("phases0", dict(phases=0)), ("phases9", dict(phases=9)), ("taps0", dict(taps=0)), ("taps17", dict(taps=17)),
                ("inf", dict(coefs=vp(bad))), ("total2^60", dict(total=2**59)), ("rows2^60", dict(most=2**58)), ("rows2^60b", dict(ntracks=2**20, most=2**39)),
                ("device-2", dict(device=-2))]:
    print("tinv", name, tcall(**k))
for name, k in [("float", dict(sf=0)), ("s24", dict(sf=24)), ("s32", dict(sf=32)), ("tp-only", dict(pk=None)), ("pk-only", dict(tp=None)), ("gain", dict(gain=p)),
                ("3x5", dict(phases=3, taps=5)), ("below2^60", dict(total=2**59 - 1)), ("rows-below", dict(most=(2**60 - 1) // 6))]:
    print("tok", name, tcall(**k))
for name, k in [("table", dict(table=None)), ("src", dict(src=None)), ("ntracks0", dict(ntracks=0)), ("nch0", dict(nch=0)), ("double", dict(sf=1)),
                ("fmt7", dict(sf=7)), ("energy", dict(e=None)), ("hops", dict(hops=None)), ("coefs", dict(coefs=None)), ("nan", dict(coefs=vp(kbad))),
                ("hop0", dict(hop=0)), ("work-short", dict(wd=3 * 2 * 40 * 4 - 1)), ("work-null", dict(work=None)), ("total2^60", dict(total=2**59)),
                ("rows2^60", dict(most=2**58, wd=2**62)), ("energy2^60", dict(es=2**58)), ("device-2", dict(device=-2))]:
    print("linv", name, lcall(**k))
for name, k in [("float", dict(sf=0)), ("s24", dict(sf=24)), ("s32", dict(sf=32)), ("gain", dict(gain=p)), ("short-energy", dict(es=1)),
                ("no-hop-fits", dict(most=99, wd=0, work=None)), ("hop17", dict(hop=17, wd=3 * 2 * (4096 // 17) * 4))]:
    print("lok", name, lcall(**k))
"""


def test_invalid_parameters_are_refused_without_a_device():
    out = subprocess.run([sys.executable, "-c", CHILD % ROOT], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))
    assert out.returncode == 0, out.stderr
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.split() and ln.split()[0] in ("uninit", "init", "tinv", "tok", "linv", "lok")]
    assert ["init", "-1"] in lines
    uninit = [ln for ln in lines if ln[0] == "uninit"]
    assert len(uninit) == 2 and all(int(v) == RR_EXTUNINIT for ln in uninit for v in ln[1:])
    for kind, count, want in (("tinv", 20, RR_INVPARAM), ("tok", 9, RR_EXTUNINIT), ("linv", 17, RR_INVPARAM), ("lok", 7, RR_EXTUNINIT)):
        got = [ln for ln in lines if ln[0] == kind]
        assert len(got) == count and all(int(ln[2]) == want for ln in got), got


def test_host_twins_refuse_as_the_device_calls_do_and_leave_the_results_alone():
    raw, _ = S.source("s16", [5, 7], 2, 1)
    table = S.table_of([5, 7])
    tp, pk = np.full((2, 2), 5, np.uint64), np.full((2, 2), 6, np.uint64)
    co = np.ascontiguousarray(S.BS1770)
    tfn, lfn = F.lib().RRX_debug_tracks_true_peak_packed_host, F.lib().RRX_debug_tracks_loudness_packed_host

    def tcall(**k):
        c = k.get("coefs", co)
        return tfn(k.get("table", table.ctypes.data), k.get("n", 2), k.get("nch", 2), k.get("sf", 16), k.get("src", raw.ctypes.data), k.get("total", 12),
                   k.get("most", 7), None, S.ptr(c), k.get("phases", 4), k.get("taps", 12), tp.ctypes.data if k.get("tp", True) else None,
                   pk.ctypes.data if k.get("pk", True) else None)

    inf = co.copy()
    inf[1, 5] = np.inf
    for k in (dict(table=None), dict(src=None), dict(n=0), dict(nch=0), dict(sf=1), dict(sf=7), dict(tp=False, pk=False), dict(coefs=None), dict(phases=9),
              dict(taps=17), dict(coefs=inf), dict(total=2 ** 59), dict(most=2 ** 59)):
        assert tcall(**k) == RR_INVPARAM, k
        assert np.all(tp == 5) and np.all(pk == 6), k
    for k in (dict(most=0), dict(total=0)):  # nothing to do: nothing is touched
        assert tcall(**k) == RR_OK and np.all(tp == 5) and np.all(pk == 6), k

    energy, hops, work = np.full((2, 2, 3), 7.0), np.full(2, 9, np.uint64), np.zeros(2 * 2 * 3 * 4)

    def lcall(**k):
        c = k.get("coefs", S.KW48)
        return lfn(k.get("table", table.ctypes.data), k.get("n", 2), k.get("nch", 2), k.get("sf", 16), k.get("src", raw.ctypes.data), k.get("total", 12),
                   k.get("most", 7), None, S.ptr(c), k.get("hop", 2), energy.ctypes.data if k.get("e", True) else None, k.get("es", 3),
                   hops.ctypes.data if k.get("hops", True) else None, work.ctypes.data if k.get("work", True) else None, k.get("wd", work.size))

    nan = S.KW48.copy()
    nan[3] = np.nan
    for k in (dict(table=None), dict(src=None), dict(n=0), dict(nch=0), dict(sf=1), dict(sf=7), dict(e=False), dict(hops=False), dict(coefs=None),
              dict(coefs=nan), dict(hop=0), dict(wd=work.size - 1), dict(work=False), dict(total=2 ** 59), dict(most=2 ** 59, wd=2 ** 62), dict(es=2 ** 59)):
        assert lcall(**k) == RR_INVPARAM, k
        assert np.all(energy == 7.0) and np.all(hops == 9), k
    for k in (dict(most=0), dict(total=0)):
        assert lcall(**k) == RR_OK and np.all(energy == 7.0) and np.all(hops == 9), k
    assert lcall() == RR_OK and list(hops) == [2, 3] and np.all(energy[0, :, 2] == 7.0) and not np.any(energy[1] == 7.0)

    code = ("import sys; sys.path.insert(0, %r)\nimport foo_dsp_resampler_amd as F\nL = F.lib()\n"
            "print(L.RRX_debug_tracks_true_peak_packed_host(None, 1, 1, 16, None, 0, 0, None, None, 4, 12, None, None),"
            " L.RRX_debug_tracks_loudness_packed_host(None, 1, 1, 16, None, 0, 0, None, None, 1, None, 0, None, None, 0))\n" % ROOT)
    env = {k: v for k, v in os.environ.items() if k != "RSMP_TEST_HOOKS"}
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-2:] == ["-1", "-1"]


@pytest.mark.parametrize("with_gain", [False, True], ids=["unity", "gain"])
@pytest.mark.parametrize("filt", ["bs1770", "3x5"])
@pytest.mark.parametrize("nch", [1, 2, 3])
@pytest.mark.parametrize("kind", list(S.KINDS))
def test_true_peak_twin_equals_one_stream_calls_on_the_exact_doubles(kind, nch, filt, with_gain):
    coefs = S.FILTERS[filt]
    lens = S.lengths(coefs.shape[1])
    raw, exact = S.source(kind, lens, nch, 10 * nch + len(filt))
    table = S.table_of(lens)
    gain = S.gains(len(lens)) if with_gain else None
    rc, tp, pk = S.host_true_peak(kind, raw, table, nch, max(lens), gain, coefs)
    assert rc == RR_OK
    want_tp, want_pk = S.ref_true_peak(exact, S.cuts_of(table, raw.shape[0], max(lens)), nch, gain, coefs)
    assert np.array_equal(tp, want_tp) and np.array_equal(pk, want_pk)
    assert not tp[0].any() and not pk[0].any() and pk[1:].all()  # a track without frames leaves nothing
    if kind == "s24" and nch == 1 and filt == "bs1770":  # mono with odd lengths: tracks begin at all four byte offsets
        assert {int(e[0]) * 3 % 4 for e in table} == {0, 1, 2, 3}


@pytest.mark.parametrize("with_gain", [False, True], ids=["unity", "gain"])
@pytest.mark.parametrize("hop", S.HOPS)
@pytest.mark.parametrize("nch", [1, 2, 3])
@pytest.mark.parametrize("kind", list(S.KINDS))
def test_loudness_twin_equals_one_stream_calls_on_the_exact_doubles(kind, nch, hop, with_gain):
    lens = S.hop_lengths(hop)
    raw, exact = S.source(kind, lens, nch, 100 * nch + hop)
    table = S.table_of(lens)
    gain = S.gains(len(lens)) if with_gain else None
    rc, energy, hops = S.host_loudness(kind, raw, table, nch, max(lens), hop, gain)
    assert rc == RR_OK
    want_e, want_h = S.ref_loudness(exact, S.cuts_of(table, raw.shape[0], max(lens)), nch, hop, max(lens) // hop, gain)
    assert list(hops) == list(want_h) == [0, 4, 4, 0, 1531 // hop]
    assert np.array_equal(energy.view(np.uint64), want_e.view(np.uint64))
    assert np.all(energy[1, :, 4:] == S.GUARD) and np.all(energy[0] == S.GUARD)  # beyond a track's hops: untouched


def test_edge_values_are_the_exact_ones():
    one = np.float64(1.0).view(np.uint64)
    for kind, value, want in (("s32", 2 ** 31 - 1, 1.0 - 2.0 ** -31), ("s32", -2 ** 31, 1.0), ("s16", -32768, 1.0), ("s24", -2 ** 23, 1.0),
                              ("s16", 32767, 1.0 - 2.0 ** -15), ("s24", 2 ** 23 - 1, 1.0 - 2.0 ** -23)):
        raw, exact = S.store(kind, np.array([[0], [value], [0]]))
        if kind == "s24" and value < 0:
            assert list(raw[1]) == [0x00, 0x00, 0x80]
        rc, tp, pk = S.host_true_peak(kind, raw, S.table_of([3]), 1, 3)
        assert rc == RR_OK
        assert as_double(pk)[0, 0] == want == abs(exact[1, 0]), (kind, value)
        assert (pk[0, 0] == one) == (want == 1.0)
    # float32 is taken as it is: a value that float32 holds and the integer grids do not
    raw, exact = S.store("f32", np.array([[np.float32(1.0) + np.float32(2.0 ** -23)]]))
    rc, tp, pk = S.host_true_peak("f32", raw, S.table_of([1]), 1, 1)
    assert rc == RR_OK and as_double(pk)[0, 0] == 1.0 + 2.0 ** -23
    # and the stage pass's float32 value of INT32_MAX is 1.0: the two conversions differ on purpose
    raw, _ = S.store("s32", np.array([[2 ** 31 - 1]]))
    out = np.zeros(1, np.float32)
    assert F.lib().RRX_debug_tracks_load_host(F.RRX_FMT_S32, raw.ctypes.data, 0, 1, out.ctypes.data) == RR_OK and out[0] == 1.0


@pytest.mark.parametrize("kind", list(S.KINDS))
def test_hostile_tables_give_the_clamped_tracks_numbers(kind):
    nch, hop, total = 2, 16, 700
    raw, exact = S.source(kind, [total], nch, 42)
    big = 2 ** 64 - 1
    table = np.zeros((6, 6), np.uint64)
    table[0, :2] = (total + 5, 10)     # begins beyond the source: nothing
    table[1, :2] = (600, 10 ** 9)      # runs past the source: [600, 700)
    table[2, :2] = (0, 650)            # longer than max_frames: [0, 500)
    table[3, :2] = (big, big)          # nothing, and no sum wraps
    table[4, :2] = (650, big)          # [650, 700)
    table[5, :2] = (100, 300)          # a right entry
    most = 500
    want_cuts = [(total, 0), (600, 100), (0, 500), (total, 0), (650, 50), (100, 300)]
    assert S.cuts_of(table, total, most) == want_cuts
    rc, tp, pk = S.host_true_peak(kind, raw, table, nch, most)
    assert rc == RR_OK
    want_tp, want_pk = S.ref_true_peak(exact, want_cuts, nch)
    assert np.array_equal(tp, want_tp) and np.array_equal(pk, want_pk)
    rc, energy, hops = S.host_loudness(kind, raw, table, nch, most, hop)
    assert rc == RR_OK
    want_e, want_h = S.ref_loudness(exact, want_cuts, nch, hop, most // hop)
    assert list(hops) == list(want_h) == [0, 6, 31, 0, 3, 18]
    assert np.array_equal(energy.view(np.uint64), want_e.view(np.uint64))


def test_hops_are_clamped_to_the_energy_stride():
    nch, hop, lens = 2, 17, [17 * 9 + 3, 17 * 2, 5]
    raw, exact = S.source("s24", lens, nch, 7)
    table = S.table_of(lens)
    rc, energy, hops = S.host_loudness("s24", raw, table, nch, max(lens), hop, stride=4)
    assert rc == RR_OK and list(hops) == [4, 2, 0]
    want_e, _ = S.ref_loudness(exact, S.cuts_of(table, raw.shape[0], max(lens)), nch, hop, 4)
    assert np.array_equal(energy.view(np.uint64), want_e.view(np.uint64))
    assert np.all(energy[1, :, 2:] == S.GUARD) and np.all(energy[2] == S.GUARD) and not np.any(energy[0] == S.GUARD)


def test_results_accumulate_as_in_the_row_form():
    raw, exact = S.source("s16", [40], 2, 9)
    huge = np.full((1, 2), np.float64(5.0).view(np.uint64), np.uint64)
    rc, tp, pk = S.host_true_peak("s16", raw, S.table_of([40]), 2, 40, tp=huge.copy(), pk=np.zeros((1, 2), np.uint64))
    assert rc == RR_OK and np.array_equal(tp, huge) and pk.all()


def test_packed_plan_and_the_python_argument_checks():
    plan = F.packed_plan([3, 0, 5])
    assert plan.array().tolist() == [[0, 3, 0, 0, 0, 0], [3, 0, 0, 0, 0, 0], [3, 5, 0, 0, 0, 0]]
    assert (plan.src_total, plan.max_frames, len(plan)) == (8, 5, 3)
    with pytest.raises(ValueError):
        F.packed_plan([])
    with pytest.raises(ValueError):
        F.packed_plan([4, -1])
    with pytest.raises(ValueError):
        F.packed_plan([2 ** 59, 2 ** 59])

    class Fake:  # stands in for a device tensor: the wrapper must refuse before any C call
        def __init__(self, shape, dtype="torch.int16", contiguous=True, cuda=True, device="cuda:0"):
            self.shape, self.dtype, self._c, self.is_cuda, self.device = shape, dtype, contiguous, cuda, device

        def dim(self):
            return len(self.shape)

        def is_contiguous(self):
            return self._c

        def data_ptr(self):
            raise AssertionError("the arguments are checked before the pointer is taken")

    table = Fake((3, 6), dtype="torch.int64")
    for fn in (F.tracks_true_peak_packed_device, lambda *a, **k: F.tracks_loudness_packed_device(*a, rate=48000, **k)):
        with pytest.raises(ValueError):
            fn(Fake((100, 2)), table)  # a bare table does not say max_frames
        with pytest.raises(ValueError):
            fn(Fake((100, 2)), table, max_frames=-1)
        with pytest.raises(TypeError):
            fn(Fake((100, 2), dtype="torch.float64"), table, max_frames=10)  # no source format
        with pytest.raises(TypeError):
            fn(Fake((100, 2), contiguous=False), table, max_frames=10)
        with pytest.raises(TypeError):
            fn(Fake((100, 2), cuda=False), table, max_frames=10)
        with pytest.raises(TypeError):
            fn(Fake((200,)), table, max_frames=10)
        with pytest.raises(ValueError):
            fn(Fake((100, 4), dtype="torch.uint8"), table, max_frames=10)  # packed 24 bit is nch * 3 bytes a frame
        with pytest.raises(TypeError):
            fn(Fake((100, 2)), Fake((3, 5), dtype="torch.int64"), max_frames=10)
        with pytest.raises(TypeError):
            fn(Fake((100, 2)), Fake((3, 6), dtype="torch.int64", device="cuda:1"), max_frames=10)
    with pytest.raises(ValueError):
        F.tracks_true_peak_packed_device(Fake((100, 2)), table, max_frames=10, filter="bs1771")
    with pytest.raises(ValueError):
        F.tracks_loudness_packed_device(Fake((100, 2)), table, max_frames=10)  # neither a rate nor coefs and hop
    with pytest.raises(ValueError):
        F.scan_tracks_pcm([], 48000)
    with pytest.raises(TypeError):
        F.scan_tracks_pcm([Fake((10, 2)), Fake((10, 3))], 48000)
    with pytest.raises(ValueError):
        F.scan_tracks_pcm([Fake((10, 2)), Fake((10, 2))], 48000, album=[0])
