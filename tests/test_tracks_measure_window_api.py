"""True peak and loudness in the windowed track path, host side (RRX_tracks_true_peak_window_device,
RRX_tracks_loudness_window_device and their host twins; DESIGN.md 11, "Windows with true peak and loudness"): the symbols and the
Python names, every refusal that needs no device, and the arithmetic -- the host twins are serial loops per (track, channel) over
the very functions the kernels call -- against what the whole-row calls are documented to equal: a one-stream
RRX_debug_true_peak_host / RRX_debug_loudness_host per track on its slice (first_frame = 0, no state, flush), itself held to
true_peak_model / loudness_model.  Windows are walked in ascending order with two state buffers handed to and fro.  CPU only."""
import inspect
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import foo_dsp_resampler_amd as F
import measure_window_cases as MW
import shaped_window_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RR_OK, RR_EXTUNINIT, RR_INVPARAM = 0, 5, 6
NEW = ("RRX_tracks_true_peak_window_device", "RRX_debug_tracks_true_peak_window_host", "RRX_tracks_loudness_window_work_doubles",
       "RRX_tracks_loudness_window_device", "RRX_debug_tracks_loudness_window_host")
HOPS = (1, 7, 64, 100, 333, 1000)
N = len(W.SLICES)


def u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_symbols_and_names_are_there():
    header = open(os.path.join(ROOT, "include", "ratelib_amd.h")).read()
    for name in NEW:
        assert name in F.EXPECTED_SYMBOLS and name in F.available_symbols()
        assert name in header
    assert "A form by windows is not offered" not in header and "#define RRX_LOUDNESS_WIN_STATE 16" in header
    assert F.RRX_LOUDNESS_WIN_STATE == 16
    for name in ("tracks_true_peak_window_device", "tracks_loudness_window_device"):
        assert callable(getattr(F, name)) and name in F.__all__
    ps = inspect.signature(F.tracks_true_peak_window_device).parameters
    assert list(ps) == ["win", "table", "row_frames", "win_first", "win_frames", "gain", "filter", "state", "true_peak", "peak", "stream"]
    assert ps["filter"].default == "bs1770" and ps["state"].default is None
    ps = inspect.signature(F.tracks_loudness_window_device).parameters
    assert list(ps) == ["win", "table", "row_frames", "win_first", "win_frames", "rate", "gain", "coefs", "hop", "state", "energy", "hops", "work",
                        "stream"]
    ps = inspect.signature(F.Resampler.convert_tracks_to_pcm_streamed_normalized).parameters
    assert list(ps) == ["self", "tracks", "dst_format", "target_dbtp", "window", "shaping", "segment", "dither", "seed"]
    assert ps["target_dbtp"].default == -1.0 and ps["segment"].default == 65536 and ps["dither"].default is False
    ps = inspect.signature(F.Resampler.convert_tracks_to_pcm_streamed_loudness_normalized).parameters
    assert list(ps) == ["self", "tracks", "dst_format", "target_lufs", "max_dbtp", "weights", "window", "shaping", "segment", "dither", "seed", "album"]
    assert ps["target_lufs"].default == -18.0 and ps["max_dbtp"].default == -1.0 and ps["album"].default is None
    # the existing streamed methods keep their signatures
    ps = inspect.signature(F.Resampler.convert_tracks_to_pcm_streamed).parameters
    assert list(ps) == ["self", "tracks", "dst_format", "window", "_scratch", "shaping", "segment", "finish_kw"]


def test_work_size_is_its_formula():
    fn = F.lib().RRX_tracks_loudness_window_work_doubles
    for n, nch, wn, hop in ((1, 1, 0, 1), (5, 2, 4099, 4410), (5, 2, 4410, 4410), (3, 7, 700, 7), (64, 2, 65536, 4800), (2, 2, 13, 8)):
        assert fn(n, nch, wn, hop) == n * nch * (wn // hop + 2) * 4
    for bad in ((0, 2, 10, 5), (-1, 2, 10, 5), (2, 0, 10, 5), (2, 2, 10, 0)):
        assert fn(*bad) == 0


TP_CASES = list(itertools.product(MW.FILTERS, (1, 2, 3)))


@pytest.mark.parametrize("j", range(len(TP_CASES)), ids=["%s-%dch" % c for c in TP_CASES])
def test_true_peak_over_windows_equals_the_whole_row_reference(j):
    """every (filter, channel count) pair under every partition, float32 / float64 and the gains going round beside them"""
    name, nch = TP_CASES[j]
    double, gains = bool((j + j // 3) % 2), (MW.GAINS if (j // 2 + j // 3) % 2 else None)
    x = MW.rows_of(N, nch, double)
    tab, _ = W.table_of()
    want = MW.tp_reference(x, tab, MW.FILTERS[name], gains)
    assert not want[0][2].any() and not want[2][2].any()      # the zero-length track: no peak, no history
    assert want[0][[0, 1, 3, 4]].all() and want[1][[0, 1, 3, 4]].all()
    for pname, part in W.PARTITIONS.items():
        got = MW.tp_host_windows(x, tab, part, MW.FILTERS[name], gains)
        what = (name, nch, double, gains is not None, pname)
        assert np.array_equal(got[0], want[0]), ("true peak",) + what
        assert np.array_equal(got[1], want[1]), ("peak",) + what
        assert np.array_equal(u64(got[2]), u64(want[2])), ("state",) + what


def test_true_peak_axes_are_all_met():
    seen = set()
    for j in range(len(TP_CASES)):
        seen.add(("double", bool((j + j // 3) % 2)))
        seen.add(("gain", bool((j // 2 + j // 3) % 2)))
    assert len(seen) == 4


LD_CASES = [(hop, nch) for hop in HOPS for nch in (1, 2, 3)]


@pytest.mark.parametrize("j", range(len(LD_CASES)), ids=["hop%d-%dch" % c for c in LD_CASES])
def test_loudness_over_windows_equals_the_whole_row_reference(j):
    """every hop -- shorter and longer than the windows, spanning three of them, longer than most slices -- under every partition"""
    hop, nch = LD_CASES[j]
    double, gains = bool((j + j // 3) % 2), (MW.GAINS if (j // 2 + j // 3) % 2 else None)
    x = MW.rows_of(N, nch, double)
    tab, _ = W.table_of()
    stride = W.R // hop
    want = MW.ld_reference(x, tab, hop, gains, stride)
    assert list(want[1]) == [n // hop for _, n in W.SLICES]
    for pname, part in W.PARTITIONS.items():
        got = MW.ld_host_windows(x, tab, part, hop, gains, stride)
        what = (hop, nch, double, gains is not None, pname)
        assert np.array_equal(u64(got[0]), u64(want[0])), ("energies",) + what
        assert np.array_equal(got[1], want[1]), ("hops",) + what
        assert np.array_equal(u64(got[2]), u64(want[2])), ("state",) + what


@pytest.mark.parametrize("hop,stride", [(7, 40), (64, 3), (100, 1), (333, 0 + 1)])
def test_loudness_energy_stride_smaller_than_the_hop_count(hop, stride):
    x = MW.rows_of(N, 2, False)
    tab, _ = W.table_of()
    want = MW.ld_reference(x, tab, hop, MW.GAINS, stride)
    assert max(n // hop for _, n in W.SLICES) > stride and int(want[1].max()) == stride
    for pname, part in W.PARTITIONS.items():
        got = MW.ld_host_windows(x, tab, part, hop, MW.GAINS, stride)
        assert np.array_equal(u64(got[0]), u64(want[0])) and np.array_equal(got[1], want[1]), (hop, stride, pname)
        assert np.array_equal(u64(got[2]), u64(want[2])), ("state", hop, stride, pname)


def test_non_finite_samples_stay_in_their_channel():
    """a NaN and an infinity in channel 1 of track 3: that channel's results are NaN / inf where the reference's are; every other
    channel is exact"""
    nch, hop = 3, 64
    x = np.array(MW.rows_of(N, nch, False))
    x[3, 450, 1], x[3, 600, 1] = np.nan, np.inf
    tab, _ = W.table_of()
    bad = np.zeros((N, nch), bool)
    bad[3, 1] = True
    tp_want = MW.tp_reference(x, tab, MW.FILTERS["bs1770"], MW.GAINS)
    ld_want = MW.ld_reference(x, tab, hop, MW.GAINS, W.R // hop)
    assert np.isnan(tp_want[0].view(np.float64)[3, 1]) and np.isnan(ld_want[0][3, 1]).any()
    for pname, part in W.PARTITIONS.items():
        tp = MW.tp_host_windows(x, tab, part, MW.FILTERS["bs1770"], MW.GAINS)
        for k in (0, 1):
            assert np.array_equal(tp[k][~bad], tp_want[k][~bad]), (pname, k)
            g, w = tp[k].view(np.float64)[bad], tp_want[k].view(np.float64)[bad]
            assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(np.isinf(g), np.isinf(w)), (pname, k)
        assert np.array_equal(u64(tp[2][~bad]), u64(tp_want[2][~bad])), pname
        ld = MW.ld_host_windows(x, tab, part, hop, MW.GAINS, W.R // hop)
        assert np.array_equal(u64(ld[0][~bad]), u64(ld_want[0][~bad])) and np.array_equal(ld[1], ld_want[1]), pname
        assert np.array_equal(np.isnan(ld[0][bad]), np.isnan(ld_want[0][bad])), pname
        assert np.array_equal(np.isinf(ld[0][bad]), np.isinf(ld_want[0][bad])), pname
        assert np.array_equal(u64(ld[2][~bad]), u64(ld_want[2][~bad])), pname


def test_windows_out_of_order_give_other_numbers_and_stay_inside():
    """the ordering rule: the windows of a partition in reverse are answered RR_OK, write nothing outside the buffers (the callers
    look at the guards) and leave other numbers than the ordered walk"""
    x = MW.rows_of(N, 2, False)
    tab, _ = W.table_of()
    back = W.PARTITIONS["333"][::-1]
    want = MW.tp_host_windows(x, tab, W.PARTITIONS["333"], MW.FILTERS["bs1770"], None)
    got = MW.tp_host_windows(x, tab, back, MW.FILTERS["bs1770"], None)
    assert np.array_equal(got[1], want[1])                      # the sample peak does not depend on the history
    assert not np.array_equal(u64(got[2]), u64(want[2]))
    want = MW.ld_host_windows(x, tab, W.PARTITIONS["333"], 100, None, 7)
    got = MW.ld_host_windows(x, tab, back, 100, None, 7)
    assert np.array_equal(got[1], want[1]) and not np.array_equal(u64(got[0]), u64(want[0]))


def test_wrong_tables_are_clamped_as_in_the_whole_row_calls():
    """out_first and out_frames beyond the row: the whole-row calls' clamped numbers, nothing written outside the buffers"""
    x = MW.rows_of(N, 2, True)
    tab, _ = W.table_of()
    wrong = tab.copy()
    wrong[-1] = (0, 0, 0, 650, 2 ** 40, 0)
    wrong[1] = (0, 0, 0, 2 ** 63, 130, 7)
    wrong[0] = (0, 0, 0, 2 ** 64 - 1, 2 ** 64 - 1, 0)
    assert MW.slices_of(wrong, W.R) == [(0, 0), (0, 0), (0, 0), (400, 690), (650, 700)]
    tp_want = MW.tp_reference(x, wrong, MW.FILTERS["bs1770"], MW.GAINS)
    ld_want = MW.ld_reference(x, wrong, 7, MW.GAINS, 100)
    for pname in ("7", "333", "on segment boundaries"):
        tp = MW.tp_host_windows(x, wrong, W.PARTITIONS[pname], MW.FILTERS["bs1770"], MW.GAINS)
        assert all(np.array_equal(u64(a), u64(b)) for a, b in zip(tp, tp_want)), pname
        ld = MW.ld_host_windows(x, wrong, W.PARTITIONS[pname], 7, MW.GAINS, 100)
        assert all(np.array_equal(u64(a), u64(b)) for a, b in zip(ld, ld_want)), pname


def test_host_twins_refuse_and_empty_calls_touch_nothing():
    n, nch = 3, 2
    tab = np.ascontiguousarray(W.table_of([(0, 40), (3, 30), (9, 0)])[0])
    win = np.zeros((n, 12, nch), np.float32)
    st = np.full((2, n, nch, 16), MW.SENTINEL)
    flat = st.reshape(-1)
    tp, pk = np.zeros((n, nch), np.uint64), np.zeros((n, nch), np.uint64)
    energy, hops, work = np.full((n, nch, 10), MW.GUARD), np.full(n, 0xdead, np.uint64), np.full(MW.work_doubles(n, nch, 10, 5), MW.GUARD)
    k = MW.FILTERS["bs1770"]
    tbase = dict(tab=tab, win=win, rows=50, wf=10, wn=10, gains=None, coefs=k, sin=st[0], sout=st[1], tp=tp, pk=pk)
    lbase = dict(tab=tab, win=win, rows=50, wf=10, wn=10, gains=None, hop=5, sin=st[0], sout=st[1], energy=energy, stride=10, hops=hops, work=work)
    states = (dict(sin=None), dict(sin=None, wn=0), dict(sin=st[0], sout=st[0]), dict(sin=flat[8:], sout=flat),
              dict(sin=flat, sout=flat[n * nch * 16 - 1:]))
    windows = (dict(wf=45), dict(wn=13), dict(wf=2 ** 64 - 5), dict(tab=None), dict(win=None, shape=win.shape))
    for kw in windows + states + (dict(tp=None, pk=None), dict(coefs=np.array([[1.0, np.nan]])), dict(coefs=None, phases=4, taps=12),
                                  dict(phases=0), dict(phases=9), dict(taps=0), dict(taps=17)):
        MW.tp_host_call(rc=RR_INVPARAM, **dict(tbase, **kw))
    nanc = np.array(MW.K)
    nanc[3] = np.inf
    for kw in windows + states + (dict(energy=None), dict(hops=None), dict(hop=0), dict(c=None), dict(c=nanc), dict(work=None),
                                  dict(work_doubles=work.size - 1), dict(stride=2 ** 58)):
        MW.ld_host_call(rc=RR_INVPARAM, **dict(lbase, **kw))
    untouched = lambda: (not tp.any() and not pk.any() and (st == MW.SENTINEL).all() and (energy == MW.GUARD).all()
                         and (hops == 0xdead).all() and (work == MW.GUARD).all())
    assert untouched()
    # empty windows and empty rows: RR_OK, and nothing is touched, the state included
    for kw in (dict(wn=0), dict(wf=0, wn=0, sin=None), dict(wf=50, wn=0), dict(rows=0, wf=0, wn=0)):
        MW.tp_host_call(rc=RR_OK, **dict(tbase, **kw))
        MW.ld_host_call(rc=RR_OK, **dict(lbase, **kw))
    assert untouched()
    # nothing to refuse: a window at frame 0 without a state, adjacent states, no state out, one statistic
    MW.tp_host_call(**dict(tbase, wf=0, sin=None))
    assert not (st[1] == MW.SENTINEL).any() and not st[1, 2].any()   # every entry written; the zero-length track: zeros
    MW.ld_host_call(**dict(lbase, wf=0, sin=None))
    assert not (st[1] == MW.SENTINEL).any() and not st[1, 2].any() and list(hops) == [8, 6, 0]
    MW.tp_host_call(**dict(tbase, sin=flat[:n * nch * 16], sout=flat[n * nch * 16:]))
    MW.tp_host_call(**dict(tbase, sout=None))
    MW.tp_host_call(**dict(tbase, pk=None))
    MW.ld_host_call(**dict(lbase, sout=None))
    code = ("import sys; sys.path.insert(0, %r)\nimport foo_dsp_resampler_amd as F\nL = F.lib()\n"
            "print(L.RRX_debug_tracks_true_peak_window_host(None, 0, 0, 0, None, 0, 0, 0, 0, None, None, 0, 0, None, None, None, None))\n"
            "print(L.RRX_debug_tracks_loudness_window_host(None, 0, 0, 0, None, 0, 0, 0, 0, None, None, 0, None, None, None, 0, None, None, 0))\n" % ROOT)
    env = {k_: v for k_, v in os.environ.items() if k_ != "RSMP_TEST_HOOKS"}
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-2:] == ["-1", "-1"]


CHILD = r"""
import sys, ctypes as C
sys.path.insert(0, %r)
import foo_dsp_resampler_amd as F
L = F.lib()
p = 0x10000  # never dereferenced: every call below is answered from its arguments, or from the library's state, alone
D = C.c_double
adr = lambda a: C.cast(a, C.c_void_p)
bs = (D * 48)(*F.TRUE_PEAK_FILTERS["bs1770"][2])
knan = (D * 48)(*([0.5] * 47 + [float("nan")]))
k128 = (D * 128)(*([0.1] * 128))
kw = (D * 10)(*F.K_WEIGHTING_48K)
kwinf = (D * 10)(*(list(F.K_WEIGHTING_48K[:9]) + [float("inf")]))
STATE = 3 * 2 * 16 * 8                          # bytes of a state of 3 tracks x 2 channels
WORK = 3 * 2 * (500 // 480 + 2) * 4
tgood = dict(device=-1, stream=None, table=p, ntracks=3, nch=2, sf=0, win=p, stride=512, row_frames=4096, first=100, frames=500, gain=None,
             coefs=adr(bs), phases=4, taps=12, sin=p, sout=p + STATE, tp=p, pk=p)
def tcall(**k):
    a = dict(tgood, **k)
    return L.RRX_tracks_true_peak_window_device(a["device"], a["stream"], a["table"], a["ntracks"], a["nch"], a["sf"], a["win"], a["stride"],
        a["row_frames"], a["first"], a["frames"], a["gain"], a["coefs"], a["phases"], a["taps"], a["sin"], a["sout"], a["tp"], a["pk"])
lgood = dict(device=-1, stream=None, table=p, ntracks=3, nch=2, sf=0, win=p, stride=512, row_frames=4096, first=100, frames=500, gain=None,
             coefs=adr(kw), hop=480, sin=p, sout=p + STATE, energy=p, es=8, hops=p, work=p, wd=WORK)
def lcall(**k):
    a = dict(lgood, **k)
    return L.RRX_tracks_loudness_window_device(a["device"], a["stream"], a["table"], a["ntracks"], a["nch"], a["sf"], a["win"], a["stride"],
        a["row_frames"], a["first"], a["frames"], a["gain"], a["coefs"], a["hop"], a["sin"], a["sout"], a["energy"], a["es"], a["hops"], a["work"],
        a["wd"])
shared = [("table", dict(table=None)), ("win", dict(win=None)), ("ntracks0", dict(ntracks=0)), ("ntracks-1", dict(ntracks=-1)), ("nch0", dict(nch=0)),
          ("sf16", dict(sf=16)), ("sf7", dict(sf=7)), ("device-2", dict(device=-2)), ("rows2^60", dict(row_frames=2**58)),
          # the three window refusals
          ("past-the-row", dict(first=3597)), ("first-past-the-row", dict(first=4097, frames=0)), ("sum-wraps", dict(first=2**64 - 1, frames=2)),
          ("sum-wraps-to-0", dict(first=2**64 - 500)), ("stride", dict(stride=499)), ("stride0", dict(stride=0)), ("window2^60", dict(stride=2**58)),
          ("empty-past-the-row", dict(first=5000, frames=0)),
          # the two state rules
          ("no-state-behind-0", dict(sin=None)), ("no-state-at-1", dict(sin=None, first=1)), ("no-state-empty-window", dict(sin=None, frames=0)),
          ("state-equal", dict(sout=p)), ("state-overlap-above", dict(sout=p + STATE - 8)), ("state-overlap-below", dict(sin=p + 8, sout=p)),
          ("state-equal-at-0", dict(first=0, sout=p))]
for name, k in shared + [("no-result", dict(tp=None, pk=None)), ("coefs-null", dict(coefs=None)), ("phases0", dict(phases=0)),
                         ("phases9", dict(phases=9)), ("taps0", dict(taps=0)), ("taps17", dict(taps=17)), ("coef-nan", dict(coefs=adr(knan)))]:
    print("inv", "tp-" + name, tcall(**k))
for name, k in shared + [("energy", dict(energy=None)), ("hops", dict(hops=None)), ("coefs-null", dict(coefs=None)), ("hop0", dict(hop=0)),
                         ("coef-inf", dict(coefs=adr(kwinf))), ("es2^60", dict(es=2**58)), ("work-small", dict(wd=WORK - 1)),
                         ("work-null", dict(work=None)), ("work-for-a-shorter-hop", dict(hop=100))]:
    print("inv", "ld-" + name, lcall(**k))
ok = [("good", dict()), ("double", dict(sf=1)), ("whole-row", dict(first=0, frames=4096, stride=4096)), ("last-frame", dict(first=4095, frames=1)),
      ("win_frames0", dict(frames=0)), ("row_frames0", dict(row_frames=0, first=0, frames=0)), ("no-state-at-0", dict(sin=None, first=0)),
      ("no-state-at-0-empty", dict(sin=None, first=0, frames=0)), ("no-state-out", dict(sout=None)),
      ("states-adjacent-below", dict(sin=p + STATE, sout=p))]
for name, k in ok + [("one-result", dict(pk=None)), ("1x1", dict(phases=1, taps=1)), ("8x16", dict(coefs=adr(k128), phases=8, taps=16))]:
    print("ok", "tp-" + name, tcall(**k))
for name, k in ok[:2] + ok[4:] + [("hop1", dict(hop=1, wd=3 * 2 * 502 * 4)), ("window-shorter-than-a-hop", dict(hop=4410)),
                                  ("whole-row", dict(first=0, frames=4096, stride=4096, wd=3 * 2 * 10 * 4)), ("es0", dict(es=0))]:
    print("ok", "ld-" + name, lcall(**k))                     # nothing to refuse: answered RR_EXTUNINIT before init_ratelib
"""


def test_the_device_calls_refuse_from_their_arguments_alone():
    """RR_INVPARAM comes before RR_EXTUNINIT: in a process that never called init_ratelib (and sees no device) every refusal is
    answered from the arguments, and a call with nothing to refuse -- an empty window among them, which is RR_OK on an initialised
    library -- gets as far as RR_EXTUNINIT and no further."""
    out = subprocess.run([sys.executable, "-c", CHILD % ROOT], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))
    assert out.returncode == 0, out.stderr
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.split() and ln.split()[0] in ("inv", "ok")]
    inv = [ln for ln in lines if ln[0] == "inv"]
    assert len(inv) == 24 + 7 + 24 + 9 and all(int(ln[2]) == RR_INVPARAM for ln in inv), [ln for ln in inv if int(ln[2]) != RR_INVPARAM]
    ok = [ln for ln in lines if ln[0] == "ok"]
    assert len(ok) == 13 + 12 and all(int(ln[2]) == RR_EXTUNINIT for ln in ok), [ln for ln in ok if int(ln[2]) != RR_EXTUNINIT]


def test_python_refusals_need_no_device():
    class Fake:                                              # enough of a tensor to reach the checks that come first
        def __init__(self, dtype, shape, cuda=True):
            self.dtype, self.shape, self.is_cuda = dtype, shape, cuda

        def dim(self):
            return len(self.shape)

        def is_contiguous(self):
            return True

    win = Fake("torch.float32", (2, 10, 2))
    for fn in (F.tracks_true_peak_window_device, F.tracks_loudness_window_device):
        with pytest.raises(TypeError):
            fn(Fake("torch.float32", (2, 10, 2), cuda=False), None, 100, 0, 10)
        with pytest.raises(TypeError):
            fn(Fake("torch.int16", (2, 10, 2)), None, 100, 0, 10)
        for args in ((100, 95, 10), (100, 0, 11), (100, -1, 5),
                     (100, 5, 10), (100, 64, 10)):               # no state behind frame 0
            with pytest.raises(ValueError):
                fn(win, None, *args)
