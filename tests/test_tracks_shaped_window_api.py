"""Noise-shaped dither in the windowed track path, host side (RRX_tracks_finish_shaped_window_device /
RRX_debug_tracks_finish_shaped_window_host; DESIGN.md 11, "Windows with noise shaping"): the symbols and the Python names, every refusal that needs no
device, and the arithmetic -- the host twin is a serial loop per (track, channel) over the very functions the kernel calls --
against shaped_model.model applied per track to its slice with the track's shifted seed, first_frame = 0 and no state, which is
what the whole-row call is documented to equal.  Windows are walked in ascending order with two state buffers handed to and fro.
CPU only."""
import inspect
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import foo_dsp_resampler_amd as F
import finish_model as M
import shaped_model as SM
import shaped_window_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RR_OK, RR_EXTUNINIT, RR_INVPARAM = 0, 5, 6
NEW = ("RRX_tracks_finish_shaped_window_device", "RRX_debug_tracks_finish_shaped_window_host")
ORDERS = (1, 5, 9, 16)
SEGMENTS = (0, 1, 16, 64, 5000)                               # the last is longer than the row
TARGETS = [(f, True) for f in SM.FORMATS] + [(F.RRX_FMT_S16, False)]      # (format, write): the last is measure only
GAINS = 0.5 + 0.4 * np.arange(len(W.SLICES))                  # 2.1 on the last track: clipped samples to count


def test_symbols_and_names_are_there():
    header = open(os.path.join(ROOT, "include", "ratelib_amd.h")).read()
    for name in NEW:
        assert name in F.EXPECTED_SYMBOLS and name in F.available_symbols()
        assert name in header
    assert callable(F.tracks_finish_shaped_window_device) and "tracks_finish_shaped_window_device" in F.__all__
    ps = inspect.signature(F.tracks_finish_shaped_window_device).parameters
    assert list(ps)[:17] == ["win", "table", "row_frames", "win_first", "win_frames", "dst_format", "dst_total", "shaping", "segment", "gain",
                             "dither", "seed", "state", "out", "peak", "clipped", "stream"]
    assert ps["segment"].default == 65536 and ps["dither"].default is True and ps["state"].default is None
    ps = inspect.signature(F.Resampler.convert_tracks_to_pcm_streamed_shaped).parameters
    assert list(ps)[:6] == ["self", "tracks", "dst_format", "shaping", "segment", "window"] and ps["segment"].default == 65536
    ps = inspect.signature(F.Resampler.convert_library_to_pcm_streamed_shaped).parameters
    assert list(ps) == ["self", "tracks", "dst_format", "window", "shaping", "segment", "gain", "dither", "seed"]
    assert ps["dither"].default is True and ps["segment"].default == 65536
    # the names the refusals are pinned under keep their signatures
    for name in ("convert_tracks_to_pcm_streamed", "convert_library_to_pcm"):
        ps = inspect.signature(getattr(F.Resampler, name)).parameters
        assert ps["shaping"].default is None and ps["segment"].default == 65536, name


def test_the_case_is_what_it_is_meant_to_be():
    tab, total = W.table_of()
    assert total == sum(n for _, n in W.SLICES) and len({of for of, _ in W.SLICES}) == len(W.SLICES)
    for name, part in W.PARTITIONS.items():
        assert part[0][0] == 0 and sum(n for _, n in part) == W.R and all(a + n == b for (a, n), (b, _) in zip(part, part[1:])), name
        if len(part) > 1:
            assert W.SLICES[3][0] >= part[1][0], name                                     # a track begins after the first window
            assert W.SLICES[1][0] + W.SLICES[1][1] <= part[-1][0] or name == "16 singles", name   # and one ends before the last
    assert all((c - W.SLICES[0][0]) % 64 == 0 for c in W.SEG_CUTS)
    assert any(n == 0 for _, n in W.SLICES) and max(SEGMENTS) > W.R


CASES = list(itertools.product(SEGMENTS, ORDERS))


@pytest.mark.parametrize("j", range(len(CASES)), ids=["seg%d-order%d" % c for c in CASES])
def test_host_twin_over_windows_equals_the_model_of_the_whole_row_call(j):
    """every (segment, order) pair under every partition, with the target format, float32 / float64, the channel count, the gains
    and the dither switch going round beside them so that every value of every axis meets several of the others"""
    segment, order = CASES[j]
    (fmt, write), double, nch = TARGETS[j % 4], bool((j // 4 + j) % 2), 1 + (j + j // 3) % 3
    gains, dith = (GAINS if (j // 2 + j // 5) % 2 else None), bool((j + j // 4) % 3)
    x = W.rows_of(len(W.SLICES), nch, fmt, double)
    tab, total = W.table_of()
    coefs = SM.coefs_of(order)
    want = W.whole_model(x, tab, total, fmt, write, coefs, segment, gains, dith)
    assert np.isnan(x).any() and np.isinf(x).any()
    for name, part in W.PARTITIONS.items():
        got = W.host_windows(x, tab, total, part, fmt, write, coefs, segment, gains, dith)
        W.same(got, want, (name, segment, order, fmt, write, double, nch, gains is not None, dith))
    assert not want[3][2].any() and not want[1][2].any()     # the zero-length track: no history, no peak


def test_every_axis_value_is_met():
    seen = {k: set() for k in ("target", "double", "nch", "gain", "dith")}
    for j in range(len(CASES)):
        seen["target"].add(TARGETS[j % 4])
        seen["double"].add(bool((j // 4 + j) % 2))
        seen["nch"].add(1 + (j + j // 3) % 3)
        seen["gain"].add(bool((j // 2 + j // 5) % 2))
        seen["dith"].add(bool((j + j // 4) % 3))
    assert seen == {"target": set(TARGETS), "double": {False, True}, "nch": {1, 2, 3}, "gain": {False, True}, "dith": {False, True}}


@pytest.mark.parametrize("fmt,write", TARGETS, ids=["s16", "s24", "s32", "measure"])
def test_a_zero_filter_is_the_unshaped_window_rule(fmt, write):
    """order = 1, coefs = [0.0]: per window, the frames the unshaped window call cuts (the restatement of
    tests/test_tracks_window_api.py), finished by finish_model.model at their index in the track -- with and without dither, and
    under a table no plan makes, whose last entry is cut to the row and to the destination"""
    nch = 2
    x = W.rows_of(len(W.SLICES), nch, fmt, False)
    good, total = W.table_of()
    wrong = good.copy()
    wrong[-1] = (0, 0, 0, 650, 2 ** 40, int(good[-1, 5]))
    wrong[1] = (0, 0, 0, 2 ** 63, 130, 7)
    nb = SM.NBYTES[fmt]
    for tab, dith, part in ((good, True, "7"), (good, False, "16 singles"), (wrong, True, "333"), (wrong, True, "on segment boundaries")):
        raw = np.full(total * nch * nb, W.GUARD, np.uint8) if write else None
        pk, cl = np.zeros((len(tab), nch), np.uint64), np.zeros((len(tab), nch), np.uint64)
        for wf, wn in W.PARTITIONS[part]:
            for t in range(len(tab)):
                w0, w1, index, df = W.cut_model([int(v) for v in tab[t]], W.R, total, write, wf, wn)
                if w1 > w0:
                    o, p, c = M.model(np.array(x[t, wf + w0:wf + w1])[None], fmt, GAINS[t:t + 1], dith, W.track_seed(t, nch), index)
                    if write:
                        raw[df * nch * nb:(df + w1 - w0) * nch * nb] = o.reshape(-1)
                    pk[t], cl[t] = np.maximum(pk[t], p[0]), cl[t] + c[0]
        got = W.host_windows(x, tab, total, W.PARTITIONS[part], fmt, write, [0.0], 64, GAINS, dith)
        nan = np.zeros(pk.shape, bool)
        for t in range(len(tab)):
            w0, w1, _, _ = W.cut_model([int(v) for v in tab[t]], W.R, total, write, 0, W.R)
            nan[t] = np.isnan(x[t, w0:w1]).any(axis=0)
        W.same(got, (raw, pk, cl, None, nan), (fmt, write, dith, part), state=False)
        assert cl.sum() > 0


def test_windows_out_of_order_give_other_samples_and_stay_inside():
    """the ordering rule: the same windows in descending order, each with a state, are answered RR_OK, write only the destination
    (guard bytes are looked at) and differ from the ascending result"""
    x = W.rows_of(len(W.SLICES), 2, F.RRX_FMT_S16, False)
    tab, total = W.table_of()
    want = W.whole_model(x, tab, total, F.RRX_FMT_S16, True, SM.W9, 64, None, True)
    part = [(a, n) for a, n in W.PARTITIONS["333"][::-1]]
    # (host_windows passes no state to the window at frame 0, which comes last here; its check of untouched tracks still holds)
    got = W.host_windows(x, tab, total, part, F.RRX_FMT_S16, True, SM.W9, 64, None, True)
    assert not np.array_equal(got[0], want[0])
    assert np.array_equal(got[1][~want[4]], want[1][~want[4]])   # the peaks do not depend on the history


def test_host_twin_refusals_and_empty_windows_touch_nothing():
    n, nch = 3, 2
    tab = np.ascontiguousarray(W.table_of([(0, 40), (3, 30), (9, 0)])[0])
    win = np.zeros((n, 12, nch), np.float32)
    k = np.array([1.0, -0.5])
    dst = np.full(70 * nch * 2, W.GUARD, np.uint8)
    pk, cl = np.zeros((n, nch), np.uint64), np.zeros((n, nch), np.uint64)
    st = np.full((2, n, nch, 16), 77.0)
    base = dict(tab=tab, win=win, rows=50, wf=10, wn=10, fmt=F.RRX_FMT_S16, dst=dst, dst_total=70, gains=None, dith=True, seed=1, coefs=k, segment=8,
                sin=st[0], sout=st[1], pk=pk, cl=cl)

    def call(rc, **kw):
        return W.host_call(rc=rc, **dict(base, **kw))

    flat = st.reshape(-1)
    for kw in (dict(tab=None), dict(win=None, shape=win.shape), dict(fmt=0), dict(fmt=8), dict(dst=None, fmt=0), dict(dst=None, pk=None, cl=None),
               dict(coefs=np.array([1.0, np.nan])), dict(coefs=np.zeros(17)), dict(wf=45), dict(wn=13), dict(wf=2 ** 64 - 5),
               dict(sin=None), dict(sin=None, wn=0), dict(sin=st[0], sout=st[0]), dict(sin=flat[8:], sout=flat), dict(sin=flat, sout=flat[n * nch * 16 - 1:])):
        call(RR_INVPARAM, **kw)
    assert (dst == W.GUARD).all() and not pk.any() and not cl.any() and (st == 77.0).all()
    # empty windows and empty rows: RR_OK, and nothing is touched, the state included
    for kw in (dict(wn=0), dict(wf=0, wn=0, sin=None), dict(wf=50, wn=0), dict(rows=0, wf=0, wn=0)):
        call(RR_OK, **kw)
    assert (dst == W.GUARD).all() and not pk.any() and not cl.any() and (st == 77.0).all()
    # nothing to refuse: a window at frame 0 without a state, adjacent states, no state out, measure only
    call(RR_OK, wf=0, sin=None)
    assert not (st[1] == 77.0).any() and not st[1, 2].any()   # every entry written; the zero-length track: zeros
    call(RR_OK, sin=flat[:n * nch * 16], sout=flat[n * nch * 16:])
    call(RR_OK, sout=None)
    call(RR_OK, dst=None)
    code = ("import sys; sys.path.insert(0, %r)\nimport foo_dsp_resampler_amd as F\n"
            "print(F.lib().RRX_debug_tracks_finish_shaped_window_host(None, 0, 0, 0, None, 0, 0, 0, 0, 16, None, 0, None, 0, 0, None, 0, 0, None, None, "
            "None, None))\n" % ROOT)
    env = {k_: v for k_, v in os.environ.items() if k_ != "RSMP_TEST_HOOKS"}
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-1] == "-1"


CHILD = r"""
import sys, ctypes as C
sys.path.insert(0, %r)
import foo_dsp_resampler_amd as F
L = F.lib()
fn = L.RRX_tracks_finish_shaped_window_device
p = 0x10000  # never dereferenced: every call below is answered from its arguments, or from the library's state, alone
D = C.c_double
k3 = (D * 3)(1.623, -0.982, 0.109)
k16 = (D * 16)(*([0.5] * 16))
knan = (D * 3)(1.0, float("nan"), 0.0)
kinf = (D * 2)(1.0, float("-inf"))
adr = lambda a: C.cast(a, C.c_void_p)
STATE = 3 * 2 * 16 * 8                          # bytes of the state of 3 tracks x 2 channels
good = dict(device=-1, stream=None, table=p, ntracks=3, nch=2, sf=0, win=p, stride=512, row_frames=4096, first=100, frames=500, df=16, dst=p,
            dst_total=9000, gain=None, dither=1, seed=7, coefs=adr(k3), order=3, segment=64, sin=p, sout=p + STATE, peak=p, clipped=p)
def call(**kw):
    a = dict(good, **kw)
    return fn(a["device"], a["stream"], a["table"], a["ntracks"], a["nch"], a["sf"], a["win"], a["stride"], a["row_frames"], a["first"],
              a["frames"], a["df"], a["dst"], a["dst_total"], a["gain"], a["dither"], a["seed"], a["coefs"], a["order"], a["segment"], a["sin"],
              a["sout"], a["peak"], a["clipped"])
# what RRX_tracks_finish_window_device refuses, the three window refusals included
window = [("past-the-row", dict(first=3597)), ("first-past-the-row", dict(first=4097, frames=0)), ("sum-wraps", dict(first=2**64 - 1, frames=2)),
          ("sum-wraps-to-0", dict(first=2**64 - 500)), ("frames-wrap", dict(first=1, frames=2**64 - 1, stride=2**64 - 1)),
          ("stride", dict(stride=499)), ("stride0", dict(stride=0)), ("window2^60", dict(stride=2**58)),
          ("window2^60-1track", dict(ntracks=1, nch=1, stride=2**60, row_frames=2**59)),
          ("empty-past-the-row", dict(first=5000, frames=0)), ("empty-stride-wide", dict(frames=0, stride=2**58))]
for name, kw in [("table", dict(table=None)), ("win", dict(win=None)), ("ntracks0", dict(ntracks=0)), ("ntracks-1", dict(ntracks=-1)),
                 ("nch0", dict(nch=0)), ("sf16", dict(sf=16)), ("sf7", dict(sf=7)), ("df0", dict(df=0)), ("df1", dict(df=1)), ("df8", dict(df=8)),
                 ("nothing-to-do", dict(dst=None, peak=None, clipped=None)), ("device-2", dict(device=-2)), ("rows2^60", dict(row_frames=2**58)),
                 ("dst2^60", dict(dst_total=2**59))] + window + [
                 # what RRX_tracks_finish_shaped_device adds
                 ("measure-df0", dict(dst=None, df=0)), ("measure-df8", dict(dst=None, df=8)), ("coefs-null", dict(coefs=None)),
                 ("order0", dict(order=0)), ("order-1", dict(order=-1)), ("order17", dict(coefs=adr(k16), order=17)),
                 ("coef-nan", dict(coefs=adr(knan))), ("coef-inf", dict(coefs=adr(kinf), order=2)),
                 # the state rules
                 ("no-state-behind-0", dict(sin=None)), ("no-state-at-1", dict(sin=None, first=1)), ("no-state-at-a-segment", dict(sin=None, first=128)),
                 ("no-state-empty-window", dict(sin=None, frames=0)), ("no-state-segment0", dict(sin=None, segment=0)),
                 ("state-equal", dict(sout=p)), ("state-overlap-above", dict(sout=p + STATE - 8)), ("state-overlap-below", dict(sin=p + 8, sout=p)),
                 ("state-equal-at-0", dict(first=0, sout=p))]:
    print("inv", name, call(**kw))
for name, kw in [("good", dict()), ("double", dict(sf=1)), ("s24", dict(df=24)), ("s32", dict(df=32)), ("measure", dict(dst=None)),
                 ("measure-s24", dict(dst=None, df=24, clipped=None)), ("whole-row", dict(first=0, frames=4096, stride=4096)),
                 ("last-frame", dict(first=4095, frames=1)), ("win_frames0", dict(frames=0)), ("row_frames0", dict(row_frames=0, first=0, frames=0)),
                 ("no-state-at-0", dict(sin=None, first=0)), ("no-state-at-0-empty", dict(sin=None, first=0, frames=0)),
                 ("no-state-out", dict(sout=None)), ("no-states-at-0", dict(sin=None, sout=None, first=0)),
                 ("states-adjacent-below", dict(sin=p + STATE, sout=p)), ("order16", dict(coefs=adr(k16), order=16)), ("order1", dict(order=1)),
                 ("segment0", dict(segment=0)), ("segment1", dict(segment=1)), ("segment-huge", dict(segment=2**64 - 1))]:
    print("ok", name, call(**kw))                         # nothing to refuse: answered RR_EXTUNINIT before init_ratelib
"""


def test_the_device_call_refuses_from_its_arguments_alone():
    """RR_INVPARAM comes before RR_EXTUNINIT: in a process that never called init_ratelib (and sees no device) every refusal is
    answered from the arguments, and a call with nothing to refuse -- an empty window among them, which is RR_OK on an initialised
    library -- gets as far as RR_EXTUNINIT and no further."""
    out = subprocess.run([sys.executable, "-c", CHILD % ROOT], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))
    assert out.returncode == 0, out.stderr
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.split() and ln.split()[0] in ("inv", "ok")]
    inv = [ln for ln in lines if ln[0] == "inv"]
    assert len(inv) == 42 and all(int(ln[2]) == RR_INVPARAM for ln in inv), inv
    ok = [ln for ln in lines if ln[0] == "ok"]
    assert len(ok) == 20 and all(int(ln[2]) == RR_EXTUNINIT for ln in ok), ok


def test_python_refusals_need_no_device():
    class Fake:                                              # enough of a tensor to reach the checks that come first
        def __init__(self, dtype, shape, cuda=True):
            self.dtype, self.shape, self.is_cuda = dtype, shape, cuda

        def dim(self):
            return len(self.shape)

        def is_contiguous(self):
            return True

    S16 = F.RRX_FMT_S16
    win = Fake("torch.float32", (2, 10, 2))
    with pytest.raises(TypeError):
        F.tracks_finish_shaped_window_device(Fake("torch.float32", (2, 10, 2), cuda=False), None, 100, 0, 10, S16, 10, "wannamaker9")
    with pytest.raises(TypeError):
        F.tracks_finish_shaped_window_device(Fake("torch.int16", (2, 10, 2)), None, 100, 0, 10, S16, 10, "wannamaker9")
    for args, kw in (((100, 0, 10, None, 10, "wannamaker9"), {}), ((100, 0, 10, 8, 10, "wannamaker9"), {}), ((100, 0, 10, S16, 10, "nobody"), {}),
                     ((100, 0, 10, S16, 10, [0.5] * 17), {}), ((100, 0, 10, S16, 10, "lipshitz5", -1), {}), ((100, 95, 10, S16, 10, "lipshitz5"), {}),
                     ((100, 0, 11, S16, 10, "lipshitz5"), {}),
                     ((100, 5, 10, S16, 10, "lipshitz5"), {}), ((100, 64, 10, S16, 10, "lipshitz5", 64), {})):   # no state behind frame 0
        with pytest.raises(ValueError):
            F.tracks_finish_shaped_window_device(win, None, *args, **kw)
