"""Ragged track batches by windows, host side (RRX_tracks_stage_window_device / RRX_tracks_finish_window_device; DESIGN.md 11,
"Windows"): the symbols, every refusal that needs no device, and the interval arithmetic of the window kernels -- the functions
they call, reached through RRX_debug_tracks_window_cut -- against a restatement in plain Python integers, which cannot wrap,
written from the clamp rules of the whole-row kernels.  CPU only."""
import ctypes as C
import os
import random
import subprocess
import sys

import pytest

import foo_dsp_resampler_amd as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RR_OK, RR_INVPARAM, RR_EXTUNINIT = 0, 6, 5
NEW = ("RRX_tracks_stage_window_device", "RRX_tracks_finish_window_device", "RRX_debug_tracks_window_cut")
LENGTHS = [0, 40, 64, 65, 100, 1500, 2206, 5000]
RATES = [(44100, 48000), (96000, 44100)]
U64 = 2 ** 64
# the entries no plan makes of tests/test_gpu_tracks.py::test_a_wrong_table_stays_inside_the_buffers, stage side and finish side
WRONG_STAGE = [(2 ** 40, 200, 2205, 0, 0, 0), (300, 2 ** 40, 2205, 0, 0, 0), (300, 200, 2 ** 62, 0, 0, 0),
               (2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1, 0, 0, 0), (850, 200, 0, 0, 0, 0), (300, 20, 2205, 0, 0, 0)]
R_OUT, D_OUT, LAST_DST = 1100, 842, 712                      # that test's output pitch, destination frames and last track's dst_first
WRONG_FINISH = [(0, 0, 0, 5, 2 ** 40, LAST_DST), (0, 0, 0, 5, 130, 2 ** 50), (0, 0, 0, 2 ** 63, 130, LAST_DST),
                (0, 0, 0, 2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1)]


def test_symbols_are_exported_and_listed():
    header = open(os.path.join(ROOT, "include", "ratelib_amd.h")).read()
    for name in NEW:
        assert name in F.EXPECTED_SYMBOLS and name in F.available_symbols()
        assert name in header
    for name in ("tracks_stage_window_device", "tracks_finish_window_device"):
        assert callable(getattr(F, name)) and name in F.__all__
    assert callable(F.Resampler.convert_tracks_to_pcm_streamed)


# ------------------------------------------------------------------------------------------------------------- the restatement

def stage_model(e, R, S, wf, wn):
    """stage[10] of the hook: tracks_copy_kernel's and tracks_lpc_kernel's clamps (Entry), then every region cut to the window"""
    src_first, frames, lead = e[0], e[1], e[2]
    lead = min(lead, R)
    frames = min(frames, R - lead)
    fwd = min(lead, R - lead - frames)
    first = min(src_first, S)
    have = min(frames, S - first)
    ext = lead + frames + fwd
    out = []
    for a, b in ((0, lead), (lead, lead + frames), (lead + frames, ext), (ext, R)):
        out += [min(max(a, wf), wf + wn) - wf, min(max(b, wf), wf + wn) - wf]
    cp0, cp1 = out[2], out[3]
    off = wf + cp0 - lead if cp1 > cp0 else 0                # the first copied frame, counted in the track
    return out + [first + off, max(0, min(have - off, cp1 - cp0))]


def finish_model(e, R, D, write, wf, wn):
    """finish[4] of the hook: the prologue of tracks_finish_kernel, then the slice cut to the window"""
    of = min(e[3], R)
    df = min(e[5], D) if write else 0
    frames = min(e[4], R - of)
    if write:
        frames = min(frames, D - df)
    lo, hi = max(of, wf), min(of + frames, wf + wn)
    return [lo - wf, hi - wf, lo - of, df + lo - of] if hi > lo else [0, 0, 0, 0]


def hook(e, R, S, D, write, wf, wn):
    entry = F.RRXTrack(*[int(v) for v in e])
    st, fi = (C.c_ulonglong * 10)(*[0xdead] * 10), (C.c_ulonglong * 4)(*[0xdead] * 4)
    assert F.lib().RRX_debug_tracks_window_cut(C.byref(entry), R, S, D, int(write), wf, wn, st, fi) == RR_OK
    return list(st), list(fi)


def check(e, R, S, D, wf, wn):
    """one entry, one window, both passes (the finish pass written and measure-only)"""
    st, fi = hook(e, R, S, D, True, wf, wn)
    want = stage_model(e, R, S, wf, wn)
    assert all(0 <= v < U64 for v in want)
    assert st == want, (e, R, S, wf, wn, st, want)
    # adjacent, in order, and covering the window exactly: every frame of the window belongs to one region
    assert st[0] == 0 and st[1] == st[2] and st[3] == st[4] and st[5] == st[6] and st[7] == wn and st[2] <= st[3] and st[4] <= st[5], st
    assert st[9] <= st[3] - st[2] and (not st[9] or st[8] + st[9] <= S), st   # what is read lies inside the source
    assert fi == finish_model(e, R, D, True, wf, wn), (e, R, D, wf, wn, fi)
    assert fi[1] <= wn and fi[3] + (fi[1] - fi[0]) <= D, fi   # inside the window and inside the destination
    _, fm = hook(e, R, S, D, False, wf, wn)
    assert fm == finish_model(e, R, D, False, wf, wn), (e, R, wf, wn, fm)


def boundaries(e, R, S, D):
    """every region boundary of the entry's row (input side and output side), and one frame on either side, inside [0, R]"""
    lead = min(e[2], R)
    frames = min(e[1], R - lead)
    ext = lead + frames + min(lead, R - lead - frames)
    of = min(e[3], R)
    end = of + min(e[4], R - of, D - min(e[5], D))
    pts = set()
    for b in (0, lead, lead + frames, ext, of, end, R):
        pts |= {b - 1, b, b + 1}
    return sorted(p for p in pts if 0 <= p <= R)


def cases():
    """(entry, row_frames, src_total, dst_total): every entry of the plans -- the stage side at the input pitch, the finish side at
    the output pitch -- and every wrong entry"""
    out = []
    for fs, fo in RATES:
        plan = F.tracks_plan(fs, fo, LENGTHS)
        for e in plan.array():
            out.append((tuple(int(v) for v in e), plan.row_frames, plan.src_total, plan.dst_total))
            out.append((tuple(int(v) for v in e), plan.out_row_cap, plan.src_total, plan.dst_total))
    plan = F.tracks_plan(44100, 48000, [300, 200, 400])
    out += [(e, plan.row_frames, plan.src_total, plan.dst_total) for e in WRONG_STAGE]
    out += [(e, R_OUT, 900, D_OUT) for e in WRONG_FINISH + WRONG_STAGE]
    return out


def test_plans_have_the_regions_the_windows_cut():
    plan = F.tracks_plan(44100, 48000, LENGTHS)
    assert plan.row_frames == 5000 + 2 * 2205 and [int(e.lead) for e in plan.table] == [0, 0, 0, 2205, 2205, 2205, 2205, 2205]


def test_window_cut_equals_the_restatement_at_every_boundary():
    n = 0
    for e, R, S, D in cases():
        pts = boundaries(e, R, S, D)
        for i, a in enumerate(pts):
            for b in pts[i:]:                                # every window that begins and ends at a boundary or next to one (empty ones too)
                check(e, R, S, D, a, b - a)
                n += 1
            if a < R:
                check(e, R, S, D, a, 1)                      # single-frame windows
                n += 1
    assert n > 3000, n


def test_window_cut_equals_the_restatement_on_random_windows():
    rng = random.Random(20)
    all_cases = cases()
    for _ in range(4000):
        e, R, S, D = rng.choice(all_cases)
        a = rng.randrange(R + 1)
        check(e, R, S, D, a, rng.randrange(R - a + 1))
    # entries and sizes of any magnitude: nothing wraps
    for _ in range(2000):
        e = tuple(rng.choice([0, 1, 7, rng.randrange(2 ** 12), rng.randrange(2 ** 40), 2 ** 63, U64 - 1 - rng.randrange(3)]) for _ in range(6))
        R, S, D = (rng.choice([1, 2, rng.randrange(1, 2 ** 13), 2 ** 58 - 1 - rng.randrange(2)]) for _ in range(3))
        a = rng.choice([0, rng.randrange(R + 1), R])
        check(e, R, S, D, a, rng.choice([0, min(1, R - a), rng.randrange(R - a + 1), R - a]))


def test_disjoint_windows_process_every_frame_of_a_slice_once():
    for e, R, S, D in cases():
        for step in (1, 7, 333, R):
            if R // step > 3000:
                continue
            stage_seen, slice_seen, nxt = [0] * 4, 0, None
            for wf in range(0, R, step):
                st, fi = hook(e, R, S, D, True, wf, min(step, R - wf))
                for k in range(4):
                    stage_seen[k] += st[2 * k + 1] - st[2 * k]
                if fi[1] > fi[0]:
                    assert nxt is None or (fi[2], fi[3]) == nxt, (e, wf, fi, nxt)   # index and destination run on from the window before
                    nxt = (fi[2] + fi[1] - fi[0], fi[3] + fi[1] - fi[0])
                    slice_seen += fi[1] - fi[0]
            whole_st, whole_fi = hook(e, R, S, D, True, 0, R)
            assert stage_seen == [whole_st[2 * k + 1] - whole_st[2 * k] for k in range(4)] and sum(stage_seen) == R
            assert slice_seen == whole_fi[1] - whole_fi[0], (e, step)


def test_hook_refusals_and_inert_without_test_hooks():
    fn = F.lib().RRX_debug_tracks_window_cut
    e = F.RRXTrack(0, 10, 0, 0, 10, 0)
    st, fi = (C.c_ulonglong * 10)(), (C.c_ulonglong * 4)()
    assert fn(C.byref(e), 100, 10, 10, 1, 0, 100, st, fi) == RR_OK
    assert fn(None, 100, 10, 10, 1, 0, 100, st, fi) == RR_INVPARAM
    assert fn(C.byref(e), 100, 10, 10, 1, 0, 100, None, fi) == RR_INVPARAM
    assert fn(C.byref(e), 100, 10, 10, 1, 0, 100, st, None) == RR_INVPARAM
    assert fn(C.byref(e), 100, 10, 10, 1, 1, 100, st, fi) == RR_INVPARAM
    assert fn(C.byref(e), 100, 10, 10, 1, 2, U64 - 1, st, fi) == RR_INVPARAM
    code = ("import sys; sys.path.insert(0, %r)\nimport foo_dsp_resampler_amd as F\n"
            "print(F.lib().RRX_debug_tracks_window_cut(None, 0, 0, 0, 0, 0, 0, None, None))\n" % ROOT)
    env = {k: v for k, v in os.environ.items() if k != "RSMP_TEST_HOOKS"}
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-1] == "-1"


# ------------------------------------------------------------------------------------------------------------------ refusals

CHILD = r"""
import sys, ctypes as C
sys.path.insert(0, %r)
import foo_dsp_resampler_amd as F
L = F.lib()
p = 0x10000  # never dereferenced: every call below is answered from its arguments, or from the library's state, alone
stage = dict(device=-1, stream=None, fs=44100, fo=48000, table=p, ntracks=3, nch=2, fmt=16, packed=p, src_total=1000, row_frames=4096,
             first=100, frames=500, win=p, stride=512)
def call_stage(**kw):
    a = dict(stage, **kw)
    return L.RRX_tracks_stage_window_device(a["device"], a["stream"], a["fs"], a["fo"], a["table"], a["ntracks"], a["nch"], a["fmt"], a["packed"],
                                            a["src_total"], a["row_frames"], a["first"], a["frames"], a["win"], a["stride"])
fin = dict(device=-1, stream=None, table=p, ntracks=3, nch=2, sf=0, win=p, stride=512, row_frames=4096, first=100, frames=500, df=16, dst=p,
           dst_total=9000, gain=None, dither=1, seed=7, peak=p, clipped=p)
def call_fin(**kw):
    a = dict(fin, **kw)
    return L.RRX_tracks_finish_window_device(a["device"], a["stream"], a["table"], a["ntracks"], a["nch"], a["sf"], a["win"], a["stride"],
                                             a["row_frames"], a["first"], a["frames"], a["df"], a["dst"], a["dst_total"], a["gain"], a["dither"],
                                             a["seed"], a["peak"], a["clipped"])
window = [("past-the-row", dict(first=3597)), ("first-past-the-row", dict(first=4097, frames=0)), ("sum-wraps", dict(first=2**64 - 1, frames=2)),
          ("sum-wraps-to-0", dict(first=2**64 - 500)), ("frames-wrap", dict(first=1, frames=2**64 - 1, stride=2**64 - 1)),
          ("stride", dict(stride=499)), ("stride0", dict(stride=0)), ("window2^60", dict(stride=2**58)),
          ("window2^60-1track", dict(ntracks=1, nch=1, stride=2**60, row_frames=2**59, src_total=10)),
          ("empty-past-the-row", dict(first=5000, frames=0)), ("empty-stride-wide", dict(frames=0, stride=2**58))]
for name, kw in [("fmt8", dict(fmt=8)), ("double", dict(fmt=1)), ("table", dict(table=None)), ("packed", dict(packed=None)), ("win", dict(win=None)),
                 ("ntracks0", dict(ntracks=0)), ("ntracks-1", dict(ntracks=-1)), ("nch0", dict(nch=0)), ("fs0", dict(fs=0)), ("fo0", dict(fo=0)),
                 ("row_frames0", dict(row_frames=0, first=0, frames=0)), ("device-2", dict(device=-2)), ("channels2^30", dict(ntracks=2**29, nch=2)),
                 ("src2^60", dict(src_total=2**59)), ("rows2^60", dict(row_frames=2**58))] + window:
    print("inv stage", name, call_stage(**kw))
for name, kw in [("table", dict(table=None)), ("win", dict(win=None)), ("ntracks0", dict(ntracks=0)), ("ntracks-1", dict(ntracks=-1)),
                 ("nch0", dict(nch=0)), ("sf16", dict(sf=16)), ("sf7", dict(sf=7)), ("df0", dict(df=0)), ("df1", dict(df=1)), ("df8", dict(df=8)),
                 ("nothing-to-do", dict(dst=None, peak=None, clipped=None)), ("device-2", dict(device=-2)), ("rows2^60", dict(row_frames=2**58)),
                 ("dst2^60", dict(dst_total=2**59))] + window:
    print("inv finish", name, call_fin(**kw))
for name, kw in [("good", dict()), ("float", dict(fmt=0)), ("s24", dict(fmt=24)), ("s32", dict(fmt=32)), ("whole-row", dict(first=0, frames=4096, stride=4096)),
                 ("last-frame", dict(first=4095, frames=1)), ("win_frames0", dict(frames=0)), ("win_frames0-at-the-end", dict(first=4096, frames=0)),
                 ("below-2^60", dict(ntracks=1, nch=1, stride=2**60 - 1, row_frames=2**60 - 1, first=0, frames=2**60 - 1, src_total=10))]:
    print("ok stage", name, call_stage(**kw))              # nothing to refuse: answered RR_EXTUNINIT before init_ratelib
for name, kw in [("good", dict()), ("double", dict(sf=1)), ("measure", dict(dst=None)), ("whole-row", dict(first=0, frames=4096, stride=4096)),
                 ("last-frame", dict(first=4095, frames=1)), ("win_frames0", dict(frames=0)), ("row_frames0", dict(row_frames=0, first=0, frames=0))]:
    print("ok finish", name, call_fin(**kw))
"""


def test_window_calls_refuse_from_their_arguments_alone():
    """RR_INVPARAM comes before RR_EXTUNINIT: in a process that never called init_ratelib (and sees no device) every refusal is
    answered from the arguments, and a call with nothing to refuse -- an empty window among them, which is RR_OK on an initialised
    library (tests/test_gpu_tracks_window.py) -- gets as far as RR_EXTUNINIT and no further."""
    out = subprocess.run([sys.executable, "-c", CHILD % ROOT], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))
    assert out.returncode == 0, out.stderr
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.split() and ln.split()[0] in ("inv", "ok")]
    for what, n_inv, n_ok in (("stage", 26, 9), ("finish", 25, 7)):
        inv = [ln for ln in lines if ln[:2] == ["inv", what]]
        assert len(inv) == n_inv and all(int(ln[3]) == RR_INVPARAM for ln in inv), inv
        ok = [ln for ln in lines if ln[:2] == ["ok", what]]
        assert len(ok) == n_ok and all(int(ln[3]) == RR_EXTUNINIT for ln in ok), ok


def test_python_refusals_need_no_device():
    class Fake:                                              # enough of a tensor to reach the checks that come first
        def __init__(self, dtype, shape):
            self.dtype, self.shape, self.is_cuda = dtype, shape, False

        def dim(self):
            return len(self.shape)

        def is_contiguous(self):
            return True

    with pytest.raises(TypeError):
        F.tracks_stage_window_device(Fake("torch.float32", (10, 2)), None, 44100, 48000, 100, 0, 10)
    with pytest.raises(TypeError):
        F.tracks_finish_window_device(Fake("torch.float32", (1, 10, 2)), None, 100, 0, 10, F.RRX_FMT_S16, 10)
    with pytest.raises(TypeError):
        F.tracks_finish_window_device(Fake("torch.int16", (1, 10, 2)), None, 100, 0, 10, F.RRX_FMT_S16, 10)
