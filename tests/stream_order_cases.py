"""The table of the stream-order tests: one row per entry point of include/ratelib_amd.h that takes `hip_stream`, and the handle
calls with their stream (tests/test_gpu_stream_order.py runs the rows on the device, tests/test_stream_order_table.py holds the
table to the header on the host).

A row is a function row(run, seam): it builds its buffers, and hands every call it makes to
    run(enqueue, inputs, outputs, entry, scratch=())
where enqueue(stream) queues the call through the C ABI on a torch stream, `inputs` are the device tensors the call only reads,
`outputs` those it writes or accumulates into -- holding what they start from: guards around what the call owns, and non-trivial
values in accumulating statistics -- and `scratch` the work buffers, whose content the header leaves unspecified.  run is the
gated driver of tests/stream_gate.py; what the gates are for is written there.

`seam` False: the smallest shape at which every launch of the call happens, the shapes the other GPU tests derive from the tile
constants.  `seam` True: 32768 + 3 streams or tracks of a few frames (65537 for the mix), so that the launches of the second slice
of 32768 are ordered too; rows whose launcher has no such loop have no seam case (SEAMLESS).  The rows whose arguments
tests/seam_cases.py already builds go through its caller and keep every assertion it makes about guards and inputs."""
import re

import numpy as np

import foo_dsp_resampler_amd as F

FS, FO = 44100, 48000             # an extension of 2205 frames at either end of a track above 64 frames
N_SEAM = 32768 + 3
GUARD = 777.25
CEILING = 0.3
TRACK_LENGTHS = (40, 65, 2300)    # no extension, the shortest extended track, and one above prime_len (2205)
WINDOW = (2180, 63)               # across the end of the backward extension (frame 2205)

_keep = []                        # host arrays whose pointers calls hold


def host(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    _keep.append(a)
    return a.ctypes.data


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def L():
    F.ratelib._ensure_init()
    return F.lib()


def rng(*key):
    return np.random.default_rng([20250101] + [int(k) for k in key])


def ok(rc, entry):
    assert rc == 0, (entry, rc)


class Guarded:
    """outputs with one guard row of the leading dimension at either end: out() gives the view a call takes, `bigs` the whole
    buffers (what the driver stages and compares), check() that the guard rows still hold the guard"""

    def __init__(self):
        self.bigs, self.fills, self.starts = [], [], []

    def out(self, shape, dtype, fill=GUARD, start=None):
        import torch
        big = torch.full((shape[0] + 2,) + tuple(shape[1:]), fill, dtype=dtype, device="cuda")
        if start is not None:
            big[1:-1] = start
        self.bigs.append(big)
        self.fills.append(fill)
        self.starts.append(start)
        return big[1:-1]

    def reset(self):
        """every buffer as it was made: a second call on them must do the work again"""
        for big, fill, start in zip(self.bigs, self.fills, self.starts):
            big.fill_(fill)
            if start is not None:
                big[1:-1] = start

    def check(self, entry):
        for big, fill in zip(self.bigs, self.fills):
            assert bool((big[0] == fill).all()) and bool((big[-1] == fill).all()), (entry, "entries around an output were written")


def slices_table(n, row):
    """n tracks as slices of rows of `row` frames: out_first cycles through 0..3, out_frames through row - 5 .. row - 3"""
    t = np.arange(n)
    tab = np.zeros((n, 6), np.uint64)
    tab[:, 3] = t % 4
    tab[:, 4] = row - 5 + t % 3
    return tab


def bs1770():
    import true_peak_model as TM
    return np.ascontiguousarray(TM.BS1770, dtype=np.float64)


# ------------------------------------------------------------------------------------------------- rows through tests/seam_cases.py

def through_seam_cases(thunk):
    def row(run, seam):
        import seam_cases as K
        with K.gated_by(lambda enqueue, ins, outs, entry: run(enqueue, ins, outs, entry)):
            thunk(K)
    return row


def _groups(percentiles):
    def thunk(K):
        import loudness_stats_model as S
        if percentiles is None:
            zs, group, ng = K.gate_groups_case(300)
            rows, nb = K.rows_of(zs)
            K.groups_call(rows, nb, group, ng, *S.gate_thresholds())
        else:
            zs, group, ng = K.range_case(700)
            rows, nb = K.rows_of(zs)
            K.groups_call(rows, nb, group, ng, *K.RANGE_GATE, percentiles=percentiles)
    return thunk


# -------------------------------------------------------------------------------------------------------------------- LPC, stage, mix

def lpc_extrapolate(run, seam):
    import torch
    n, nch, order, bk, fw, ns = 1024, 2, 32, 40, 50, 2
    stride = bk + n + fw
    g = Guarded()
    x = g.out((ns, stride, nch), torch.float32, start=dev((rng(1).standard_normal((ns, stride, nch)) * 0.3).astype(np.float32)))
    lib = L()
    run(lambda s: ok(lib.RRX_lpc_extrapolate_device(-1, s.cuda_stream, x.data_ptr() + bk * nch * 4, stride, ns, n, nch, order, bk, fw), "lpc"),
        [], g.bigs, "RRX_lpc_extrapolate_device")
    g.check("lpc")
    g.reset()                                        # the Python wrapper forwards its stream
    run(lambda s: F.lpc_extrapolate_device(x, bk, n, bk, fw, order=order, stream=s), [], g.bigs, "RRX_lpc_extrapolate_device")


def _stage_case(seam, nch_src, dtype=np.float32):
    """(fs, fo, plan, packed source, device table): TRACK_LENGTHS at 44.1k -> 48k, or 32771 tracks of 0..70 frames at 1000 -> 2000
    Hz as tests/test_gpu_stream_seams.py has them"""
    if seam:
        fs, fo = 1000, 2000
        lengths = np.array([0, 70, 65, 69, 40, 66, 64])[np.arange(N_SEAM) % 7].tolist()
    else:
        fs, fo, lengths = FS, FO, list(TRACK_LENGTHS)
    plan = F.tracks_plan(fs, fo, lengths)
    total = int(sum(lengths))
    r = rng(2, nch_src, seam)
    if dtype == np.float32:
        x = (r.standard_normal((total, nch_src)) * 0.3).astype(np.float32)
    else:
        x = r.integers(-20000, 20000, (total, nch_src)).astype(np.int16)
    return fs, fo, plan, dev(x), plan.to_device("cuda")


def _window(plan, seam):
    return (45, 10) if seam else WINDOW  # seam: an extension is 50 frames


def tracks_stage(run, seam, samples=False, window=False, mix=None):
    import torch
    nch_src = 2 if mix is None else mix.shape[1]
    nch = 2 if mix is None else mix.shape[0]
    fs, fo, plan, packed, table = _stage_case(seam, nch_src, np.int16 if samples else np.float32)
    n, R, total = len(plan), plan.row_frames, plan.src_total
    fmt = F.RRX_FMT_S16 if samples else F.RRX_FMT_FLOAT
    g = Guarded()
    lib = L()
    m = None if mix is None else host(mix)
    if window:
        wf, wn = _window(plan, seam)
        win = g.out((n, wn + 2, nch), torch.float32)
        if mix is None:
            entry = "RRX_tracks_stage_window_device"
            enqueue = lambda s: ok(lib.RRX_tracks_stage_window_device(-1, s.cuda_stream, fs, fo, table.data_ptr(), n, nch, fmt, packed.data_ptr(), total,
                                                                       R, wf, wn, win.data_ptr(), wn + 2), entry)
        else:
            entry = "RRX_tracks_stage_mix_window_device"
            enqueue = lambda s: ok(lib.RRX_tracks_stage_mix_window_device(-1, s.cuda_stream, fs, fo, table.data_ptr(), n, fmt, nch_src, packed.data_ptr(),
                                                                           total, nch, m, R, wf, wn, win.data_ptr(), wn + 2), entry)
    else:
        rows = g.out((n, R, nch), torch.float32)
        if mix is not None:
            entry = "RRX_tracks_stage_mix_device"
            enqueue = lambda s: ok(lib.RRX_tracks_stage_mix_device(-1, s.cuda_stream, fs, fo, table.data_ptr(), n, fmt, nch_src, packed.data_ptr(), total,
                                                                    nch, m, rows.data_ptr(), R), entry)
        elif samples:
            entry = "RRX_tracks_stage_device_samples"
            enqueue = lambda s: ok(lib.RRX_tracks_stage_device_samples(-1, s.cuda_stream, fs, fo, table.data_ptr(), n, nch, fmt, packed.data_ptr(), total,
                                                                        rows.data_ptr(), R), entry)
        else:
            entry = "RRX_tracks_stage_device"
            enqueue = lambda s: ok(lib.RRX_tracks_stage_device(-1, s.cuda_stream, fs, fo, table.data_ptr(), n, nch, packed.data_ptr(), total,
                                                                rows.data_ptr(), R), entry)
    run(enqueue, [packed, table], g.bigs, entry)
    g.check(entry)
    if not seam and not window:
        # every frame of every row was written, and both launches had work: a copied track and an LPC extension that is not silence
        assert not bool((rows == GUARD).any()) and float(rows[2, :2205].abs().max()) > 0 and float(rows[0, :40].abs().max()) > 0
        g.reset()
        if mix is None:                              # the Python wrapper forwards its stream
            run(lambda s: F.tracks_stage_device(packed, table, fs, fo, R, out=rows, stream=s), [packed, table], g.bigs, entry)
        else:
            run(lambda s: F.tracks_stage_mix_device(packed, table, mix, fs, fo, R, out=rows, stream=s), [packed, table], g.bigs, entry)
    if not seam and window:
        g.reset()
        if mix is None:
            run(lambda s: F.tracks_stage_window_device(packed, table, fs, fo, R, wf, wn, out=win, stream=s), [packed, table], g.bigs, entry)
        else:
            run(lambda s: F.tracks_stage_mix_window_device(packed, table, mix, fs, fo, R, wf, wn, out=win, stream=s), [packed, table], g.bigs, entry)


def mix_rows(run, seam):
    import torch
    import mix_cases as MC
    if seam:
        M, ns, frames, dtype = MC.MATRICES["2to1"], 65537, 2, np.float32
    else:
        M, ns, frames, dtype = MC.MATRICES["6to2"], 3, 1025, np.float64
    stride, dstride = frames + 5, frames + 3
    x = dev(rng(3, seam).standard_normal((ns, stride, M.shape[1])).astype(dtype))
    g = Guarded()
    out = g.out((ns, dstride, M.shape[0]), x.dtype)
    m, lib = host(M), L()
    fmt = F.RRX_FMT_DOUBLE if dtype == np.float64 else F.RRX_FMT_FLOAT
    run(lambda s: ok(lib.RRX_mix_device(-1, s.cuda_stream, fmt, x.data_ptr(), stride, ns, frames, M.shape[1], out.data_ptr(), dstride, M.shape[0], m), "mix"),
        [x], g.bigs, "RRX_mix_device")
    g.check("mix")
    assert bool((out[:, frames:] == GUARD).all()), "frames outside [0, frames) were written"
    if not seam:
        g.reset()
        run(lambda s: F.mix_device(x, M, out=out, frames=frames, stream=s), [x], g.bigs, "RRX_mix_device")


# -------------------------------------------------------------------------------------------------------------------------- packed

def _packed_case():
    lengths = [40, 65, 2300, 1]
    total = sum(lengths)
    x = dev(rng(4).integers(-20000, 20000, (total, 2)).astype(np.int16))
    tab = F.packed_plan(lengths).array()
    return lengths, total, x, dev(tab), dev(0.5 + 0.25 * np.arange(len(lengths)))


def tracks_true_peak_packed(run, seam):
    import torch
    lengths, total, x, table, gain = _packed_case()
    n, nch = len(lengths), 2
    g = Guarded()
    tp = g.out((n, nch), torch.float64, start=1e-3)
    pk = g.out((n, nch), torch.float64, start=2e-3)
    k, lib = host(bs1770()), L()
    run(lambda s: ok(lib.RRX_tracks_true_peak_packed_device(-1, s.cuda_stream, table.data_ptr(), n, nch, F.RRX_FMT_S16, x.data_ptr(), total, max(lengths),
                                                            gain.data_ptr(), k, 4, 12, tp.data_ptr(), pk.data_ptr()), "tp packed"),
        [x, table, gain], g.bigs, "RRX_tracks_true_peak_packed_device")
    g.check("tp packed")
    assert float(tp.max()) > 2e-3 and float(tp.min()) >= 1e-3, "the staged statistics were not accumulated into"


def tracks_loudness_packed(run, seam):
    import torch
    import loudness_model as LM
    lengths, total, x, table, gain = _packed_case()
    n, nch, hop = len(lengths), 2, 16
    stride = max(lengths) // hop + 1
    lib = L()
    need = lib.RRX_loudness_work_doubles(n, nch, max(lengths), hop)
    g = Guarded()
    e = g.out((n, nch, stride), torch.float64)
    hops = g.out((n,), torch.int64, fill=12345)
    work = torch.zeros((max(need, 1),), dtype=torch.float64, device="cuda")
    k = host(LM.K48)
    run(lambda s: ok(lib.RRX_tracks_loudness_packed_device(-1, s.cuda_stream, table.data_ptr(), n, nch, F.RRX_FMT_S16, x.data_ptr(), total, max(lengths),
                                                           gain.data_ptr(), k, hop, e.data_ptr(), stride, hops.data_ptr(), work.data_ptr(), need),
                     "loudness packed"),
        [x, table, gain], g.bigs, "RRX_tracks_loudness_packed_device", scratch=[work])
    g.check("loudness packed")
    assert hops.tolist() == [v // hop for v in lengths]


# ------------------------------------------------------------------------------------------------------------------------ limiter

def _limit_rows(seam, shape):
    """(x [ns, frames, nch] float32 with peaks above the ceiling, gain [ns])"""
    ns, nch, frames = shape
    x = (rng(5, ns, nch, frames).standard_normal((ns, frames, nch)) * 0.25).astype(np.float32)
    return dev(x), dev(0.75 + 0.5 * (np.arange(ns) % 7) / 7.0)


def limit(run, seam, release=None, tracks=False):
    """RRX_limit_device and its three siblings: (2 streams, 2 channels, 1025 frames, L 64, H 0) is one frame past the smoothing
    launch's 1024 frames a workgroup, (1, 2, 2036, 1024, 4096) one value past a tile of the window minimum; with a release the
    block of 64 entries gives the scan several blocks a row"""
    import torch
    lib = L()
    entry = "RRX_%slimit%s_device" % ("tracks_" if tracks else "", "" if release is None else "_release")
    shapes = [(N_SEAM, 1, 6, 2, 1)] if seam else [(2, 2, 1025, 64, 0), (1, 2, 2036, 1024, 4096)]
    k = host(bs1770())
    for ns, nch, frames, look, hold in shapes:
        x, gain = _limit_rows(seam, (ns, nch, frames))
        g = Guarded()
        y = g.out((ns, frames, nch), torch.float64)
        red = g.out((ns,), torch.float64, start=0.97)
        lim = g.out((ns,), torch.int64, fill=12345, start=7)
        if release is None:
            need, rel = lib.RRX_limit_work_doubles(ns, frames, 12, look), ()
        else:
            need, rel = lib.RRX_limit_release_work_doubles(ns, frames, 12, look, 64), (float(release), 64)
        assert need
        work = torch.zeros((need,), dtype=torch.float64, device="cuda")
        tail = (red.data_ptr(), lim.data_ptr(), work.data_ptr(), need)
        ins = [x, gain]
        if tracks:
            table = dev(slices_table(ns, frames))
            ins.append(table)
            head = (table.data_ptr(), ns, nch, F.RRX_FMT_FLOAT, x.data_ptr(), F.RRX_FMT_DOUBLE, y.data_ptr(), frames, gain.data_ptr(), CEILING, k, 4, 12,
                    look, hold)
        else:
            head = (F.RRX_FMT_FLOAT, x.data_ptr(), frames, F.RRX_FMT_DOUBLE, y.data_ptr(), frames, ns, frames, nch, gain.data_ptr(), CEILING, k, 4, 12,
                    look, hold)
        fn = getattr(lib, entry)
        run(lambda s: ok(fn(-1, s.cuda_stream, *(head + rel + tail)), entry), ins, g.bigs, entry, scratch=[work])
        g.check(entry)
        assert float(red.min()) < 0.97 and int(lim.max()) > 7, (entry, "nothing was limited: the case is trivial")


def limit_window(run, seam, release=None):
    """the window forms on whole rows as the halo buffer: a window in the middle of the rows; with a release, the state of the
    window in front of it (made by a synchronised call) is an input"""
    import torch
    lib = L()
    entry = "RRX_tracks_limit%s_window_device" % ("" if release is None else "_release")
    ns, nch, R, look, hold = (N_SEAM, 1, 12, 2, 1) if seam else (3, 2, 1500, 64, 0)
    wf, wn = (4, 6) if seam else (300, 1025)
    x, gain = _limit_rows(seam, (ns, nch, R))
    table = dev(slices_table(ns, R))
    k = host(bs1770())
    g = Guarded()
    y = g.out((ns, wn + 2, nch), torch.float64)
    red = g.out((ns,), torch.float64, start=0.97)
    lim = g.out((ns,), torch.int64, fill=12345, start=7)

    def args(first, frames, dst, state):
        head = (table.data_ptr(), ns, nch, F.RRX_FMT_FLOAT, x.data_ptr(), R, 0, R, R, first, frames, F.RRX_FMT_DOUBLE, dst.data_ptr(), dst.shape[1],
                gain.data_ptr(), CEILING, k, 4, 12, look, hold)
        return head + state

    ins = [x, gain, table]
    if release is None:
        need, state = lib.RRX_tracks_limit_window_work_doubles(ns, max(wn, wf), 12, look, hold), ()
    else:
        need = lib.RRX_tracks_limit_release_window_work_doubles(ns, max(wn, wf), 12, look, hold, 64)
        sin = torch.zeros((ns, 8), dtype=torch.float64, device="cuda")
        sout = g.out((ns, 8), torch.float64)
        state = (float(release), 64, sin.data_ptr(), sout.data_ptr())
        ins.append(sin)
    assert need
    work = torch.zeros((need,), dtype=torch.float64, device="cuda")
    tail = (red.data_ptr(), lim.data_ptr(), work.data_ptr(), need)
    fn = getattr(lib, entry)
    if release is not None:                          # the window [0, wf) in front, the old way: its state out is the gated call's state in
        front = torch.zeros((ns, wf, nch), dtype=torch.float64, device="cuda")
        r0, l0 = torch.ones((ns,), dtype=torch.float64, device="cuda"), torch.zeros((ns,), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ok(fn(-1, None, *(args(0, wf, front, (float(release), 64, None, sin.data_ptr())) + (r0.data_ptr(), l0.data_ptr(), work.data_ptr(), need))), entry)
        torch.cuda.synchronize()
        assert bool(sin.abs().sum() > 0)
    run(lambda s: ok(fn(-1, s.cuda_stream, *(args(wf, wn, y, state) + tail)), entry), ins, g.bigs, entry, scratch=[work])
    g.check(entry)
    assert bool((y[:, wn:] == GUARD).all()), "frames behind the window were written"
    assert float(red.min()) < 0.97 and int(lim.max()) > 7, (entry, "nothing was limited: the case is trivial")


# --------------------------------------------------------------------------------------------------- the measuring passes by windows

def measure_window(run, seam, loudness=False):
    """RRX_tracks_true_peak_window_device / RRX_tracks_loudness_window_device on the second of two windows: the state of the first
    (a synchronised call) is an input"""
    import torch
    import loudness_model as LM
    lib = L()
    entry = "RRX_tracks_%s_window_device" % ("loudness" if loudness else "true_peak")
    n, nch, R = (N_SEAM, 2, 12) if seam else (3, 2, 700)
    wf, wn = (5, 6) if seam else (333, 300)
    hop, stride = (2, 8) if seam else (16, 50)
    x = dev((rng(6, seam).standard_normal((n, R, nch)) * 0.3).astype(np.float32))
    table, gain = dev(slices_table(n, R)), dev(0.5 + 0.25 * (np.arange(n) % 5))
    k = host(LM.K48 if loudness else bs1770())
    g = Guarded()
    sin = torch.zeros((n * nch, 16), dtype=torch.float64, device="cuda")
    sout = g.out((n * nch, 16), torch.float64)
    if loudness:
        e = g.out((n, nch, stride), torch.float64)
        hops = g.out((n,), torch.int64, fill=12345)
        need = lib.RRX_tracks_loudness_window_work_doubles(n, nch, max(wf, wn), hop)
        work = torch.zeros((need,), dtype=torch.float64, device="cuda")
        scratch = [work]

        def args(first, frames, win, s_in, s_out):
            return (table.data_ptr(), n, nch, F.RRX_FMT_FLOAT, win.data_ptr(), win.shape[1], R, first, frames, gain.data_ptr(), k, hop, s_in, s_out,
                    e.data_ptr(), stride, hops.data_ptr(), work.data_ptr(), need)
    else:
        tp = g.out((n, nch), torch.float64, start=1e-3)
        pk = g.out((n, nch), torch.float64, start=2e-3)
        scratch = []

        def args(first, frames, win, s_in, s_out):
            return (table.data_ptr(), n, nch, F.RRX_FMT_FLOAT, win.data_ptr(), win.shape[1], R, first, frames, gain.data_ptr(), k, 4, 12, s_in, s_out,
                    tp.data_ptr(), pk.data_ptr())
    fn = getattr(lib, entry)
    w0 = x[:, :wf].contiguous()
    w1 = torch.full((n, wn + 2, nch), 1e30, dtype=torch.float32, device="cuda")
    w1[:, :wn] = x[:, wf:wf + wn]
    torch.cuda.synchronize()
    ok(fn(-1, None, *args(0, wf, w0, None, sin.data_ptr())), entry)       # the first window, the old way; what it left in the
    torch.cuda.synchronize()                                              # statistics is what the gated call starts from
    assert bool(sin.abs().sum() > 0)
    run(lambda s: ok(fn(-1, s.cuda_stream, *args(wf, wn, w1, sin.data_ptr(), sout.data_ptr())), entry), [w1, table, gain, sin], g.bigs, entry,
        scratch=scratch)
    g.check(entry)
    assert bool(sout.abs().sum() > 0)


# --------------------------------------------------------------------------------------------------------------------------- the table

def _rows():
    import mix_cases as MC
    T = through_seam_cases
    six = MC.MATRICES["6to2"]
    return {
        "RRX_lpc_extrapolate_device": lpc_extrapolate,
        "RRX_finish_device": T(lambda K: K.finish_call("f32-s16", True)),
        "RRX_finish_shaped_device": T(lambda K: K.shaped_call("order9", True)),          # nine frames from frame 2: the incoming state is read
        "RRX_true_peak_device": T(lambda K: K.tp_call("bs1770", True)),
        "RRX_tracks_stage_device": tracks_stage,
        "RRX_tracks_stage_device_samples": lambda run, seam: tracks_stage(run, seam, samples=True),
        "RRX_tracks_finish_device": T(lambda K: K.tracks_finish_call(False, F.RRX_FMT_S16, "rows")),
        "RRX_tracks_finish_shaped_device": T(lambda K: K.tracks_finish_call(False, F.RRX_FMT_S16, "shaped", 9)),
        "RRX_tracks_true_peak_device": T(lambda K: K.tracks_true_peak_call(False)),
        "RRX_tracks_true_peak_packed_device": tracks_true_peak_packed,
        "RRX_limit_device": limit,
        "RRX_tracks_limit_device": lambda run, seam: limit(run, seam, tracks=True),
        "RRX_limit_release_device": lambda run, seam: limit(run, seam, release=0.999),
        "RRX_tracks_limit_release_device": lambda run, seam: limit(run, seam, release=0.999, tracks=True),
        "RRX_loudness_device": T(lambda K: K.loudness_call(False, True)),
        "RRX_tracks_loudness_device": T(lambda K: K.tracks_loudness_call(False)),
        "RRX_tracks_loudness_packed_device": tracks_loudness_packed,
        "RRX_loudness_gate_device": T(lambda K: K.gate_call(True)),
        "RRX_loudness_blocks_device": T(lambda K: K.blocks_call(4, 1, True)),               # d_max is given: the memset path
        "RRX_loudness_gate_groups_device": T(_groups(None)),
        "RRX_loudness_range_groups_device": T(_groups((10, 95))),
        "RRX_tracks_stage_window_device": lambda run, seam: tracks_stage(run, seam, samples=True, window=True),
        "RRX_tracks_finish_window_device": T(lambda K: K.tracks_finish_call(True, F.RRX_FMT_S24_3, "windows")),
        "RRX_tracks_finish_shaped_window_device": T(lambda K: K.tracks_finish_call(True, F.RRX_FMT_S24_3, "shaped-windows", 4)),
        "RRX_tracks_true_peak_window_device": measure_window,
        "RRX_tracks_loudness_window_device": lambda run, seam: measure_window(run, seam, loudness=True),
        "RRX_tracks_limit_window_device": limit_window,
        "RRX_tracks_limit_release_window_device": lambda run, seam: limit_window(run, seam, release=0.999),
        "RRX_mix_device": mix_rows,
        "RRX_tracks_stage_mix_device": lambda run, seam: tracks_stage(run, seam, samples=True, mix=six if not seam else MC.MATRICES["2to1"]),
        "RRX_tracks_stage_mix_window_device": lambda run, seam: tracks_stage(run, seam, samples=True, window=True,
                                                                             mix=six if not seam else MC.MATRICES["2to1"]),
    }


_cache = None


def rows():
    global _cache
    if _cache is None:
        _cache = _rows()
    return _cache


# ------------------------------------------------------------------------------------------------------- the Python wrappers

# the thin wrapper of foo_dsp_resampler_amd/ratelib.py that takes `stream=` for each entry point
WRAPPER_OF = {
    "RRX_lpc_extrapolate_device": "lpc_extrapolate_device", "RRX_finish_device": "finish_device",
    "RRX_finish_shaped_device": "finish_shaped_device", "RRX_true_peak_device": "true_peak_device",
    "RRX_tracks_stage_device": "tracks_stage_device", "RRX_tracks_stage_device_samples": "tracks_stage_device",
    "RRX_tracks_finish_device": "tracks_finish_device", "RRX_tracks_finish_shaped_device": "tracks_finish_shaped_device",
    "RRX_tracks_true_peak_device": "tracks_true_peak_device", "RRX_tracks_true_peak_packed_device": "tracks_true_peak_packed_device",
    "RRX_limit_device": "limit_device", "RRX_tracks_limit_device": "tracks_limit_device", "RRX_limit_release_device": "limit_release_device",
    "RRX_tracks_limit_release_device": "tracks_limit_release_device", "RRX_loudness_device": "loudness_device",
    "RRX_tracks_loudness_device": "tracks_loudness_device", "RRX_tracks_loudness_packed_device": "tracks_loudness_packed_device",
    "RRX_loudness_gate_device": "loudness_gate_device", "RRX_loudness_blocks_device": "loudness_blocks_device",
    "RRX_loudness_gate_groups_device": "loudness_gate_groups_device", "RRX_loudness_range_groups_device": "loudness_range_device",
    "RRX_tracks_stage_window_device": "tracks_stage_window_device", "RRX_tracks_finish_window_device": "tracks_finish_window_device",
    "RRX_tracks_finish_shaped_window_device": "tracks_finish_shaped_window_device",
    "RRX_tracks_true_peak_window_device": "tracks_true_peak_window_device", "RRX_tracks_loudness_window_device": "tracks_loudness_window_device",
    "RRX_tracks_limit_window_device": "tracks_limit_window_device", "RRX_tracks_limit_release_window_device": "tracks_limit_release_window_device",
    "RRX_mix_device": "mix_device", "RRX_tracks_stage_mix_device": "tracks_stage_mix_device",
    "RRX_tracks_stage_mix_window_device": "tracks_stage_mix_window_device",
}
# the rows above that make the wrapper's call themselves, behind their C call, on the same guarded buffers
WRAPPER_IN_ROW = ("RRX_lpc_extrapolate_device", "RRX_tracks_stage_device", "RRX_tracks_stage_device_samples", "RRX_tracks_stage_window_device",
                  "RRX_mix_device", "RRX_tracks_stage_mix_device", "RRX_tracks_stage_mix_window_device")
# a wrapper that is not called behind gates, with its reason
WRAPPER_EXEMPT = {}
SEED = 0x1234567887654321
W_ROW = 700


def _w_streams():
    """(x float32 [2, 1025, 2] with peaks above the ceiling, gain [2])"""
    return dev((rng(20).standard_normal((2, 1025, 2)) * 0.25).astype(np.float32)), dev(np.array([0.75, 1.25]))


def _w_tracks():
    """(rows float32 [3, 700, 2], device table of slices with a packed destination, gain [3], frames of the destination)"""
    tab = slices_table(3, W_ROW)
    tab[:, 5] = np.cumsum(tab[:, 4]) - tab[:, 4]
    return dev((rng(21).standard_normal((3, W_ROW, 2)) * 0.25).astype(np.float32)), dev(tab), dev(np.array([0.5, 0.75, 1.0])), int(tab[:, 4].sum())


def _w_energy():
    """(hop energies [3, 2, 40], hops [3], channel weights [2])"""
    r = rng(22)
    e = r.uniform(1.0, 50.0, (3, 2, 40)) * r.choice([1.0, 0.01, 1e-12], size=(3, 1, 40), p=[0.5, 0.3, 0.2])
    return dev(e), dev(np.array([40, 17, 3], np.int64)), dev(np.array([1.0, 1.41]))


def _w_blocks():
    """(blocks [8, 10], nblocks [8], groups int32 [8] of 3 groups)"""
    r = rng(23)
    return dev(r.uniform(1.0, 50.0, (8, 10))), dev(np.array([10, 0, 3, 7, 10, 1, 5, 9], np.int64)), dev(np.array([0, 1, 2, 0, 1, 2, 0, -1], np.int32))


def _k48():
    import loudness_model as LM
    return [float(v) for v in np.asarray(LM.K48).reshape(-1)]


def _wrapper_rows():
    """entry point -> row(run): the wrapper's call behind the gates, on small inputs; what the wrapper allocates and returns counts
    as its output.  An output of which a call writes a part only (a packed destination under a window, the slices of rows) is
    passed in, behind a guard: torch.empty would hand the two runs different bytes there."""
    import torch
    S16 = F.RRX_FMT_S16

    def streams(entry, fn):
        def row(run):
            x, gain = _w_streams()
            run(lambda s: fn(x, gain, s), [x, gain], [], entry)
        return row

    def tracks(entry, fn, out=None):
        def row(run):
            rows, tab, gain, total = _w_tracks()
            outs = [] if out is None else [out(rows, total)]
            run(lambda s: fn(rows, tab, gain, total, s, *outs), [rows, tab, gain], outs, entry)
        return row

    def window(lo, n):
        return lambda rows: rows[:, lo:lo + n].contiguous()

    def win_row(entry, fn, out=None):
        def row(run):
            rows, tab, gain, total = _w_tracks()
            win = window(0, 300)(rows)
            outs = [] if out is None else [out(rows, total)]
            run(lambda s: fn(win, tab, gain, total, s, *outs), [win, tab, gain], outs, entry)
        return row

    def packed(entry, fn):
        def row(run):
            lengths, total, x, table, gain = _packed_case()
            run(lambda s: fn(x, table, gain, max(lengths), s), [x, table, gain], [], entry)
        return row

    def energy(entry, fn):
        def row(run):
            e, hops, w = _w_energy()
            run(lambda s: fn(e, hops, w, s), [e, hops, w], [], entry)
        return row

    def blocks(entry, fn):
        def row(run):
            b, nb, grp = _w_blocks()
            run(lambda s: fn(b, nb, grp, s), [b, nb, grp], [], entry)
        return row

    pcm = lambda rows, total: torch.full((total, 2), 0x5A5A, dtype=torch.int16, device="cuda")
    like64 = lambda rows, total: torch.full(tuple(rows.shape), GUARD, dtype=torch.float64, device="cuda")
    win64 = lambda rows, total: torch.full((rows.shape[0], 300, 2), GUARD, dtype=torch.float64, device="cuda")
    k48 = _k48()
    table = [
        streams("RRX_finish_device", lambda x, g, s: F.finish_device(x, S16, gain=g, dither=True, seed=SEED, first_frame=7, stream=s)),
        streams("RRX_finish_shaped_device", lambda x, g, s: F.finish_shaped_device(x, S16, "wannamaker9", segment=256, gain=g, seed=SEED, stream=s)),
        streams("RRX_true_peak_device", lambda x, g, s: F.true_peak_device(x, gain=g, stream=s)),
        streams("RRX_limit_device", lambda x, g, s: F.limit_device(x, CEILING, gain=g, lookahead=64, hold=0, stream=s)),
        streams("RRX_limit_release_device", lambda x, g, s: F.limit_release_device(x, CEILING, 0.999, gain=g, lookahead=64, block=64, stream=s)),
        streams("RRX_loudness_device", lambda x, g, s: F.loudness_device(x, gain=g, coefs=k48, hop=16, stream=s)),
        tracks("RRX_tracks_finish_device", lambda r, t, g, n, s: F.tracks_finish_device(r, t, S16, n, gain=g, dither=True, seed=SEED, stream=s)),
        tracks("RRX_tracks_finish_shaped_device",
               lambda r, t, g, n, s: F.tracks_finish_shaped_device(r, t, S16, n, "wannamaker9", segment=64, gain=g, seed=SEED, stream=s)),
        tracks("RRX_tracks_true_peak_device", lambda r, t, g, n, s: F.tracks_true_peak_device(r, t, gain=g, stream=s)),
        tracks("RRX_tracks_loudness_device", lambda r, t, g, n, s: F.tracks_loudness_device(r, t, gain=g, coefs=k48, hop=16, stream=s)),
        tracks("RRX_tracks_limit_device", lambda r, t, g, n, s, y: F.tracks_limit_device(r, t, CEILING, gain=g, out=y, stream=s)[1:], out=like64),
        tracks("RRX_tracks_limit_release_device",
               lambda r, t, g, n, s, y: F.tracks_limit_release_device(r, t, CEILING, 0.999, gain=g, block=64, out=y, stream=s)[1:], out=like64),
        tracks("RRX_tracks_limit_window_device",
               lambda r, t, g, n, s, y: F.tracks_limit_window_device(r, t, W_ROW, 0, 100, 300, CEILING, gain=g, out=y, stream=s)[1:], out=win64),
        tracks("RRX_tracks_limit_release_window_device",
               lambda r, t, g, n, s, y: F.tracks_limit_release_window_device(r, t, W_ROW, 0, 0, 300, CEILING, 0.999, gain=g, block=64, out=y,
                                                                             stream=s)[1:], out=win64),
        win_row("RRX_tracks_finish_window_device",
                lambda w, t, g, n, s, o: F.tracks_finish_window_device(w, t, W_ROW, 0, 300, S16, n, gain=g, dither=True, seed=SEED, out=o, stream=s)[1:],
                out=pcm),
        win_row("RRX_tracks_finish_shaped_window_device",
                lambda w, t, g, n, s, o: F.tracks_finish_shaped_window_device(w, t, W_ROW, 0, 300, S16, n, "wannamaker9", segment=64, gain=g, seed=SEED,
                                                                              out=o, stream=s)[1:], out=pcm),
        win_row("RRX_tracks_true_peak_window_device", lambda w, t, g, n, s: F.tracks_true_peak_window_device(w, t, W_ROW, 0, 300, gain=g, stream=s)),
        win_row("RRX_tracks_loudness_window_device",
                lambda w, t, g, n, s: F.tracks_loudness_window_device(w, t, W_ROW, 0, 300, gain=g, coefs=k48, hop=16, stream=s)),
        packed("RRX_tracks_true_peak_packed_device", lambda x, t, g, m, s: F.tracks_true_peak_packed_device(x, t, gain=g, max_frames=m, stream=s)),
        packed("RRX_tracks_loudness_packed_device",
               lambda x, t, g, m, s: F.tracks_loudness_packed_device(x, t, gain=g, coefs=k48, hop=16, max_frames=m, stream=s)),
        energy("RRX_loudness_gate_device", lambda e, h, w, s: F.loudness_gate_device(e, 16, hops=h, weights=w, stream=s)),
        energy("RRX_loudness_blocks_device", lambda e, h, w, s: F.loudness_blocks_device(e, 16, 4, 1, hops=h, weights=w, stream=s)),
        blocks("RRX_loudness_gate_groups_device", lambda b, nb, grp, s: F.loudness_gate_groups_device(b, nb, grp, 3, stream=s)),
        blocks("RRX_loudness_range_groups_device", lambda b, nb, grp, s: F.loudness_range_device(b, nb, grp, 3, stream=s)),
    ]
    return dict(zip(WRAPPER_ROWS, table))


WRAPPER_ROWS = ("RRX_finish_device", "RRX_finish_shaped_device", "RRX_true_peak_device", "RRX_limit_device", "RRX_limit_release_device",
                "RRX_loudness_device", "RRX_tracks_finish_device", "RRX_tracks_finish_shaped_device", "RRX_tracks_true_peak_device",
                "RRX_tracks_loudness_device", "RRX_tracks_limit_device", "RRX_tracks_limit_release_device", "RRX_tracks_limit_window_device",
                "RRX_tracks_limit_release_window_device", "RRX_tracks_finish_window_device", "RRX_tracks_finish_shaped_window_device",
                "RRX_tracks_true_peak_window_device", "RRX_tracks_loudness_window_device", "RRX_tracks_true_peak_packed_device",
                "RRX_tracks_loudness_packed_device", "RRX_loudness_gate_device", "RRX_loudness_blocks_device", "RRX_loudness_gate_groups_device",
                "RRX_loudness_range_groups_device")
_wcache = None


def wrapper_rows():
    global _wcache
    if _wcache is None:
        _wcache = _wrapper_rows()
        assert tuple(_wcache) == WRAPPER_ROWS
    return _wcache


# rows that go through tests/seam_cases.py run 32771 streams or tracks in their one case: it is their small case and their seam case
SEAM_IS_THE_CASE = ("RRX_finish_device", "RRX_finish_shaped_device", "RRX_true_peak_device", "RRX_tracks_finish_device",
                    "RRX_tracks_finish_shaped_device", "RRX_tracks_true_peak_device", "RRX_loudness_device", "RRX_tracks_loudness_device",
                    "RRX_loudness_gate_device", "RRX_loudness_blocks_device", "RRX_tracks_finish_window_device",
                    "RRX_tracks_finish_shaped_window_device")
# launchers without a loop over slices of 32768: one workgroup per (stream, channel, direction) of a 32-bit grid.x, the packed
# scans (a grid over tracks in x), and the group kernels, whose chunk loops of 64 and 256 streams their one case crosses
SEAMLESS = ("RRX_lpc_extrapolate_device", "RRX_tracks_true_peak_packed_device", "RRX_tracks_loudness_packed_device",
            "RRX_loudness_gate_groups_device", "RRX_loudness_range_groups_device")

# the handle calls: which group of tests/test_gpu_stream_order.py holds them
HANDLE_CALLS = {
    "RRX_push_device": "handle script", "RRX_pull_device": "handle script", "RRX_flow_device": "handle script",
    "RRX_push_device_double": "handle script, float64", "RRX_pull_device_double": "handle script, float64",
    "RRX_flow_device_double": "handle script, float64",
    "RRX_push_device_samples": "handle script, S16", "RRX_pull_device_samples": "handle script, S16", "RRX_flow_device_samples": "handle script, S16",
    "RRX_reset": "handle script: in the middle of the second pass", "RRX_set_stream": "handle script and the switch case",
}

# entry points that a row would not fit, each with its reason
EXEMPT = {}


def header_entries(text):
    """(entry points of the header whose parameter list names hip_stream, the handle's device calls with RRX_reset and
    RRX_set_stream) as two sorted lists"""
    protos = re.findall(r"^[A-Za-z_][\w \t\*]*?[ \t\*](RRX_\w+)[ \t]*\(([^;{}]*)\)\s*;", text, re.M)  # any return type
    free = sorted(n for n, args in protos if "hip_stream" in args and n != "RRX_set_stream")
    handle = sorted(n for n, args in protos if args.lstrip().startswith("RR_handle *h")
                    and (re.search(r"_(push|pull|flow)_device", n) or n in ("RRX_reset", "RRX_set_stream")))
    return free, handle
