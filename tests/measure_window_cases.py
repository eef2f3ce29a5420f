"""What the tests of RRX_tracks_true_peak_window_device and RRX_tracks_loudness_window_device share
(tests/test_tracks_measure_window_api.py on the host, tests/test_gpu_tracks_measure_window.py on the device): the rows, slices and
partitions of shaped_window_cases, the references -- a one-stream RRX_debug_true_peak_host / RRX_debug_loudness_host call per
track on its slice with first_frame = 0, no state and flush, which is what the whole-row calls are documented to equal -- and
callers of the host twins and of the device calls that walk a partition with two ping-ponged state buffers."""
import contextlib
import ctypes as C
import functools

import numpy as np

import foo_dsp_resampler_amd as F
import loudness_model as LM
import shaped_window_cases as W
import true_peak_model as TM
from test_tracks_window_api import finish_model as cut_model   # the window cut in plain Python integers: [w0, w1, index, dst_frame]

R = W.R
TAPS16 = 16                                                    # doubles per (track, channel) of both states
SENTINEL = 77.0
GUARD = -12345.0
GAINS = 0.5 + 0.4 * np.arange(len(W.SLICES))
FILTERS = {"1x1": np.array([[0.75]]), "bs1770": TM.BS1770, "8x16": np.random.default_rng(816).standard_normal((8, 16)) * 0.3,
           "2x2": np.array([[0.5, 0.5], [1.0, -0.25]])}
K = LM.K48


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def fmt_of(x):
    return F.RRX_FMT_DOUBLE if x.dtype == np.float64 else F.RRX_FMT_FLOAT


@functools.lru_cache(maxsize=None)
def rows_of(ntracks, nch, double, frames=R, seed=5):
    """finite seeded noise [ntracks, frames, nch]; read-only"""
    x = (np.random.default_rng(seed + 10 * nch + double).standard_normal((ntracks, frames, nch)) * 0.4).astype(np.float64 if double else np.float32)
    x.setflags(write=False)
    return x


def slices_of(tab, rows):
    """[(w0, w1)] per track: its clamped slice, as the whole-row calls cut it"""
    return [tuple(cut_model([int(v) for v in e], rows, 0, False, 0, rows)[:2]) for e in tab]


# ------------------------------------------------------------------------------------------------------------------ true peak
def tp_reference(x, tab, coefs, gains):
    """(true peak bits [n, nch], peak bits [n, nch], state after every track's last frame [n, nch, 16]) of the whole-row call by
    its documentation: RRX_debug_true_peak_host per track on its slice, held to true_peak_model on the way"""
    n, rows, nch = x.shape
    coefs = np.ascontiguousarray(coefs, dtype=np.float64)
    tp, pk, st = np.zeros((n, nch), np.uint64), np.zeros((n, nch), np.uint64), np.zeros((n, nch, TAPS16))
    for t, (w0, w1) in enumerate(slices_of(tab, rows)):
        if w1 == w0:
            continue
        sl = np.ascontiguousarray(x[t, w0:w1])[None]
        g = None if gains is None else np.ascontiguousarray(gains[t:t + 1], dtype=np.float64)
        a, b, s = np.zeros((1, nch), np.uint64), np.zeros((1, nch), np.uint64), np.zeros((1, nch, TAPS16))
        rc = F.lib().RRX_debug_true_peak_host(fmt_of(x), _ptr(sl), (w1 - w0) * nch, 1, w1 - w0, nch, _ptr(g), 0, _ptr(coefs), coefs.shape[0],
                                              coefs.shape[1], 1, None, _ptr(s), _ptr(a), _ptr(b))
        assert rc == 0, rc
        ma, mb, ms = TM.true_peak(sl, coefs, g, True, None)
        finite = np.isfinite(sl[0]).all(axis=0)
        assert np.array_equal(a[0][finite], ma[0][finite]) and np.array_equal(b[0][finite], mb[0][finite]), ("the model", t)
        assert np.array_equal(s[0][finite].view(np.uint64), ms[0][finite].view(np.uint64)), ("the model's state", t)
        tp[t], pk[t], st[t] = a[0], b[0], s[0]
    return tp, pk, st


def window_of(x, wf, wn, pad=2):
    """frames [wf, wf + wn) of every row as a window buffer of wn + pad frames a row, poison behind win_frames"""
    win = np.full((x.shape[0], wn + pad, x.shape[2]), W.POISON, x.dtype)
    win[:, :wn] = x[:, wf:wf + wn]
    return win


def tp_host_call(tab, win, rows, wf, wn, gains, coefs, sin, sout, tp, pk, rc=0, shape=None, phases=None, taps=None):
    n, stride, nch = shape if win is None else win.shape
    k = None if coefs is None else np.ascontiguousarray(coefs, dtype=np.float64)
    g = None if gains is None else np.ascontiguousarray(gains, dtype=np.float64)
    got = F.lib().RRX_debug_tracks_true_peak_window_host(_ptr(tab), n, nch, fmt_of(win) if win is not None else 0, _ptr(win), stride, rows, wf, wn,
                                                         _ptr(g), _ptr(k), k.shape[0] if phases is None else phases,
                                                         k.shape[1] if taps is None else taps, _ptr(sin), _ptr(sout), _ptr(tp), _ptr(pk))
    assert got == rc, got
    return got


def untouched_ok(tab, rows, wf, wn, sin, sout):
    """after a window: the entries of every track without a frame in it are those that came in (zeros without a state)"""
    for t in range(len(tab)):
        c = cut_model([int(v) for v in tab[t]], rows, 0, False, wf, wn)
        if c[1] == c[0]:
            want = np.zeros(sout[t].shape) if sin is None else sin[t]
            assert np.array_equal(sout[t].view(np.uint64), want.view(np.uint64)), ("the state of an untouched track", t, wf, wn)


def tp_host_windows(x, tab, part, coefs, gains, rows=None):
    """the host twin over the windows of `part` in the order given, two state buffers handed to and fro (no state for a window at
    frame 0), the receiving one pre-filled with a sentinel; (true peak bits, peak bits, state after the last window)"""
    n, rows_, nch = x.shape
    rows = rows_ if rows is None else rows
    tab = np.ascontiguousarray(tab)
    tp, pk = np.zeros((n, nch), np.uint64), np.zeros((n, nch), np.uint64)
    states = [np.zeros((n, nch, TAPS16)), np.zeros((n, nch, TAPS16))]
    for wf, wn in part:
        sin = None if wf == 0 else states[0]
        states[1][:] = SENTINEL
        tp_host_call(tab, window_of(x, wf, wn), rows, wf, wn, gains, coefs, sin, states[1], tp, pk)
        assert not (states[1] == SENTINEL).any(), ("entries of the state were not written", wf, wn)
        untouched_ok(tab, rows, wf, wn, sin, states[1])
        states.reverse()
    return tp, pk, states[0]


# ------------------------------------------------------------------------------------------------------------------- loudness
def ld_reference(x, tab, hop, gains, stride, c=K):
    """(energy [n, nch, stride] with GUARD where the whole-row call writes nothing, hops [n], the window state after every track's
    last whole hop [n, nch, 16]) by the documentation: RRX_debug_loudness_host per track on its slice, held to loudness_model"""
    n, rows, nch = x.shape
    c = np.ascontiguousarray(c, dtype=np.float64)
    energy, hops, st = np.full((n, nch, max(stride, 1)), GUARD), np.zeros(n, np.uint64), np.zeros((n, nch, TAPS16))
    for t, (w0, w1) in enumerate(slices_of(tab, rows)):
        k = min((w1 - w0) // hop, stride)
        hops[t] = k
        if not k:
            continue
        sl = np.ascontiguousarray(x[t, w0:w0 + k * hop])[None]
        g = None if gains is None else np.ascontiguousarray(gains[t:t + 1], dtype=np.float64)
        e, s, work = np.zeros((1, nch, k)), np.zeros((1, nch, 4)), np.zeros(nch * k * 4)
        rc = F.lib().RRX_debug_loudness_host(fmt_of(x), _ptr(sl), k * hop * nch, 1, k * hop, nch, _ptr(g), 0, _ptr(c), hop, None, _ptr(s), _ptr(e), k,
                                             _ptr(work), work.size)
        assert rc == 0, rc
        with np.errstate(all="ignore"):
            me, ms = LM.hop_energies(LM.gained(sl, g), c, hop)
        finite = np.isfinite(sl[0]).all(axis=0)
        assert np.array_equal(e[0][finite].view(np.uint64), me[0][finite].view(np.uint64)), ("the model", t)
        assert np.array_equal(s[0][finite].view(np.uint64), ms[0][finite].view(np.uint64)), ("the model's state", t)
        energy[t, :, :k] = e[0]
        st[t, :, 0:4] = s[0]                                  # on a hop boundary: S, Z = 0, C = S, E = +0.0
        st[t, :, 8:12] = s[0]
    return energy[:, :, :stride], hops, st


def work_doubles(n, nch, wn, hop):
    return n * nch * (wn // hop + 2) * 4


def ld_host_call(tab, win, rows, wf, wn, gains, hop, sin, sout, energy, stride, hops, work, rc=0, shape=None, c=K, work_doubles=None):
    n, wstride, nch = shape if win is None else win.shape
    k = None if c is None else np.ascontiguousarray(c, dtype=np.float64)
    g = None if gains is None else np.ascontiguousarray(gains, dtype=np.float64)
    got = F.lib().RRX_debug_tracks_loudness_window_host(_ptr(tab), n, nch, fmt_of(win) if win is not None else 0, _ptr(win), wstride, rows, wf, wn,
                                                        _ptr(g), _ptr(k), hop, _ptr(sin), _ptr(sout), _ptr(energy), stride, _ptr(hops), _ptr(work),
                                                        (0 if work is None else work.size) if work_doubles is None else work_doubles)
    assert got == rc, got
    return got


def ld_host_windows(x, tab, part, hop, gains, stride, rows=None):
    """the host twin over the windows of `part`; the energies lie between guard doubles, the work buffer is the size the call asks
    for and guarded too; (energy [n, nch, stride], hops [n], state after the last window)"""
    n, rows_, nch = x.shape
    rows = rows_ if rows is None else rows
    tab = np.ascontiguousarray(tab)
    buf = np.full(8 + n * nch * stride + 8, GUARD)
    energy = buf[8:8 + n * nch * stride]
    hops = np.full(n, 0xdead, np.uint64)
    states = [np.zeros((n, nch, TAPS16)), np.zeros((n, nch, TAPS16))]
    for wf, wn in part:
        need = work_doubles(n, nch, wn, hop)
        assert F.lib().RRX_tracks_loudness_window_work_doubles(n, nch, wn, hop) == need
        wbuf = np.full(8 + need + 8, GUARD)
        sin = None if wf == 0 else states[0]
        states[1][:] = SENTINEL
        ld_host_call(tab, window_of(x, wf, wn), rows, wf, wn, gains, hop, sin, states[1], energy, stride, hops, wbuf[8:8 + need])
        assert (wbuf[:8] == GUARD).all() and (wbuf[-8:] == GUARD).all(), "doubles around the work buffer were written"
        assert not (states[1] == SENTINEL).any(), ("entries of the state were not written", wf, wn)
        untouched_ok(tab, rows, wf, wn, sin, states[1])
        states.reverse()
    assert (buf[:8] == GUARD).all() and (buf[-8:] == GUARD).all(), "doubles around the energies were written"
    return energy.reshape(n, nch, stride).copy(), hops, states[0]


# ------------------------------------------------------------------------------------------------------------------ the device
def device_windows(x, tab, part, coefs, gains, hop, stride, rows=None, stream=None):
    """both device calls over the windows of `part`: every window handed over as a buffer of win_frames + 2 frames a row with poison
    behind win_frames; states, energies and work between 8 guard doubles, the receiving states pre-filled with a sentinel.
    ((true peak bits, peak bits, state), (energy, hops, state))"""
    import torch
    n, rows_, nch = x.shape
    rows = rows_ if rows is None else rows
    F.ratelib._ensure_init()
    vp = C.c_void_p
    L = F.lib()
    xd = torch.from_numpy(np.array(x)).cuda()
    table = torch.from_numpy(np.ascontiguousarray(tab).view(np.int64)).cuda()
    g = None if gains is None else torch.from_numpy(np.ascontiguousarray(gains, dtype=np.float64)).cuda()
    f64 = dict(dtype=torch.float64, device="cuda")
    tp, pk = torch.zeros((n, nch), dtype=torch.int64, device="cuda"), torch.zeros((n, nch), dtype=torch.int64, device="cuda")
    ebuf = torch.full((8 + n * nch * stride + 8,), GUARD, **f64)
    hops = torch.full((n,), 0xdead, dtype=torch.int64, device="cuda")
    tps = [torch.full((8 + n * nch * TAPS16 + 8,), SENTINEL, **f64) for _ in range(2)]
    lds = [torch.full((8 + n * nch * TAPS16 + 8,), SENTINEL, **f64) for _ in range(2)]
    for s in (tps[0], lds[0]):
        s[8:-8] = 0.0
    need = max(work_doubles(n, nch, wn, hop) for _, wn in part)
    wbuf = torch.full((8 + need + 8,), GUARD, **f64)
    k = np.ascontiguousarray(coefs, dtype=np.float64)
    c = np.ascontiguousarray(K, dtype=np.float64)
    sp = vp(getattr(stream, "cuda_stream", 0) or 0)
    fmt = fmt_of(x)
    gp = vp(g.data_ptr()) if g is not None else None
    torch.cuda.synchronize()
    # on a side stream torch's own work (the window tensors, the sentinels) runs there too, so one stream orders everything
    ctx = torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
    with ctx:
        _device_walk(L, part, xd, table, n, nch, rows, fmt, gp, k, c, hop, stride, sp, tps, lds, tp, pk, ebuf, hops, wbuf)
    torch.cuda.synchronize()
    out = []
    for s, o in ((tps[0], tps[1]), (lds[0], lds[1])):
        a, b = s.cpu().numpy(), o.cpu().numpy()
        assert all((v[:8] == SENTINEL).all() and (v[-8:] == SENTINEL).all() for v in (a, b)), "doubles outside a state were written"
        assert not (a[8:-8] == SENTINEL).any(), "entries of a state were not written"
        out.append(a[8:-8].reshape(n, nch, TAPS16).copy())
    e, w = ebuf.cpu().numpy(), wbuf.cpu().numpy()
    assert (e[:8] == GUARD).all() and (e[-8:] == GUARD).all(), "doubles around the energies were written"
    assert (w[:8] == GUARD).all() and (w[-8:] == GUARD).all(), "doubles around the work buffer were written"
    assert np.array_equal(xd.cpu().numpy().view(np.uint8), np.array(x).view(np.uint8)), "the rows were written"
    return ((tp.cpu().numpy().view(np.uint64), pk.cpu().numpy().view(np.uint64), out[0]),
            (e[8:-8].reshape(n, nch, stride).copy(), hops.cpu().numpy().view(np.uint64), out[1]))


def _device_walk(L, part, xd, table, n, nch, rows, fmt, gp, k, c, hop, stride, sp, tps, lds, tp, pk, ebuf, hops, wbuf):
    import torch
    vp = C.c_void_p
    for wf, wn in part:
        win = torch.full((n, wn + 2, nch), W.POISON, dtype=xd.dtype, device="cuda")
        win[:, :wn] = xd[:, wf:wf + wn]
        tps[1].fill_(SENTINEL)
        lds[1].fill_(SENTINEL)
        rc = L.RRX_tracks_true_peak_window_device(-1, sp, vp(table.data_ptr()), n, nch, fmt, vp(win.data_ptr()), wn + 2, rows, wf, wn, gp,
                                                  vp(k.ctypes.data), k.shape[0], k.shape[1], None if wf == 0 else vp(tps[0].data_ptr() + 64),
                                                  vp(tps[1].data_ptr() + 64), vp(tp.data_ptr()), vp(pk.data_ptr()))
        assert rc == 0, (rc, wf, wn)
        rc = L.RRX_tracks_loudness_window_device(-1, sp, vp(table.data_ptr()), n, nch, fmt, vp(win.data_ptr()), wn + 2, rows, wf, wn, gp,
                                                 vp(c.ctypes.data), hop, None if wf == 0 else vp(lds[0].data_ptr() + 64), vp(lds[1].data_ptr() + 64),
                                                 vp(ebuf.data_ptr() + 64), stride, vp(hops.data_ptr()), vp(wbuf.data_ptr() + 64),
                                                 work_doubles(n, nch, wn, hop))
        assert rc == 0, (rc, wf, wn)
        tps.reverse()
        lds.reverse()


def device_whole(x, tab, coefs, gains, hop, stride):
    """RRX_tracks_true_peak_device and RRX_tracks_loudness_device on the same rows: (true peak bits, peak bits, energy with GUARD
    where nothing is written, hops)"""
    import torch
    n, rows, nch = x.shape
    F.ratelib._ensure_init()
    vp = C.c_void_p
    L = F.lib()
    xd = torch.from_numpy(np.array(x)).cuda()
    table = torch.from_numpy(np.ascontiguousarray(tab).view(np.int64)).cuda()
    g = None if gains is None else torch.from_numpy(np.ascontiguousarray(gains, dtype=np.float64)).cuda()
    gp = vp(g.data_ptr()) if g is not None else None
    tp, pk = torch.zeros((n, nch), dtype=torch.int64, device="cuda"), torch.zeros((n, nch), dtype=torch.int64, device="cuda")
    k = np.ascontiguousarray(coefs, dtype=np.float64)
    c = np.ascontiguousarray(K, dtype=np.float64)
    assert L.RRX_tracks_true_peak_device(-1, None, vp(table.data_ptr()), n, nch, fmt_of(x), vp(xd.data_ptr()), rows, gp, vp(k.ctypes.data),
                                         k.shape[0], k.shape[1], vp(tp.data_ptr()), vp(pk.data_ptr())) == 0
    energy = torch.full((n, nch, stride), GUARD, dtype=torch.float64, device="cuda")
    hops = torch.zeros((n,), dtype=torch.int64, device="cuda")
    need = L.RRX_loudness_work_doubles(n, nch, rows, hop)
    work = torch.zeros((max(need, 1),), dtype=torch.float64, device="cuda")
    assert L.RRX_tracks_loudness_device(-1, None, vp(table.data_ptr()), n, nch, fmt_of(x), vp(xd.data_ptr()), rows, gp, vp(c.ctypes.data), hop,
                                        vp(energy.data_ptr()), stride, vp(hops.data_ptr()), vp(work.data_ptr()), need) == 0
    torch.cuda.synchronize()
    return tp.cpu().numpy().view(np.uint64), pk.cpu().numpy().view(np.uint64), energy.cpu().numpy(), hops.cpu().numpy().view(np.uint64)
