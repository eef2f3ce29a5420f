"""What the tests of RRX_tracks_finish_shaped_window_device share (tests/test_tracks_shaped_window_api.py on the host,
tests/test_gpu_tracks_shaped_window.py on the device): a table of tracks whose slices begin at different frames of their rows,
the partitions of the rows into windows, the reference -- shaped_model.model per track on its slice, with the track's shifted
seed, first_frame = 0 and no state, i.e. what the whole-row call is documented to equal -- and callers of the host twin and of
the device call that walk a partition with two ping-ponged state buffers."""
import ctypes as C
import functools

import numpy as np

import foo_dsp_resampler_amd as F
import shaped_model as SM
from test_tracks_window_api import finish_model as cut_model   # the window cut in plain Python integers: [w0, w1, index, dst_frame]

SEED = 0x1234567887654321
MIX = 0xBF58476D1CE4E5B9
ORDER = SM.ORDER
GUARD = 0xA5
POISON = 1e30                                                 # in the frames between win_frames and win_stride: never read
R = 700                                                       # pitch of the (virtual) output rows
# (out_first, out_frames): the whole row but its edges; a track that ends before the last window (of every partition but
# "16 singles", whose last window is the rest of the row); a zero-length track; a track that begins after the first window; a track that ends with the row
SLICES = [(5, 690), (0, 250), (17, 0), (400, 290), (37, 663)]
SEG_CUTS = [5 + 64 * k for k in (1, 2, 5, 9)]                 # segment boundaries of track 0 at segment 64 (and 16, and 1)


def table_of(slices=SLICES):
    """(table uint64 [n, 6], dst_total): the slices packed end to end in the destination"""
    tab = np.zeros((len(slices), 6), np.uint64)
    pos = 0
    for t, (of, n) in enumerate(slices):
        tab[t] = (0, 0, 0, of, n, pos)
        pos += n
    return tab, pos


def even(step, n=R):
    return [(a, min(step, n - a)) for a in range(0, n, step)]


def cuts(points, n=R):
    edges = [0] + list(points) + [n]
    return [(a, b - a) for a, b in zip(edges, edges[1:])]


PARTITIONS = {"one": even(R), "7": even(7), "333": even(333), "16 singles": [(a, 1) for a in range(16)] + [(16, R - 16)],
              "on segment boundaries": cuts(SEG_CUTS)}


def track_seed(t, nch, seed=SEED):
    return (seed + t * nch * MIX) % 2 ** 64


@functools.lru_cache(maxsize=None)
def rows_of(ntracks, nch, fmt, double, frames=R):
    """seeded noise with finish_model's planted values (NaN, +-inf, ties, ...) in every row; read-only"""
    return SM.make_input(ntracks, frames, nch, fmt, double)


def whole_model(x, tab, dst_total, fmt, write, coefs, segment, gains, dith, seed=SEED):
    """the whole-row call by its documentation: (bytes uint8 [dst_total * nch * size] with GUARD where no track writes, or None;
    peak bits [n, nch]; clipped [n, nch]; the history after every track's last frame [n, nch, 16]; NaN channels [n, nch])"""
    n, rows, nch = x.shape
    nb = SM.NBYTES[fmt]
    raw = np.full(dst_total * nch * nb, GUARD, np.uint8) if write else None
    pk, cl = np.zeros((n, nch), np.uint64), np.zeros((n, nch), np.uint64)
    st, nan = np.zeros((n, nch, ORDER)), np.zeros((n, nch), bool)
    for t in range(n):
        w0, w1, index, df = cut_model([int(v) for v in tab[t]], rows, dst_total, write, 0, rows)
        if w1 == w0:
            continue
        sl = np.array(x[t, w0:w1])[None]
        g = None if gains is None else np.asarray(gains, dtype=np.float64)[t:t + 1]
        o, p, c, s = SM.model(sl, fmt, coefs, segment, g, dith, (seed + t * nch * MIX) % 2 ** 64, 0, None, write=write)
        if write:
            raw[df * nch * nb:(df + w1 - w0) * nch * nb] = o.reshape(-1)
        pk[t], cl[t], st[t], nan[t] = p[0], c[0], s[0], np.isnan(sl[0]).any(axis=0)
    return raw, pk, cl, st, nan


def same(got, want, what, state=True):
    """bytes, clip counts and the state bit for bit; peaks bit for bit except that of a channel with a NaN, which must be a NaN"""
    raw, pk, cl, st, nan = want
    assert (got[0] is None) == (raw is None), ("output",) + what
    if raw is not None:
        assert np.array_equal(got[0], raw), ("output bytes", int((got[0] != raw).sum())) + what
    assert np.array_equal(got[1][~nan], pk[~nan]), ("peak bit patterns",) + what
    assert np.isnan(got[1].view(np.float64)[nan]).all(), ("peak of a NaN channel",) + what
    assert np.array_equal(got[2], cl), ("clip counts",) + what
    if state:
        assert np.array_equal(got[3].view(np.uint64), st.view(np.uint64)), ("state",) + what


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def window_of(x, wf, wn, pad=2):
    """frames [wf, wf + wn) of every row as a window buffer of wn + pad frames a row, poison behind win_frames"""
    win = np.full((x.shape[0], wn + pad, x.shape[2]), POISON, x.dtype)
    win[:, :wn] = x[:, wf:wf + wn]
    return win


def host_call(tab, win, rows, wf, wn, fmt, dst, dst_total, gains, dith, seed, coefs, segment, sin, sout, pk, cl, rc=0, shape=None):
    """RRX_debug_tracks_finish_shaped_window_host on numpy arrays, every pointer as given (None: NULL; `shape`: that of a NULL window)"""
    n, stride, nch = shape if win is None else win.shape
    k = np.ascontiguousarray(coefs, dtype=np.float64)
    g = None if gains is None else np.ascontiguousarray(gains, dtype=np.float64)
    got = F.lib().RRX_debug_tracks_finish_shaped_window_host(_ptr(tab), n, nch, F.RRX_FMT_DOUBLE if win is not None and win.dtype == np.float64 else F.RRX_FMT_FLOAT,
                                                             _ptr(win), stride, rows, wf, wn, fmt, _ptr(dst), dst_total, _ptr(g), int(dith), seed,
                                                             _ptr(k), len(k), segment, _ptr(sin), _ptr(sout), _ptr(pk), _ptr(cl))
    assert got == rc, got
    return got


def host_windows(x, tab, dst_total, part, fmt, write, coefs, segment, gains, dith, seed=SEED, pre=65):
    """the host twin over the windows of `part` in the order given: one destination `pre` bytes into a guarded buffer, one pair of
    statistics, two state buffers handed to and fro (no state for a window at frame 0).  Before every call the receiving state is
    filled with 77, so an entry the call leaves out shows; after it, the entries of every track without a frame in the window
    must be those that came in (zeros without a state).  (bytes or None, peak bits, clipped, state after the last window)"""
    n, rows, nch = x.shape
    nb = SM.NBYTES[fmt]
    tab = np.ascontiguousarray(tab)
    nbytes = dst_total * nch * nb
    buf = np.full(pre + nbytes + 64, GUARD, np.uint8) if write else None
    dst = buf[pre:pre + nbytes] if write else None
    pk, cl = np.zeros((n, nch), np.uint64), np.zeros((n, nch), np.uint64)
    states = [np.zeros((n, nch, ORDER)), np.zeros((n, nch, ORDER))]
    for wf, wn in part:
        sin = None if wf == 0 else states[0]
        states[1][:] = 77.0
        host_call(tab, window_of(x, wf, wn), rows, wf, wn, fmt, dst, dst_total, gains, dith, seed, coefs, segment, sin, states[1], pk, cl)
        assert not (states[1] == 77.0).any(), ("entries of the state were not written", wf, wn)
        for t in range(n):
            c = cut_model([int(v) for v in tab[t]], rows, dst_total, write, wf, wn)
            if c[1] == c[0]:
                want = np.zeros((nch, ORDER)) if sin is None else sin[t]
                assert np.array_equal(states[1][t].view(np.uint64), want.view(np.uint64)), ("the state of an untouched track", t, wf, wn)
        states.reverse()
    if write:
        assert (buf[:pre] == GUARD).all() and (buf[pre + nbytes:] == GUARD).all(), "bytes around the destination were written"
    return (dst.copy() if write else None), pk, cl, states[0]


def device_windows(x, tab, dst_total, part, fmt, write, coefs, segment, gains, dith, seed=SEED, pre=65, stream=None):
    """host_windows on the device (RRX_tracks_finish_shaped_window_device): every window is handed over as a buffer of
    win_frames + 2 frames a row with poison behind win_frames, the destination lies `pre` bytes into a guarded byte buffer, and the
    state goes through two tensors handed to and fro, each with 8 guard doubles on either side and filled with 77 before it
    receives.  Returns what host_windows returns."""
    import torch
    n, rows, nch = x.shape
    nb = SM.NBYTES[fmt]
    F.ratelib._ensure_init()
    xd = torch.from_numpy(np.array(x)).cuda()
    table = torch.from_numpy(np.ascontiguousarray(tab).view(np.int64)).cuda()
    g = None if gains is None else torch.from_numpy(np.ascontiguousarray(gains, dtype=np.float64)).cuda()
    nbytes = dst_total * nch * nb
    buf = torch.full((pre + nbytes + 64,), GUARD, dtype=torch.uint8, device="cuda") if write else None
    pk = torch.zeros((n, nch), dtype=torch.int64, device="cuda")
    cl = torch.zeros((n, nch), dtype=torch.int64, device="cuda")
    states = [torch.full((8 + n * nch * ORDER + 8,), 77.0, dtype=torch.float64, device="cuda") for _ in range(2)]
    k = np.ascontiguousarray(coefs, dtype=np.float64)
    vp = C.c_void_p
    fn = F.lib().RRX_tracks_finish_shaped_window_device
    for wf, wn in part:
        win = torch.full((n, wn + 2, nch), POISON, dtype=xd.dtype, device="cuda")
        win[:, :wn] = xd[:, wf:wf + wn]
        states[1].fill_(77.0)
        rc = fn(-1, vp(getattr(stream, "cuda_stream", 0) or 0), vp(table.data_ptr()), n, nch, F.RRX_FMT_DOUBLE if x.dtype == np.float64 else F.RRX_FMT_FLOAT,
                vp(win.data_ptr()), wn + 2, rows, wf, wn, fmt, vp(buf.data_ptr() + pre) if write else None, dst_total,
                vp(g.data_ptr()) if g is not None else None, int(dith), seed, vp(k.ctypes.data), len(k), segment,
                None if wf == 0 else vp(states[0].data_ptr() + 64), vp(states[1].data_ptr() + 64), vp(pk.data_ptr()), vp(cl.data_ptr()))
        assert rc == 0, (rc, wf, wn)
        states.reverse()
    if stream is not None:
        stream.synchronize()
    raw = None
    if write:
        host = buf.cpu().numpy()
        assert (host[:pre] == GUARD).all() and (host[pre + nbytes:] == GUARD).all(), "bytes around the destination were written"
        raw = host[pre:pre + nbytes]
    st, other = states[0].cpu().numpy(), states[1].cpu().numpy()
    assert all((s[:8] == 77.0).all() and (s[-8:] == 77.0).all() for s in (st, other)), "doubles outside the state were written"
    assert not (st[8:-8] == 77.0).any(), "entries of the state were not written"
    assert np.array_equal(xd.cpu().numpy().view(np.uint8), np.array(x).view(np.uint8)), "the rows were written"
    return raw, pk.cpu().numpy().view(np.uint64), cl.cpu().numpy().view(np.uint64), st[8:-8].reshape(n, nch, ORDER).copy()
