"""numpy restatement of the shaped output stage's arithmetic (include/ratelib_amd.h, RRX_finish_shaped_device) and ctypes callers
of its host twin and of the device call, with finish_model.device's guard-byte layout.  The dither, the test inputs and the
planted edge values are finish_model's.

The model is vectorised over (stream, segment, channel) and loops over the position inside the segment: segments are independent
chains, which is the point of the ABI."""
import ctypes as C

import numpy as np

import foo_dsp_resampler_amd as F
from finish_model import BITS, NBYTES, GUARD, dither, make_input, planted, nan_channels  # noqa: F401  (re-exported for the tests)

ORDER = F.RRX_SHAPE_MAX_ORDER
FORMATS = (F.RRX_FMT_S16, F.RRX_FMT_S24_3, F.RRX_FMT_S32)
W9 = F.NOISE_SHAPES["wannamaker9"]
L5 = F.NOISE_SHAPES["lipshitz5"]


def coefs_of(order, seed=3):
    """a filter of `order` taps: the presets where they have that order, else seeded values of their size"""
    if order == 5:
        return np.array(L5)
    if order == 9:
        return np.array(W9)
    if order == 1:
        return np.array([0.75])
    return np.random.default_rng([seed, order]).uniform(-1.5, 1.5, order) * 0.9 ** np.arange(order)


def random_state(nstreams, nch, order, seed=5):
    """an incoming history: errors of the size real ones have, zeros from `order` on"""
    st = np.zeros((nstreams, nch, ORDER))
    st[:, :, :order] = np.random.default_rng([seed, nstreams, nch, order]).uniform(-1.2, 1.2, (nstreams, nch, order))
    return st


def restarts(F0, segment):
    return F0 % segment == 0 if segment else F0 == 0


def model(x, fmt, coefs, segment, gain=None, dith=True, seed=0, first_frame=0, state=None, peak=None, clipped=None, write=True):
    """x: float32 / float64 [nstreams, frames, nch].  Returns (bytes uint8 [nstreams, frames, nch * size] or None (write=False),
    peak bit patterns uint64 [nstreams, nch], clipped uint64 [nstreams, nch], state float64 [nstreams, nch, 16])."""
    S, n, nch = x.shape
    coefs = np.asarray(coefs, dtype=np.float64)
    order = len(coefs)
    bits = BITS[fmt]
    lo, hi = -2.0 ** bits, 2.0 ** bits - 1
    with np.errstate(invalid="ignore", over="ignore"):
        g = x.astype(np.float64)
        if gain is not None:
            g = g * np.asarray(gain, dtype=np.float64)[:, None, None]
        a = np.abs(g)
        t = g * 2.0 ** bits
        d = dither(seed, first_frame, n, S, nch) if dith else None
        # segment j of the call holds the call's frames [j * segment - pos0, (j + 1) * segment - pos0), cut to [0, n)
        seglen = segment if segment else first_frame + n
        pos0 = first_frame % segment if segment else first_frame
        nseg = (pos0 + n + seglen - 1) // seglen if n else 0
        E = np.zeros((S, nseg, nch, order))
        if nseg and not restarts(first_frame, segment):
            E[:, 0] = state[:, :, :order]
        q_all = np.zeros((S, n, nch))
        clip_all = np.zeros((S, n, nch), bool)
        # (one segment: its frames are the call's, whatever the numbers; several: the segment is no longer than the call)
        starts = np.zeros(1, np.int64) if nseg == 1 else np.arange(nseg, dtype=np.int64) * seglen - pos0
        for p in range(n if nseg == 1 else seglen):
            idx = starts + p
            v = (idx >= 0) & (idx < n)
            if not v.any():
                continue
            i = idx[v]
            e = E[:, v]                                   # [S, segments at work, nch, order]
            acc = np.zeros(e.shape[:3])
            for k in range(order, 0, -1):
                acc = acc + coefs[k - 1] * e[..., k - 1]
            w = t[:, i] - acc
            u = w + d[:, i] if dith else w
            q = np.rint(u)
            clip_all[:, i] = ~((q >= lo) & (q <= hi))
            q_all[:, i] = np.fmin(np.fmax(q, lo), hi)     # fmax / fmin return their other operand for a NaN, as C's do
            err = q - w
            err[~(np.abs(err) <= 2.0)] = 0.0
            e[..., 1:] = e[..., :-1].copy()
            e[..., 0] = err
            E[:, v] = e
    out = None
    if write:
        wide = "<i2" if fmt == F.RRX_FMT_S16 else "<i4"
        out = np.ascontiguousarray(q_all.astype(np.int64).astype(wide)).view(np.uint8).reshape(S, n, nch, -1)
        out = np.ascontiguousarray(out[..., :NBYTES[fmt]]).reshape(S, n, nch * NBYTES[fmt])
    pk = np.zeros((S, nch), np.uint64) if peak is None else peak.copy()
    if n:
        pk = np.maximum(pk, np.ascontiguousarray(a).view(np.uint64).max(axis=1))
    cl = (np.zeros((S, nch), np.uint64) if clipped is None else clipped.copy()) + clip_all.sum(axis=1).astype(np.uint64)
    st = np.zeros((S, nch, ORDER))
    if nseg:
        st[:, :, :order] = E[:, -1]
    return out, pk, cl, st


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _coefs(coefs):
    return np.ascontiguousarray(coefs, dtype=np.float64)


def host(x, fmt, coefs, segment, gain=None, dith=True, seed=0, first_frame=0, state=None, peak=None, clipped=None, write=True, rc=0):
    """RRX_debug_finish_shaped_host on numpy arrays: (bytes or None, peak bits, clipped, state out)"""
    S, n, nch = x.shape
    x = np.ascontiguousarray(x)
    nb = NBYTES[fmt]
    out = np.full((S, n, nch * nb), 0xA5, np.uint8) if write else None
    pk = np.zeros((S, nch), np.uint64) if peak is None else peak.copy()
    cl = np.zeros((S, nch), np.uint64) if clipped is None else clipped.copy()
    g = None if gain is None else np.ascontiguousarray(gain, dtype=np.float64)
    k = _coefs(coefs)
    sin = None if state is None else np.ascontiguousarray(state, dtype=np.float64)
    sout = np.full((S, nch, ORDER), 77.0)
    got = F.lib().RRX_debug_finish_shaped_host(F.RRX_FMT_DOUBLE if x.dtype == np.float64 else F.RRX_FMT_FLOAT, _ptr(x), n, fmt, _ptr(out), n, S, n,
                                               nch, _ptr(g), int(dith), seed, first_frame, _ptr(k), len(k), segment, _ptr(sin), _ptr(sout),
                                               _ptr(pk), _ptr(cl))
    assert got == rc, got
    return out, pk, cl, sout


def device(x, fmt, coefs, segment, gain=None, dith=True, seed=0, first_frame=0, state=None, peak=None, clipped=None, write=True, pad=3, src_off=0,
           dst_off=0, stream=None):
    """RRX_finish_shaped_device on the rows of x placed `pad` frames apart inside larger device buffers that start `src_off` /
    `dst_off` SAMPLES behind an aligned address (finish_model.device's layout): (bytes or None, peak bits, clipped, state out) as
    numpy arrays.  Every byte of the destination buffer outside the rows must still hold the guard pattern afterwards, the state
    buffer's surroundings too, and the source must be unchanged."""
    import torch
    S, n, nch = x.shape
    nb = NBYTES[fmt]
    pitch = (n + pad) * nch                      # samples between streams
    F.ratelib._ensure_init()
    hb = np.full(16 + src_off + S * pitch + 16, 7.0, x.dtype)
    for s in range(S):
        hb[16 + src_off + s * pitch:][:n * nch] = x[s].ravel()
    src = torch.from_numpy(hb).cuda()
    dst = torch.full((64 + (dst_off + S * pitch) * nb + 64,), GUARD, dtype=torch.uint8, device="cuda") if write else None
    g = None if gain is None else torch.from_numpy(np.ascontiguousarray(gain, dtype=np.float64)).cuda()
    pk = torch.from_numpy((np.zeros((S, nch), np.uint64) if peak is None else peak).view(np.int64)).cuda()
    cl = torch.from_numpy((np.zeros((S, nch), np.uint64) if clipped is None else clipped).view(np.int64)).cuda()
    sin = None if state is None else torch.from_numpy(np.ascontiguousarray(state, dtype=np.float64)).cuda()
    sout = torch.full((8 + S * nch * ORDER + 8,), 77.0, dtype=torch.float64, device="cuda")
    k = _coefs(coefs)
    vp = C.c_void_p
    rc = F.lib().RRX_finish_shaped_device(-1, vp(getattr(stream, "cuda_stream", 0) or 0), F.RRX_FMT_DOUBLE if x.dtype == np.float64 else F.RRX_FMT_FLOAT,
                                          vp(src.data_ptr() + (16 + src_off) * x.itemsize), n + pad, fmt,
                                          vp(dst.data_ptr() + 64 + dst_off * nb) if dst is not None else None, n + pad, S, n, nch,
                                          vp(g.data_ptr()) if g is not None else None, int(dith), seed, first_frame, _ptr(k), len(k), segment,
                                          vp(sin.data_ptr()) if sin is not None else None, vp(sout.data_ptr() + 64),
                                          vp(pk.data_ptr()), vp(cl.data_ptr()))
    assert rc == 0, rc
    if stream is not None:
        stream.synchronize()
    out = None
    if dst is not None:
        raw = dst.cpu().numpy()
        rows = raw[64 + dst_off * nb:][:S * pitch * nb].reshape(S, pitch * nb)
        out = rows[:, :n * nch * nb].reshape(S, n, nch * nb).copy()
        rows[:, :n * nch * nb] = GUARD
        assert (raw == GUARD).all(), "bytes outside the destination rows were written"
    assert np.array_equal(src.cpu().numpy().view(np.uint8), hb.view(np.uint8)), "the source was written"
    st = sout.cpu().numpy()
    assert (st[:8] == 77.0).all() and (st[-8:] == 77.0).all(), "doubles outside the state were written"
    return out, pk.cpu().numpy().view(np.uint64), cl.cpu().numpy().view(np.uint64), st[8:-8].reshape(S, nch, ORDER).copy()


def same(got, want, x, what, state=True):
    """bytes, clip counts and the state bit for bit; peaks bit for bit except that of a channel with a NaN, which must be a NaN"""
    assert (got[0] is None) == (want[0] is None), ("output",) + what
    if want[0] is not None:
        assert np.array_equal(got[0], want[0]), ("output bytes",) + what
    nanch = nan_channels(x)
    assert np.array_equal(got[1][~nanch], want[1][~nanch]), ("peak bit patterns",) + what
    assert np.isnan(got[1].view(np.float64)[nanch]).all(), ("peak of the NaN channel",) + what
    assert np.array_equal(got[2], want[2]), ("clip counts",) + what
    if state:
        assert np.array_equal(got[3].view(np.uint64), want[3].view(np.uint64)), ("state",) + what
