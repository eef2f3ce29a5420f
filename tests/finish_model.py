"""numpy restatement of the output stage's per-sample arithmetic (include/ratelib_amd.h, RRX_finish_device), the test inputs with
their planted edge values, and ctypes callers of the host twin and of the device call with explicit strides and offsets.

64-bit integer arithmetic is done on uint64 ARRAYS throughout: array arithmetic wraps, scalar arithmetic warns."""
import ctypes as C
import functools

import numpy as np

import foo_dsp_resampler_amd as F

BITS = {F.RRX_FMT_S16: 15, F.RRX_FMT_S24_3: 23, F.RRX_FMT_S32: 31}
NBYTES = {F.RRX_FMT_S16: 2, F.RRX_FMT_S24_3: 3, F.RRX_FMT_S32: 4}
FORMATS = (F.RRX_FMT_S16, F.RRX_FMT_S24_3, F.RRX_FMT_S32)
GAINS = (None, 0.5, 1.7)
SHAPES = [(1, 1), (1, 2), (3, 3), (2, 8)]        # nstreams, nch
FRAMES = (1, 5, 4099)


def u64(v):
    return np.array([int(v) & (2 ** 64 - 1)], dtype=np.uint64)


G1, M1, M2 = u64(0x9E3779B97F4A7C15), u64(0xBF58476D1CE4E5B9), u64(0x94D049BB133111EB)


def dither(seed, first_frame, frames, nstreams, nch):
    """d of every (stream, frame, channel) of a call, in LSB: float64 [nstreams, frames, nch]"""
    fr = (u64(first_frame) + np.arange(frames, dtype=np.uint64))[None, :, None]
    c = np.arange(nstreams * nch, dtype=np.uint64).reshape(nstreams, 1, nch)
    z = u64(seed) + fr * G1 + c * M1
    z = (z ^ (z >> np.uint64(30))) * M1
    z = (z ^ (z >> np.uint64(27))) * M2
    z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(32)).astype(np.float64) - (z & np.uint64(0xffffffff)).astype(np.float64)) * 2.0 ** -32


def model(x, fmt, gain=None, dith=False, seed=0, first_frame=0, peak=None, clipped=None):
    """x: float32 / float64 [nstreams, frames, nch]; gain: None or float64 [nstreams]; fmt None = measure only (the S32 quantiser).
    Returns (bytes uint8 [nstreams, frames, nch * size] or None, peak bit patterns uint64 [nstreams, nch], clipped uint64)."""
    S, n, nch = x.shape
    bits = BITS[fmt] if fmt is not None else 31
    lo, hi = -2.0 ** bits, 2.0 ** bits - 1
    with np.errstate(invalid="ignore", over="ignore"):
        g = x.astype(np.float64)
        if gain is not None:
            g = g * np.asarray(gain, dtype=np.float64)[:, None, None]
        a = np.abs(g)
        t = g * 2.0 ** bits
        if dith:
            t = t + dither(seed, first_frame, n, S, nch)
        q = np.rint(t)
        clip = ~((q >= lo) & (q <= hi))
        q = np.fmin(np.fmax(q, lo), hi)          # fmax / fmin return their other operand for a NaN, as C's do
    out = None
    if fmt is not None:
        wide = "<i2" if fmt == F.RRX_FMT_S16 else "<i4"   # packed 24 bit: the low three bytes of the 32-bit word
        out = np.ascontiguousarray(q.astype(np.int64).astype(wide)).view(np.uint8).reshape(S, n, nch, -1)
        out = np.ascontiguousarray(out[..., :NBYTES[fmt]]).reshape(S, n, nch * NBYTES[fmt])
    pk = np.zeros((S, nch), np.uint64) if peak is None else peak.copy()
    if n:
        pk = np.maximum(pk, np.ascontiguousarray(a).view(np.uint64).max(axis=1))
    cl = (np.zeros((S, nch), np.uint64) if clipped is None else clipped.copy()) + clip.sum(axis=1).astype(np.uint64)
    return out, pk, cl


def planted(bits):
    tie = lambda k: (k + 0.5) * 2.0 ** -bits
    tiny = np.array([1, 0x7fffff, 0x80000001], np.uint32).view(np.float32).astype(np.float64)   # float32 denormals
    return np.concatenate([[np.nan, 0.0, 1.0, -1.0, 1 - 2.0 ** -bits, -(1 - 2.0 ** -bits), tie(0), tie(1), tie(2), tie(7), tie(-1), tie(-2),
                            tie(-8), 3.0, -3.0, np.inf, -np.inf], tiny])


@functools.lru_cache(maxsize=None)
def make_input(nstreams, frames, nch, fmt, double, seed=1):
    """Seeded noise at about -6 dBFS (uniform on +-0.5) with the edge values of the format planted in every stream; the one NaN goes
    into stream 0 only.  Short inputs take as many of the values as they have room for, from a start that
    moves with the shape, so the small cases cover the list between them.  Read-only: the tests share it."""
    rng = np.random.default_rng([seed, nstreams, frames, nch])
    x = rng.uniform(-0.5, 0.5, (nstreams, frames, nch))
    p = planted(BITS[fmt])
    flat = x.reshape(nstreams, frames * nch)
    n = frames * nch
    if n >= 4 * len(p):
        for s in range(nstreams):
            pos = (np.arange(len(p)) * (n // len(p)) + 3 * s) % n
            flat[s, pos] = p
    else:
        for s in range(nstreams):
            k = (np.arange(n) + 1 + 5 * s + 3 * nch + frames) % len(p)
            k[k == 0] = 1 + s                     # the NaN is not part of the short cases
            flat[s] = p[k]
    x[1:][np.isnan(x[1:])] = 0.25
    x = x.astype(np.float64 if double else np.float32)
    x.setflags(write=False)
    return x


def nan_channels(x):
    return np.isnan(x).any(axis=1)                # [nstreams, nch]


@functools.lru_cache(maxsize=None)
def case(nstreams, frames, nch, fmt, double, gain, dith, seed=0x1234567887654321, first_frame=0):
    """(input, model output) of one case of the matrix, computed once per process"""
    x = make_input(nstreams, frames, nch, fmt if fmt is not None else F.RRX_FMT_S32, double)
    g = None if gain is None else gain * (1 + 0.25 * np.arange(nstreams))
    return x, g, model(x, fmt, g, dith, seed, first_frame)


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def host(x, fmt, gain=None, dith=False, seed=0, first_frame=0, peak=None, clipped=None, src_stride=None, dst_stride=None, write=True):
    """RRX_debug_finish_host on numpy arrays: (bytes or None, peak bits, clipped), accumulating into peak / clipped when given"""
    S, n, nch = x.shape
    x = np.ascontiguousarray(x)
    nb = NBYTES[fmt] if fmt is not None else 0
    out = np.full((S, n, nch * nb), 0xA5, np.uint8) if fmt is not None and write else None
    pk = np.zeros((S, nch), np.uint64) if peak is None else peak.copy()
    cl = np.zeros((S, nch), np.uint64) if clipped is None else clipped.copy()
    g = None if gain is None else np.ascontiguousarray(gain, dtype=np.float64)
    rc = F.lib().RRX_debug_finish_host(F.RRX_FMT_DOUBLE if x.dtype == np.float64 else F.RRX_FMT_FLOAT, _ptr(x), src_stride or n,
                                       fmt or 0, _ptr(out), dst_stride or n, S, n, nch, _ptr(g), int(dith), seed, first_frame, _ptr(pk), _ptr(cl))
    assert rc == 0, rc
    return out, pk, cl


GUARD = 0xA5


def device(x, fmt, gain=None, dith=False, seed=0, first_frame=0, peak=None, clipped=None, pad=3, src_off=0, dst_off=0, stream=None):
    """RRX_finish_device on the rows of x placed `pad` frames apart inside larger device buffers that start `src_off` / `dst_off`
    SAMPLES behind an aligned address: (bytes or None, peak bits, clipped) as numpy arrays.  Every byte of the destination buffer
    outside the rows must still hold the guard pattern afterwards."""
    import torch
    S, n, nch = x.shape
    nb = NBYTES[fmt] if fmt is not None else 0
    pitch = (n + pad) * nch                      # samples between streams
    F.ratelib._ensure_init()
    hb = np.full(16 + src_off + S * pitch + 16, 7.0, x.dtype)
    for s in range(S):
        hb[16 + src_off + s * pitch:][:n * nch] = x[s].ravel()
    src = torch.from_numpy(hb).cuda()
    dst = torch.full((64 + (dst_off + S * pitch) * nb + 64,), GUARD, dtype=torch.uint8, device="cuda") if fmt is not None else None
    g = None if gain is None else torch.from_numpy(np.ascontiguousarray(gain, dtype=np.float64)).cuda()
    pk = torch.from_numpy((np.zeros((S, nch), np.uint64) if peak is None else peak).view(np.int64)).cuda()
    cl = torch.from_numpy((np.zeros((S, nch), np.uint64) if clipped is None else clipped).view(np.int64)).cuda()
    vp = C.c_void_p
    rc = F.lib().RRX_finish_device(-1, vp(getattr(stream, "cuda_stream", 0) or 0), F.RRX_FMT_DOUBLE if x.dtype == np.float64 else F.RRX_FMT_FLOAT,
                                   vp(src.data_ptr() + (16 + src_off) * x.itemsize), n + pad, fmt or 0,
                                   vp(dst.data_ptr() + 64 + dst_off * nb) if dst is not None else None, n + pad, S, n, nch,
                                   vp(g.data_ptr()) if g is not None else None, int(dith), seed, first_frame, vp(pk.data_ptr()), vp(cl.data_ptr()))
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
    return out, pk.cpu().numpy().view(np.uint64), cl.cpu().numpy().view(np.uint64)
