"""What the tests of the launch and chunk seams share (tests/test_stream_seams_api.py on the host, tests/test_gpu_stream_seams.py
on the device): inputs of 32768 + 3 streams or tracks whose two sides of the 32768 seam differ in everything a kernel takes per
stream, the references -- the numpy models over all streams, and where a model loops over streams or groups in Python a
vectorised restatement of it that the host module holds to the model at a small size -- and one caller that hands the same
argument list to a host twin (RRX_debug_*_host) or to the device call (RRX_*_device), every output starting as a guard pattern
with a few entries more than the call owns."""
import contextlib
import functools

import numpy as np

import foo_dsp_resampler_amd as F
import finish_model as FM
import loudness_model as LM
import loudness_stats_model as S
import shaped_model as SM
import true_peak_model as TM

SLICE = 32768                     # streams or tracks per launch: grid.y is a 16-bit count
N = SLICE + 3
GRID_X = 1 << 22                  # loudness_stats.hip, kMaxGridX
SEED = 0x1234567887654321
MIX = 0xBF58476D1CE4E5B9
GUARD = 777.25                    # doubles
NGUARD = 12345                    # counts
BGUARD = 0xA5                     # bytes
TAIL = 3                          # entries behind what a call owns, in every output
ORDER = SM.ORDER


def subset(n=N):
    """the streams around the seam and about 50 more, with a fixed seed"""
    near = [0, 1, SLICE - 2, SLICE - 1, SLICE, SLICE + 1, n - 1]
    return sorted(set(near) | set(int(v) for v in np.random.default_rng(50).integers(0, n, 50)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """equal bit patterns, or NaN in both (test_gpu_loudness_stats.same)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def two_sides_differ(*arrays):
    """every array [N, ...] differs between stream s and stream s - 32768, for every s behind the seam"""
    return all(bool((np.asarray(a[SLICE:]).reshape(len(a) - SLICE, -1) != np.asarray(a[:len(a) - SLICE]).reshape(len(a) - SLICE, -1)).any(axis=1).all())
               for a in arrays)


def live_on_both_sides(a):
    """something non-zero on either side of the seam"""
    a = np.asarray(a).reshape(len(a), -1)
    return bool(a[:SLICE].any() and a[SLICE:].any())


# ------------------------------------------------------------------------------------------------------------------ the caller

class Out:
    """an output of a call: a numpy array that starts as a guard pattern and receives what the call wrote; `skip` bytes in front
    of the pointer handed over"""

    def __init__(self, a, skip=0):
        self.a, self.skip = a, skip


class Host:
    """an argument that is a host pointer in the device call too (filter coefficients)"""

    def __init__(self, a):
        self.a = np.ascontiguousarray(a, dtype=np.float64)


_gated_run = None


@contextlib.contextmanager
def gated_by(run):
    """while this is entered, the device calls of call() are made by run(enqueue, inputs, outputs, entry point) -- enqueue(stream)
    queues the call on a torch stream, inputs and outputs are its device tensors -- instead of on the null stream between two
    synchronisations (tests/test_gpu_stream_order.py: the gated driver of tests/stream_gate.py).  What the callers assert of the
    outputs stays as it is."""
    global _gated_run
    assert _gated_run is None
    _gated_run = run
    try:
        yield
    finally:
        _gated_run = None


def call(name, args, on_device):
    """RRX_<name>_device(-1, NULL, *args) or RRX_debug_<name>_host(*args): numpy arrays go as pointers (on the device: to copies
    there, which must come back unchanged), Out arrays are filled with what the call left, None is NULL"""
    L = F.lib()
    if not on_device:
        ptrs = []
        for v in args:
            if isinstance(v, Out):
                ptrs.append(v.a.ctypes.data + v.skip)
            elif isinstance(v, Host):
                ptrs.append(v.a.ctypes.data)
            elif isinstance(v, np.ndarray):
                assert v.flags.c_contiguous
                ptrs.append(v.ctypes.data)
            else:
                ptrs.append(v)
        rc = getattr(L, "RRX_debug_%s_host" % name)(*ptrs)
        assert rc == 0, (name, rc)
        return
    import torch

    def up(a):
        assert a.flags.c_contiguous
        return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()

    F.ratelib._ensure_init()
    ptrs, outs, ins = [], [], []
    for v in args:
        if isinstance(v, Out):
            t = up(v.a)
            outs.append((v, t))
            ptrs.append(t.data_ptr() + v.skip)
        elif isinstance(v, Host):
            ptrs.append(v.a.ctypes.data)
        elif isinstance(v, np.ndarray):
            t = up(v)
            ins.append((v, t))
            ptrs.append(t.data_ptr())
        else:
            ptrs.append(v)
    torch.cuda.synchronize()
    if _gated_run is not None:
        def enqueue(stream):
            rc = getattr(L, "RRX_%s_device" % name)(-1, stream.cuda_stream, *ptrs)
            assert rc == 0, (name, rc)

        _gated_run(enqueue, [t for _, t in ins], [t for _, t in outs], "RRX_%s_device" % name)
    else:
        rc = getattr(L, "RRX_%s_device" % name)(-1, None, *ptrs)
        assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    for v, t in outs:
        got = t.cpu().numpy()
        v.a[...] = got.view(np.uint64) if v.a.dtype == np.uint64 else got
    for v, t in ins:
        assert np.array_equal(t.cpu().numpy().view(np.uint8).reshape(-1), v.view(np.uint8).reshape(-1)), (name, "an input was written")


def guarded(n, dtype, guard):
    return np.full(n + TAIL, guard, dtype)


def owned(a, n, guard):
    """the first n entries of a guarded output; the tail must still hold the guard"""
    assert (a[n:] == guard).all(), "entries behind the output were written"
    return a[:n]


def src_format(x):
    return F.RRX_FMT_DOUBLE if x.dtype == np.float64 else F.RRX_FMT_FLOAT


def stream_seed(s, nch, seed=SEED):
    """the seed under which stream 0 of a one-stream call gets the dither of stream s"""
    return (seed + s * nch * MIX) % 2 ** 64


def gains(n=N):
    """from 0.5 to 2: distinct for every stream, and above 1 behind the seam"""
    return 0.5 + 1.5 * np.arange(n) / n


def planted_noise(key, shape, nbits, dtype, frac=0.25):
    """seeded noise on +-0.6 with finish_model's edge values of the format (ties, +-1, +-3, +-inf, denormals; no NaN) in a
    quarter of the samples, and full-scale samples in the first sample of two streams on either side of the seam"""
    rng = np.random.default_rng(key)
    x = rng.uniform(-0.6, 0.6, shape)
    p = FM.planted(nbits)[1:]
    put = rng.uniform(size=shape) < frac
    x[put] = p[rng.integers(0, len(p), int(put.sum()))]
    first = x.reshape(shape[0], -1)[:, 0]
    first[[0, 1, SLICE, SLICE + 1]] = [1.0, -3.0, -1.0, 3.0]
    with np.errstate(over="ignore"):
        return x.astype(dtype)


# ------------------------------------------------------------------------------------------------ RRX_finish_device (finish.hip)

# fmt (None: measure only), float64 source, nch, frames, dither.  257 channels: lcm(4, 257) = 1028 is above kSpanMax = 1024 of
# finish.hip, which selects the kernel with its channel table in LDS
FINISH = {"f32-s16": (F.RRX_FMT_S16, False, 2, 5, True), "f64-s24": (F.RRX_FMT_S24_3, True, 3, 5, False),
          "measure": (None, False, 1, 1, True), "lds-table": (F.RRX_FMT_S16, False, 257, 2, True)}
FIRST_FRAME = 1000003
PEAK0, CLIPPED0 = 3, 1000        # what the accumulating statistics start from: a denormal's pattern, and a count


@functools.lru_cache(maxsize=None)
def finish_input(key):
    fmt, double, nch, frames, dith = FINISH[key]
    return planted_noise([1, nch, frames], (N, frames, nch), FM.BITS[fmt] if fmt is not None else 31, np.float64 if double else np.float32)


def finish_model(key, streams=None):
    """(bytes or None, peak bits, clipped) of finish_model.model: over all streams at once, or stream by stream over `streams`"""
    fmt, double, nch, frames, dith = FINISH[key]
    x, g = finish_input(key), gains()
    pk0, cl0 = np.full((N, nch), PEAK0, np.uint64), np.full((N, nch), CLIPPED0, np.uint64)
    if streams is None:
        return FM.model(x, fmt, g, dith, SEED, FIRST_FRAME, pk0, cl0)
    parts = [FM.model(x[s:s + 1], fmt, g[s:s + 1], dith, stream_seed(s, nch), FIRST_FRAME, pk0[:1], cl0[:1]) for s in streams]
    return tuple(None if parts[0][i] is None else np.concatenate([p[i] for p in parts]) for i in range(3))


def finish_call(key, on_device):
    """the call on rows one frame apart beyond their length, the destination 65 bytes into its buffer: (bytes [N, frames, nch *
    size] or None, peak bits [N, nch], clipped [N, nch]); everything outside them must hold its guard"""
    fmt, double, nch, frames, dith = FINISH[key]
    x = finish_input(key)
    stride = frames + 1
    src = np.full((N, stride, nch), 7.0, x.dtype)
    src[:, :frames] = x
    nb = FM.NBYTES[fmt] if fmt is not None else 0
    dst = np.full(65 + N * stride * nch * nb + 64, BGUARD, np.uint8)
    pk, cl = guarded(N * nch, np.uint64, PEAK0), guarded(N * nch, np.uint64, CLIPPED0)
    call("finish", [src_format(x), src, stride, fmt or 0, Out(dst, 65) if fmt is not None else None, stride, N, frames, nch, gains(), int(dith), SEED,
                    FIRST_FRAME, Out(pk), Out(cl)], on_device)
    out = None
    if fmt is not None:
        rows = dst[65:65 + N * stride * nch * nb].reshape(N, stride * nch * nb)
        out = rows[:, :frames * nch * nb].reshape(N, frames, nch * nb).copy()
        rows[:, :frames * nch * nb] = BGUARD
        assert (dst == BGUARD).all(), "bytes outside the destination rows were written"
    return out, owned(pk, N * nch, PEAK0).reshape(N, nch), owned(cl, N * nch, CLIPPED0).reshape(N, nch)


# ---------------------------------------------------------------------------------- RRX_finish_shaped_device (finish_shaped.hip)

# order, fmt, float64 source.  9 frames from absolute frame 2 in segments of 4: a first segment that begins inside (the incoming
# state is read), a whole one, and a last partial one
SHAPED = {"order9": (9, F.RRX_FMT_S16, False), "order4": (4, F.RRX_FMT_S24_3, True)}
SHAPED_NCH, SHAPED_FRAMES, SHAPED_FIRST, SEGMENT = 2, 9, 2, 4


@functools.lru_cache(maxsize=None)
def shaped_input(key):
    order, fmt, double = SHAPED[key]
    x = planted_noise([2, order], (N, SHAPED_FRAMES, SHAPED_NCH), FM.BITS[fmt], np.float64 if double else np.float32)
    return x, SM.random_state(N, SHAPED_NCH, order)


def shaped_model(key, streams=None):
    """(bytes, peak bits, clipped, state out) of shaped_model.model"""
    order, fmt, double = SHAPED[key]
    (x, st), g, nch = shaped_input(key), gains(), SHAPED_NCH
    pk0, cl0 = np.full((N, nch), PEAK0, np.uint64), np.full((N, nch), CLIPPED0, np.uint64)
    if streams is None:
        return SM.model(x, fmt, SM.coefs_of(order), SEGMENT, g, True, SEED, SHAPED_FIRST, st, pk0, cl0)
    parts = [SM.model(x[s:s + 1], fmt, SM.coefs_of(order), SEGMENT, g[s:s + 1], True, stream_seed(s, nch), SHAPED_FIRST, st[s:s + 1], pk0[:1], cl0[:1])
             for s in streams]
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(4))


def shaped_call(key, on_device):
    order, fmt, double = SHAPED[key]
    x, st = shaped_input(key)
    nch, frames, stride, nb = SHAPED_NCH, SHAPED_FRAMES, SHAPED_FRAMES + 1, FM.NBYTES[fmt]
    src = np.full((N, stride, nch), 7.0, x.dtype)
    src[:, :frames] = x
    dst = np.full(65 + N * stride * nch * nb + 64, BGUARD, np.uint8)
    pk, cl = guarded(N * nch, np.uint64, PEAK0), guarded(N * nch, np.uint64, CLIPPED0)
    so = guarded(N * nch * ORDER, np.float64, GUARD)
    call("finish_shaped", [src_format(x), src, stride, fmt, Out(dst, 65), stride, N, frames, nch, gains(), 1, SEED, SHAPED_FIRST,
                           Host(SM.coefs_of(order)), order, SEGMENT, st, Out(so), Out(pk), Out(cl)], on_device)
    rows = dst[65:65 + N * stride * nch * nb].reshape(N, stride * nch * nb)
    out = rows[:, :frames * nch * nb].reshape(N, frames, nch * nb).copy()
    rows[:, :frames * nch * nb] = BGUARD
    assert (dst == BGUARD).all(), "bytes outside the destination rows were written"
    return (out, owned(pk, N * nch, PEAK0).reshape(N, nch), owned(cl, N * nch, CLIPPED0).reshape(N, nch),
            owned(so, N * nch * ORDER, GUARD).reshape(N, nch, ORDER))


# ------------------------------------------------------------------------------------------ RRX_true_peak_device (true_peak.hip)

# phases, taps, float64 source, nch, frames, flush, with states.  nch * taps above 4096 doubles leaves the LDS form
# (true_peak_lds_form): 257 channels under 16 taps are the smallest such shape.  Its state would be 16 doubles for each of
# 32771 * 257 channels, a gigabyte each way, so the direct kernel runs from absolute frame 0 and hands no state on
TRUE_PEAK = {"bs1770": (4, 12, False, 2, 20, True, True), "generic-3x5": (3, 5, True, 2, 6, True, True),
             "direct": (2, 16, False, 257, 1, False, False)}
TP_FIRST = 7


def tp_coefs(key):
    phases, taps = TRUE_PEAK[key][:2]
    return TM.BS1770 if key == "bs1770" else np.random.default_rng([3, phases, taps]).standard_normal((phases, taps))


@functools.lru_cache(maxsize=None)
def tp_input(key):
    phases, taps, double, nch, frames, flush, states = TRUE_PEAK[key]
    rng = np.random.default_rng([4, phases, taps])
    x = (rng.standard_normal((N, frames, nch)) * 0.5).astype(np.float64 if double else np.float32)
    st = None
    if states:
        st = np.zeros((N, nch, TM.MAX_TAPS))
        st[:, :, :taps - 1] = rng.standard_normal((N, nch, taps - 1)) * 0.5
    return x, st


def tp_model(key, streams=None):
    """(true peak bits, peak bits, state out) of true_peak_model.true_peak, in slices of 4096 streams: its history array is
    taps - 1 frames for every channel"""
    phases, taps, double, nch, frames, flush, states = TRUE_PEAK[key]
    (x, st), g = tp_input(key), gains()
    groups = [slice(a, min(a + 4096, N)) for a in range(0, N, 4096)] if streams is None else [slice(s, s + 1) for s in streams]
    parts = [TM.true_peak(x[i], tp_coefs(key), g[i], flush, None if st is None else st[i]) for i in groups]
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))


def tp_call(key, on_device):
    phases, taps, double, nch, frames, flush, states = TRUE_PEAK[key]
    x, st = tp_input(key)
    stride = frames + 1
    src = np.full((N, stride, nch), 7.0, x.dtype)
    src[:, :frames] = x
    tp, pk = guarded(N * nch, np.uint64, PEAK0), guarded(N * nch, np.uint64, PEAK0)
    so = guarded(N * nch * TM.MAX_TAPS, np.float64, GUARD) if states else None
    call("true_peak", [src_format(x), src, stride, N, frames, nch, gains(), TP_FIRST if states else 0, Host(tp_coefs(key)), phases, taps, int(flush), st,
                       Out(so) if states else None, Out(tp), Out(pk)], on_device)
    return (owned(tp, N * nch, PEAK0).reshape(N, nch), owned(pk, N * nch, PEAK0).reshape(N, nch),
            owned(so, N * nch * TM.MAX_TAPS, GUARD).reshape(N, nch, TM.MAX_TAPS) if states else None)


# -------------------------------------------------------------------------------------------- RRX_loudness_device (loudness.hip)

HOP, L_FRAMES, L_NCH, L_FIRST = 3, 10, 2, 3     # 3 whole hops and a remainder, from the second hop of the stream on
L_HOPS, L_STRIDE = L_FRAMES // HOP, L_FIRST // HOP + L_FRAMES // HOP + 2


@functools.lru_cache(maxsize=None)
def loudness_input(double):
    rng = np.random.default_rng([5, int(double)])
    x = (rng.standard_normal((N, L_FRAMES, L_NCH)) * 0.3).astype(np.float64 if double else np.float32)
    return x, rng.standard_normal((N, L_NCH, 4)) * 0.1


def loudness_model(double):
    """(energy [N, nch, hops], state out [N, nch, 4]) of loudness_model.hop_energies, which is vectorised over streams"""
    x, st = loudness_input(double)
    return LM.hop_energies(LM.gained(x, gains()), LM.K48, HOP, st)


def loudness_call(double, on_device):
    """(the energy buffer [N, nch, stride] with the guard where nothing was written, state out, work)"""
    x, st = loudness_input(double)
    stride = L_FRAMES + 1
    src = np.full((N, stride, L_NCH), 7.0, x.dtype)
    src[:, :L_FRAMES] = x
    need = F.lib().RRX_loudness_work_doubles(N, L_NCH, L_FRAMES, HOP)
    assert need == N * L_NCH * L_HOPS * 4
    e, so, work = guarded(N * L_NCH * L_STRIDE, np.float64, GUARD), guarded(N * L_NCH * 4, np.float64, GUARD), guarded(need, np.float64, GUARD)
    call("loudness", [src_format(x), src, stride, N, L_FRAMES, L_NCH, gains(), L_FIRST, Host(LM.K48), HOP, st, Out(so), Out(e), L_STRIDE, Out(work), need],
         on_device)
    owned(work, need, GUARD)
    return owned(e, N * L_NCH * L_STRIDE, GUARD).reshape(N, L_NCH, L_STRIDE), owned(so, N * L_NCH * 4, GUARD).reshape(N, L_NCH, 4)


# ------------------------------------------------------------- RRX_loudness_gate_device, RRX_loudness_blocks_device (the meter)

NHOPS = 8
WEIGHTS = np.array([1.0, 1.41])
BLOCK_SHAPES = [(4, 1), (3, 2)]


@functools.lru_cache(maxsize=None)
def hop_energies():
    """(energy [N, 2, 8], hops [N] cycling through 0..8): every hop is loud, 20 dB down or under the absolute gate, so that both
    gates remove blocks of many streams.  The three streams behind the seam have 3, 4 and 5 hops -- none, one and two (4, 1)
    blocks -- and the last one a loud block and one the relative gate removes"""
    rng = np.random.default_rng(6)
    e = rng.uniform(1.0, 50.0, (N, 2, NHOPS)) * rng.choice([1.0, 0.01, 1e-12], size=(N, 1, NHOPS), p=[0.5, 0.3, 0.2])
    e[N - 1, :, 0], e[N - 1, :, 1:5] = 40.0, 0.2
    return e, ((np.arange(N) + 4) % 9).astype(np.uint64)


def block_hops():
    """the hops of the blocks cases: 2, 3 and 4 behind the seam, so that streams without a block and streams with one lie on both
    sides of it under both block shapes"""
    return ((np.arange(N) + 3) % 9).astype(np.uint64)


def gate_call(on_device):
    e, hops = hop_energies()
    res = guarded(N * 4, np.float64, GUARD)
    call("loudness_gate", [e, NHOPS, N, 2, NHOPS, hops, WEIGHTS, HOP, *LM.gate_thresholds(), Out(res)], on_device)
    return owned(res, N * 4, GUARD).reshape(N, 4)


@functools.lru_cache(maxsize=None)
def gate_model():
    e, hops = hop_energies()
    return LM.gate(e, HOP, hops, WEIGHTS)


def blocks_call(L, P, on_device, blocks=True):
    """(blocks [N, stride] with the guard where nothing was written, or None; nblocks; max)"""
    e, hops = hop_energies()[0], block_hops()
    stride = S.count(NHOPS, L, P)
    b, nb, mx = guarded(N * stride, np.float64, GUARD), guarded(N, np.uint64, NGUARD), guarded(N, np.float64, GUARD)
    call("loudness_blocks", [e, NHOPS, N, 2, NHOPS, hops, WEIGHTS, HOP, L, P, Out(b) if blocks else None, stride if blocks else 0, Out(nb), Out(mx)],
         on_device)
    return owned(b, N * stride, GUARD).reshape(N, stride) if blocks else None, owned(nb, N, NGUARD), owned(mx, N, GUARD)


def blocks_model(L, P):
    e, hops = hop_energies()[0], block_hops()
    zs, nbs, top = S.blocks(e, HOP, L, P, hops=hops, weights=WEIGHTS)
    return S.as_rows(zs, S.count(NHOPS, L, P), GUARD), nbs, top


# ------------------------------------------------------------------------------------------------- the per-track forms (tracks.hip)

ROW = 8                           # frames of a row
T_NCH = 2
T_MAX = 5                         # the longest slice
WINDOWS = [(0, 3), (3, 5)]        # two windows that partition the rows


@functools.lru_cache(maxsize=None)
def track_table():
    """(table uint64 [N, 6], dst_total): out_first cycles through 0..3 with period 5, out_frames through 0..5 with period 11,
    dst_first is the running sum"""
    t = np.arange(N)
    of, cnt = (t % 5) % 4, (t % 11) % 6
    tab = np.zeros((N, 6), np.uint64)
    tab[:, 3], tab[:, 4] = of, cnt
    tab[:, 5] = np.cumsum(cnt) - cnt
    return tab, int(cnt.sum())


@functools.lru_cache(maxsize=None)
def track_rows(double):
    """rows [N, 8, 2] of planted noise, with a huge value in the frame on either side of each track's slice"""
    x = planted_noise([7, int(double)], (N, ROW, T_NCH), 15, np.float64 if double else np.float32)
    tab, _ = track_table()
    of, cnt = tab[:, 3].astype(np.int64), tab[:, 4].astype(np.int64)
    t = np.arange(N)
    x[t[of > 0], of[of > 0] - 1] = 1e30
    x[t[of + cnt < ROW], (of + cnt)[of + cnt < ROW]] = -1e30
    return x


def track_slices(double):
    """(slices [N, 5, 2]: every track's own frames from frame 0 on, +0.0 behind them; valid [N, 5]).  A frame of +0.0 behind a
    track leaves its peak, its clip count, the frames before it and the filter tails behind it as they are, so a model of the
    uniform call on these equal-length slices is the one-stream call on each track's slice"""
    x = track_rows(double)
    tab, _ = track_table()
    of, cnt = tab[:, 3].astype(np.int64), tab[:, 4].astype(np.int64)
    i = np.arange(T_MAX)
    valid = i[None, :] < cnt[:, None]
    sl = x[np.arange(N)[:, None], np.minimum(of[:, None] + i[None, :], ROW - 1)]
    sl[~valid] = 0.0
    return sl, valid


def packed_bytes(out, valid):
    """the frames of every track, in track order: the packed destination (dst_first is the running sum)"""
    return np.ascontiguousarray(out[valid]).reshape(-1)


def tracks_finish_model(double, fmt):
    sl, valid = track_slices(double)
    out, pk, cl = FM.model(sl, fmt, gains(), True, SEED, 0, np.full((N, T_NCH), PEAK0, np.uint64), np.full((N, T_NCH), CLIPPED0, np.uint64))
    return packed_bytes(out, valid), pk, cl


def tracks_shaped_model(double, fmt, order, streams=None):
    """(packed bytes, peak bits, clipped) over all tracks; over `streams`, one track at a time on its own slice, also the state
    behind its last frame: (bytes per track, peak bits, clipped, state)"""
    sl, valid = track_slices(double)
    coefs, g = SM.coefs_of(order), gains()
    assert 1.0 + 1.5 * np.abs(coefs).sum() < 2.0 ** FM.BITS[fmt]  # a frame of +0.0 cannot clip under any error history
    pk0, cl0 = np.full((N, T_NCH), PEAK0, np.uint64), np.full((N, T_NCH), CLIPPED0, np.uint64)
    if streams is None:
        out, pk, cl, _ = SM.model(sl, fmt, coefs, SEGMENT, g, True, SEED, 0, None, pk0, cl0)
        return packed_bytes(out, valid), pk, cl
    parts = []
    for t in streams:
        n = int(valid[t].sum())
        if not n:                                    # an empty track: no bytes, statistics untouched, a state of zeros
            parts.append((np.zeros(0, np.uint8), pk0[:1], cl0[:1], np.zeros((1, T_NCH, ORDER))))
            continue
        parts.append(SM.model(sl[t:t + 1, :n], fmt, coefs, SEGMENT, g[t:t + 1], True, stream_seed(t, T_NCH), 0, None, pk0[:1], cl0[:1]))
    return [p[0].reshape(-1) for p in parts], np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]), np.concatenate([p[3] for p in parts])


def window_of(x, wf, wn):
    """frames [wf, wf + wn) of every row as a window buffer of one frame more a row, which holds a huge value"""
    win = np.full((x.shape[0], wn + 1, x.shape[2]), 1e30, x.dtype)
    win[:, :wn] = x[:, wf:wf + wn]
    return win


def tracks_finish_call(double, fmt, form, order=9, on_device=True):
    """form "rows" / "windows" of the plain call or "shaped" / "shaped-windows" of the shaped one: (packed bytes, peak bits,
    clipped, state after the last window or None); the destination lies 65 bytes into a guarded buffer"""
    x = track_rows(double)
    tab, total = track_table()
    nb = FM.NBYTES[fmt]
    dst = np.full(65 + total * T_NCH * nb + 64, BGUARD, np.uint8)
    pk, cl = guarded(N * T_NCH, np.uint64, PEAK0), guarded(N * T_NCH, np.uint64, CLIPPED0)
    head = [tab, N, T_NCH, src_format(x)]
    tail = [fmt, Out(dst, 65), total, gains(), 1, SEED]
    shape = [Host(SM.coefs_of(order)), order, SEGMENT]
    state = None
    if form == "rows":
        call("tracks_finish", head + [x, ROW] + tail + [Out(pk), Out(cl)], on_device)
    elif form == "shaped":
        call("tracks_finish_shaped", head + [x, ROW] + tail + shape + [Out(pk), Out(cl)], on_device)
    else:
        states = [guarded(N * T_NCH * ORDER, np.float64, GUARD) for _ in range(2)]
        for wf, wn in WINDOWS:
            win = [window_of(x, wf, wn), wn + 1, ROW, wf, wn]
            if form == "windows":
                call("tracks_finish_window", head + win + tail + [Out(pk), Out(cl)], on_device)
            else:
                states[1][:] = GUARD
                call("tracks_finish_shaped_window", head + win + tail + shape + [None if wf == 0 else states[0][:N * T_NCH * ORDER].copy(), Out(states[1]),
                                                                               Out(pk), Out(cl)], on_device)
                states.reverse()
        if form != "windows":
            state = owned(states[0], N * T_NCH * ORDER, GUARD).reshape(N, T_NCH, ORDER)
    assert (dst[:65] == BGUARD).all() and (dst[65 + total * T_NCH * nb:] == BGUARD).all(), "bytes around the destination were written"
    return dst[65:65 + total * T_NCH * nb], owned(pk, N * T_NCH, PEAK0).reshape(N, T_NCH), owned(cl, N * T_NCH, CLIPPED0).reshape(N, T_NCH), state


def tracks_true_peak_model(double):
    sl, _ = track_slices(double)
    tp, pk, _ = tp_model_of(sl, TM.BS1770, gains())
    return tp, pk


def tp_model_of(x, coefs, g):
    parts = [TM.true_peak(x[a:a + 4096], coefs, g[a:a + 4096], True, None) for a in range(0, len(x), 4096)]
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))


def tracks_true_peak_call(double):
    x = track_rows(double)
    tab, _ = track_table()
    tp, pk = guarded(N * T_NCH, np.uint64, PEAK0), guarded(N * T_NCH, np.uint64, PEAK0)
    call("tracks_true_peak", [tab, N, T_NCH, src_format(x), x, ROW, gains(), Host(TM.BS1770), 4, 12, Out(tp), Out(pk)], True)
    return owned(tp, N * T_NCH, PEAK0).reshape(N, T_NCH), owned(pk, N * T_NCH, PEAK0).reshape(N, T_NCH)


T_HOP = 2                         # slices of 0..5 frames: 0, 1 or 2 hops a track
T_ESTRIDE = 4


def tracks_loudness_model(double):
    """(energy [N, 2, 2] of the slices taken as 2 hops each, hops [N]): hop k of a track depends on its frames below 2 k + 2 alone"""
    sl, valid = track_slices(double)
    with np.errstate(invalid="ignore"):             # an infinite sample poisons its channel: NaN energies
        e, _ = LM.hop_energies(LM.gained(sl, gains()), LM.K48, T_HOP)
    return e, (valid.sum(axis=1) // T_HOP).astype(np.uint64)


def tracks_loudness_call(double):
    """(the energy buffer [N, 2, 4] with the guard where nothing was written, hops)"""
    x = track_rows(double)
    tab, _ = track_table()
    need = F.lib().RRX_loudness_work_doubles(N, T_NCH, ROW, T_HOP)
    e, hops, work = guarded(N * T_NCH * T_ESTRIDE, np.float64, GUARD), guarded(N, np.uint64, NGUARD), guarded(need, np.float64, GUARD)
    call("tracks_loudness", [tab, N, T_NCH, src_format(x), x, ROW, gains(), Host(LM.K48), T_HOP, Out(e), T_ESTRIDE, Out(hops), Out(work), need], True)
    owned(work, need, GUARD)
    return owned(e, N * T_NCH * T_ESTRIDE, GUARD).reshape(N, T_NCH, T_ESTRIDE), owned(hops, N, NGUARD)


# ----------------------------------------------------------------------------------- the group kernels (loudness_stats.hip)

def groups_call(rows, nblocks, group, ngroups, abs_threshold, rel_factor, percentiles=None, on_device=True):
    """the gate (percentiles None) or the range call on blocks [nstreams, stride]: [ngroups, 4]; result and work under guards"""
    ns, stride = rows.shape
    need = F.lib().RRX_loudness_groups_work_doubles(ns, ngroups)
    res, work = guarded(ngroups * 4, np.float64, GUARD), guarded(need, np.float64, GUARD)
    args = [np.ascontiguousarray(rows, dtype=np.float64), stride, ns, np.ascontiguousarray(nblocks, dtype=np.uint64), np.ascontiguousarray(group, dtype=np.int32),
            ngroups, abs_threshold, rel_factor]
    if percentiles is None:
        call("loudness_gate_groups", args + [Out(res), Out(work), need], on_device)
    else:
        call("loudness_range_groups", args + [int(percentiles[0]), int(percentiles[1]), Out(res), Out(work), need], on_device)
    owned(work, need, GUARD)
    return owned(res, ngroups * 4, GUARD).reshape(ngroups, 4)


def rows_of(values, fill=GUARD):
    """a list of one array of blocks per stream as (rows [nstreams, stride], nblocks)"""
    return S.as_rows(values, max(max(len(v) for v in values), 1) + 1, fill), np.array([len(v) for v in values], np.uint64)


@functools.lru_cache(maxsize=None)
def gate_groups_case(ns):
    """ns streams of 0..70 blocks (both sides of a wave's 64) as test_gpu_loudness_stats.energies makes them, a NaN block in one
    member, and five groups over chunks of 64 streams: 0 interleaved over every chunk, 1 with all its members in the last, partial
    chunk, 2 with members in the first and the last chunk and none between, 3 empty; some streams in no group (-1 and ngroups).
    (blocks per stream, group, ngroups)"""
    rng = np.random.default_rng([8, ns])
    nb = rng.integers(0, 71, ns)
    nb[:4] = [64, 0, 65, 63]
    zs = []
    for s in range(ns):
        z = rng.uniform(1.0, 50.0, int(nb[s])) * rng.choice([1.0, 0.01, 1e-12], size=int(nb[s]), p=[0.5, 0.3, 0.2])
        zs.append(z)
    zs[2][5] = np.nan
    last = (ns - 1) // 64 * 64                      # first stream of the last chunk
    group = np.where(np.arange(ns) % 3 == 0, 0, np.where(np.arange(ns) % 3 == 1, 4, -1)).astype(np.int32)
    group[np.arange(ns) % 7 == 5] = 5                # == ngroups: in no group
    if last:
        group[last:] = np.where(np.arange(ns - last) % 2 == 0, 1, 0)
    else:
        group[ns - 3:] = 1                           # one chunk in all
    group[[2, 5, 7]] = 2
    if ns - 1 > last > 0:
        group[ns - 1] = 2                            # (with chunks between, at 300 streams)
    return zs, group, 5


@functools.lru_cache(maxsize=None)
def scattered_groups_case(ns, ngroups=300):
    """ns streams scattered over 300 groups, two or three streams each where ns allows it"""
    rng = np.random.default_rng([9, ns])
    zs, _, _ = gate_groups_case(ns)
    return zs, rng.permutation(np.arange(ns) % ngroups).astype(np.int32), ngroups


PCTS = [(10, 95), (0, 100), (50, 50), (95, 10)]
RANGE_GATE = (0.5, 0.1)           # every block of the range cases is above 0.5 but those of the gated case


@functools.lru_cache(maxsize=None)
def range_case(ns):
    """ns streams over chunks of 256 and 4 groups.  Group 0 has members in chunks 0 and 2 and none in chunk 1; among them runs of
    zero-block members that include the first and the last member of a chunk.  Group 1 pools one stream of 3000 blocks among
    one-block streams in chunk 0, so that the cursor jumps many members in one step, and fewer than 256 blocks in its later
    chunks.  Group 2 is chunk 1.  Group 3 takes what is left; some streams are in no group."""
    rng = np.random.default_rng([10, ns])
    nb = rng.integers(0, 6, ns)
    group = np.full(ns, 3, np.int32)
    group[0:256:2] = 0
    group[1:256:2] = 1
    group[256:min(512, ns)] = 2
    if ns > 512:
        group[512:ns:2] = 0
        group[513:ns:2] = 1
    group[np.arange(ns) % 11 == 9] = -1
    nb[group == 1] = 1
    nb[np.flatnonzero(group == 1)[::5]] = 0
    nb[101] = 3000
    group[101] = 1
    for a, b in ((0, 8), (120, 140), (250, 256), (512, 520), (ns - 6, ns)):   # zero-block runs at the edges of chunks and inside
        nb[a:b] = 0
    scale = np.where(rng.uniform(size=ns) < 0.8, 1.0, 1e-3)          # a fifth of the streams lies under the absolute gate
    scale[101] = 1.0
    zs = [rng.uniform(1.0, 2.0, int(n)) * scale[s] for s, n in enumerate(nb)]
    return zs, group, 4


def hard_multisets():
    """the multisets of test_gpu_loudness_stats.test_range_select_on_hard_multisets: 90 % duplicates, differences in the lowest
    byte only, 300 binary orders of magnitude (with the gate each needs)"""
    rng = np.random.default_rng(1)
    dup = np.where(rng.uniform(size=3000) < 0.9, 1.5, rng.uniform(1.0, 2.0, 3000))
    low8 = (np.uint64(0x3FF8000000000000) + rng.integers(0, 256, 2000).astype(np.uint64)).view(np.float64)
    spread = 2.0 ** rng.uniform(-150.0, 150.0, 2000)
    return {"duplicates": (dup, 0.5, 0.1), "lowest byte": (low8, 0.5, 0.1), "spread": (spread, 0.0, 0.0)}


def over_three_chunks(values, ns=700):
    """`values` dealt out in pieces of 0..12 blocks to the even streams of three chunks of 256; the odd ones are another group"""
    rng = np.random.default_rng(len(values))
    zs, pos = [], 0
    for s in range(ns):
        if s % 2:
            zs.append(np.full(int(rng.integers(0, 3)), 1e30))
            continue
        left = (ns - s + 1) // 2                     # even streams still to come, this one included
        n = len(values) - pos if left == 1 else min(int(rng.integers(0, 13)), len(values) - pos)
        zs.append(values[pos:pos + n])
        pos += n
    assert pos == len(values)
    return zs, (np.arange(ns) % 2).astype(np.int32), 2


# ------------------------------------------------------------------------------------------------------------ the 2^22 seams

NS_BIG = GRID_X + 3
NG_BIG = GRID_X + 1


@functools.lru_cache(maxsize=None)
def big_streams_case():
    """2^22 + 3 streams of at most one block, blocks_stride 1, group s % 67 of 64 groups: (rows [ns, 1], nblocks, group).  A third
    of the blocks fails the absolute gate and about a fifth the relative one"""
    rng = np.random.default_rng(11)
    z = rng.uniform(1.0, 50.0, NS_BIG) * rng.choice([1.0, 0.01, 1e-12], size=NS_BIG, p=[0.5, 0.3, 0.2])
    nb = (rng.uniform(size=NS_BIG) < 0.8).astype(np.uint64)
    nb[[0, GRID_X - 1, GRID_X, NS_BIG - 1]] = 1
    return z.reshape(NS_BIG, 1), nb, (np.arange(NS_BIG) % 67).astype(np.int32)


def gate_groups_one_block(rows, nblocks, group, ngroups, abs_threshold, rel_factor):
    """loudness_stats_model.gate_groups for streams of at most one block, vectorised over streams: a stream's own sum is its
    block or +0.0, and +0.0 + x is x, so a group's serial sum over its members ascending is np.cumsum over its passing blocks"""
    z, has = rows[:, 0], np.asarray(nblocks) > 0
    out = np.zeros((ngroups, 4))
    with np.errstate(invalid="ignore", divide="ignore"):
        for g in range(ngroups):
            zg = z[has & (group == g)]
            a = zg[zg > abs_threshold]
            s1, n1 = (np.cumsum(a)[-1] if a.size else np.float64(0.0)), np.float64(a.size)
            t = np.float64(rel_factor) * (s1 / n1)
            b = a[a > t]
            out[g] = (np.cumsum(b)[-1] if b.size else np.float64(0.0), b.size, s1, n1)
    return out


@functools.lru_cache(maxsize=None)
def big_groups_case():
    """3 streams in groups 0, 2^22 - 1 and 2^22 of 2^22 + 1: (blocks per stream, group)"""
    rng = np.random.default_rng(12)
    zs = [rng.uniform(1.0, 50.0, n) * rng.choice([1.0, 0.01, 1e-12], size=n, p=[0.5, 0.3, 0.2]) for n in (40, 70, 55)]
    return zs, np.array([0, GRID_X - 1, GRID_X], np.int32)


def big_groups_model(percentiles=None):
    """the model on the three populated groups taken as groups 0, 1, 2, spread over 2^22 + 1 rows; every other row is the empty
    group's: {+0.0, 0, +0.0, 0}, or {+0.0, +0.0, 0, T = NaN} of the range call"""
    zs, group = big_groups_case()
    if percentiles is None:
        small, empty = S.gate_groups(zs, [0, 1, 2], 3), [0.0, 0.0, 0.0, 0.0]
    else:
        small, empty = S.range_groups(zs, [0, 1, 2], 3, *S.gate_thresholds(-70.0, -20.0), low=percentiles[0], high=percentiles[1]), [0.0, 0.0, 0.0, np.nan]
    out = np.tile(np.array(empty), (NG_BIG, 1))
    out[group] = small
    return out
