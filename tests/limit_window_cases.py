"""What the host and the device tests of the limiter's window form share (RRX_tracks_limit_window_device): one ragged batch of rows
with noise outside the slices too, the window partitions, the minimal-coverage buffer of a window, and the expectation -- the
one-stream host call on every slice.  numpy only."""
import numpy as np

import foo_dsp_resampler_amd as F
import limit_model as M

ROW = 9000
LH = [(1, 0), (7, 3), (72, 480), (1024, 4096)]
REACH = [(11, 11), (20, 17), (562, 82), (5130, 1034)]  # (back, ahead) of LH at 12 taps
LENGTHS = (0, 1, 11, 300, 4097, ROW)
FIRSTS = (0, 5, 1023, 1024, 2000)
BS = np.ascontiguousarray(M.BS1770.reshape(-1))
GUARD = 777.25
CEILING = 0.5


def table_of(slices):
    """an RRX_track table (uint64 [ntracks, 6]) whose output slices are (out_first, out_frames); the other fields are not looked at"""
    t = np.zeros((len(slices), 6), np.uint64)
    for i, (first, frames) in enumerate(slices):
        t[i] = (3 * i, frames, 1, first, frames, 7 * i)
    return t


def batch(nch, dtype, seed=5):
    """(rows [ntracks, ROW, nch], table, gain [ntracks]): every length at every first frame; a slice that runs past the row is the
    call's to clamp.  Noise of sigma 0.5 everywhere, so that about a third of the frames is over the ceiling."""
    rng = np.random.default_rng(seed)
    slices = [(first, n) for n in LENGTHS for first in FIRSTS]
    rows = (rng.standard_normal((len(slices), ROW, nch)) * 0.5).astype(dtype)
    gain = 0.5 + rng.random(len(slices))
    return rows, table_of(slices), gain


def clamped(table, row_frames):
    out = []
    for e in table:
        of = min(int(e[3]), row_frames)
        out.append((of, min(int(e[4]), row_frames - of)))
    return out


def partitions(row_frames=ROW, seed=11):
    """{name: [(first, frames) ...]}, each covering [0, row_frames) with disjoint windows; every one also in descending order"""
    def cut(points):
        points = [0] + sorted(set(p for p in points if 0 < p < row_frames)) + [row_frames]
        return [(a, b - a) for a, b in zip(points[:-1], points[1:])]
    widths, at = [], 0
    for w in (1, 2, 11, 257, 1023, 1025, 3058):
        at += w
        widths.append(at)
    rng = np.random.default_rng(seed)
    out = {"one": cut([]), "k1024": cut(range(1024, row_frames, 1024)), "widths": cut(widths),
           "random": cut(int(v) for v in rng.integers(1, row_frames, 7))}
    for name in list(out):
        out[name + "-descending"] = out[name][::-1]
    return out


def coverage(first, frames, back, ahead, row_frames=ROW):
    """the smallest [buf_first, buf_first + buf_frames) the coverage rule allows for a window"""
    lo, hi = max(0, first - back), min(row_frames, first + frames + ahead)
    return lo, hi - lo


def expected(rows, table, gain, L, H, dst, coefs=M.BS1770, ceiling=CEILING):
    """(rows' shape of dtype dst with GUARD outside the slices, reduction bits, limited): RRX_debug_limit_host on every slice"""
    nt, row_frames, nch = rows.shape
    coefs = np.ascontiguousarray(coefs, dtype=np.float64)
    want = np.full(rows.shape, GUARD, dst)
    red, lim = np.full(nt, M.ONE), np.zeros(nt, np.uint64)
    for t, (of, n) in enumerate(clamped(table, row_frames)):
        if not n:
            continue
        x = np.ascontiguousarray(rows[t:t + 1, of:of + n])
        y = np.empty(x.shape, dst)
        need = F.limit_work_doubles(1, n, coefs.shape[1], L)
        work = np.empty(need)
        g = np.ascontiguousarray(gain[t:t + 1] if gain is not None else [1.0], dtype=np.float64)  # (the rows under unity are the rows)
        rc = F.lib().RRX_debug_limit_host(int(x.dtype == np.float64), x.ctypes.data, n, int(y.dtype == np.float64), y.ctypes.data, n, 1, n, nch,
                                          g.ctypes.data, float(ceiling), coefs.ctypes.data, coefs.shape[0], coefs.shape[1], L, H,
                                          red[t:].ctypes.data, lim[t:].ctypes.data, work.ctypes.data, need)
        assert rc == 0
        want[t, of:of + n] = y[0]
    return want, red, lim


def twin_window(rows, table, gain, L, H, first, frames, out, red, lim, coefs=M.BS1770, ceiling=CEILING, pad=3, row_frames=None):
    """RRX_debug_tracks_limit_window_host on the window [first, first + frames) of `rows`, from a minimal-coverage copy at a pitch
    of `pad` frames more, padded with +inf, into a destination of its own under GUARD, with an exactly sized work buffer under a
    guard; the emitted frames go to `out` [ntracks, row_frames, nch] (everything else of the destination must be GUARD still)."""
    nt, have, nch = rows.shape
    row_frames = have if row_frames is None else row_frames
    coefs = np.ascontiguousarray(coefs, dtype=np.float64)
    taps = coefs.shape[1]
    back, ahead = L - 1 + H + taps - 1, L - 1 + taps - 1
    b0, bn = coverage(first, frames, back, ahead, row_frames)
    fence = 64  # elements in front of either buffer and behind it: +inf around the source, so that a stray read shows
    bmem = np.full(nt * (bn + pad) * nch + 2 * fence, np.inf, rows.dtype)
    buf = bmem[fence:len(bmem) - fence].reshape(nt, bn + pad, nch)
    buf[:, :bn] = rows[:, b0:b0 + bn]
    dmem = np.full(nt * (frames + pad) * nch + 2 * fence, GUARD, out.dtype)
    dst = dmem[fence:len(dmem) - fence].reshape(nt, frames + pad, nch)
    need = F.tracks_limit_window_work_doubles(nt, frames, taps, L, H)
    work = np.full(need + 3, GUARD)
    g = None if gain is None else np.ascontiguousarray(gain, dtype=np.float64)
    tab = np.ascontiguousarray(table, dtype=np.uint64)
    rc = F.lib().RRX_debug_tracks_limit_window_host(tab.ctypes.data, nt, nch, int(rows.dtype == np.float64), buf.ctypes.data, bn + pad, b0, bn,
                                                    row_frames, first, frames, int(out.dtype == np.float64), dst.ctypes.data, frames + pad,
                                                    None if g is None else g.ctypes.data, float(ceiling), coefs.ctypes.data, coefs.shape[0],
                                                    taps, L, H, red.ctypes.data, lim.ctypes.data, work.ctypes.data, need)
    assert rc == 0, rc
    assert np.all(work[need:] == GUARD)
    assert np.all(dst[:, frames:] == GUARD) and np.all(dmem[:fence] == GUARD) and np.all(dmem[len(dmem) - fence:] == GUARD)
    for t, (of, n) in enumerate(clamped(table, row_frames)):
        lo, hi = max(of, first), min(of + n, first + frames)
        inside = np.zeros(frames, bool)
        if hi > lo:
            inside[lo - first:hi - first] = True
            out[t, lo:hi] = dst[t, lo - first:hi - first]
        assert np.all(dst[t, :frames][~inside] == GUARD), (t, first, frames)
