"""numpy restatement of the state RRX_tracks_limit_release_window_device carries between two windows (include/ratelib_amd.h), on
top of limit_release_model.py: the state at an entry e of a slice is what the WHOLE-ROW scan has at that entry -- S_i of its
carry, the summary (C, A, B) of the entries [i * block, e) by a direct walk, and p = q[e - 1] of limit_release_model.release.
Also the work formula, and the expectation the host and the device tests share: the one-stream release call on every slice."""
import numpy as np

import foo_dsp_resampler_amd as F
import limit_release_model as R
import limit_window_cases as W

STATE = 8


def work_doubles(ntracks, win_frames, taps, lookahead, hold, block):
    n = ntracks * (2 * (win_frames + 2 * lookahead + hold + 2 * taps) + 4 * ((win_frames + lookahead - 1) // block + 2))
    return n if n < 2 ** 60 else 0


class Scan:
    """the whole-row scan of one slice's entries m [J]: q, the carry S [nb + 1] and the summaries of every prefix of every block"""

    def __init__(self, m, a, block):
        m = np.asarray(m, dtype=np.float64)
        J = len(m)
        self.block, self.J = block, J
        self.q = R.release(m[None], a, block)[0]
        a = np.float64(a)
        b = np.float64(1.0) - a
        nb = -(-J // block)
        v = np.ones(nb * block)
        v[:J] = m
        v = v.reshape(nb, block)
        # pre[k][i, t]: the summary of the entries [i * block, i * block + t] by the first-entry step and t extensions, in order
        pre = [np.empty((nb, block)) for _ in range(3)]
        with np.errstate(all="ignore"):
            C, A, B = v[:, 0].copy(), np.full(nb, a), b * v[:, 0]
            for t in range(block):
                if t:
                    u = b * v[:, t]
                    C, A, B = np.fmin(v[:, t], a * C + u), a * A, a * B + u
                pre[0][:, t], pre[1][:, t], pre[2][:, t] = C, A, B
            n = np.minimum(block, J - np.arange(nb) * block)
            self.S = np.ones(nb + 1)
            for i in range(nb):  # the whole block's summary is the prefix that ends at its last entry
                self.S[i + 1] = np.fmin(pre[0][i, n[i] - 1], pre[1][i, n[i] - 1] * self.S[i] + pre[2][i, n[i] - 1])
        self.pre = [p.reshape(-1) for p in pre]

    def state(self, e):
        """the eight doubles at entry e <= J"""
        i, r = divmod(e, self.block)
        s = np.zeros(STATE)
        s[0] = self.S[i]
        if r:
            s[1], s[2], s[3] = (p[e - 1] for p in self.pre)
            s[4] = self.q[e - 1]
        else:
            s[4] = self.S[i]
        return s


def scans(rows, table, gain, L, H, a, block, coefs=R.BS1770, ceiling=W.CEILING):
    """one Scan per track of the batch (None for an empty slice), from limit_release_model's window minima"""
    out = []
    for t, (of, n) in enumerate(W.clamped(table, rows.shape[1])):
        if not n:
            out.append(None)
            continue
        _, m = R.window_minima(rows[t:t + 1, of:of + n], coefs, ceiling, L, H, None if gain is None else gain[t:t + 1])
        out.append(Scan(m[0], a, block))
    return out


def states_after(scan_list, table, row_frames, end):
    """[ntracks, 8]: the state every track has once the windows up to row frame `end` are done, ascending from frame 0 and the
    first without a state -- zeros for a track not begun or without a frame, the state at its last entry for one that has ended"""
    out = np.zeros((len(scan_list), STATE))
    for t, (of, n) in enumerate(W.clamped(table, row_frames)):
        if n and end > of:
            out[t] = scan_list[t].state(min(end, of + n) - of)
    return out


def expected(rows, table, gain, L, H, a, block, dst, coefs=R.BS1770, ceiling=W.CEILING):
    """(rows' shape of dtype dst with GUARD outside the slices, reduction bits, limited): RRX_debug_limit_release_host on every slice"""
    nt, row_frames, nch = rows.shape
    coefs = np.ascontiguousarray(coefs, dtype=np.float64)
    want = np.full(rows.shape, W.GUARD, dst)
    red, lim = np.full(nt, R.ONE), np.zeros(nt, np.uint64)
    for t, (of, n) in enumerate(W.clamped(table, row_frames)):
        if not n:
            continue
        x = np.ascontiguousarray(rows[t:t + 1, of:of + n])
        y = np.empty(x.shape, dst)
        need = F.limit_release_work_doubles(1, n, coefs.shape[1], L, block)
        work = np.empty(need)
        g = np.ascontiguousarray(gain[t:t + 1] if gain is not None else [1.0], dtype=np.float64)
        rc = F.lib().RRX_debug_limit_release_host(int(x.dtype == np.float64), x.ctypes.data, n, int(y.dtype == np.float64), y.ctypes.data, n, 1, n,
                                                  nch, g.ctypes.data, float(ceiling), coefs.ctypes.data, coefs.shape[0], coefs.shape[1], L, H,
                                                  float(a), block, red[t:].ctypes.data, lim[t:].ctypes.data, work.ctypes.data, need)
        assert rc == 0
        want[t, of:of + n] = y[0]
    return want, red, lim


def twin_window(rows, table, gain, L, H, a, block, first, frames, out, red, lim, state_in, coefs=R.BS1770, ceiling=W.CEILING, pad=3,
                row_frames=None, state_out=True):
    """RRX_debug_tracks_limit_release_window_host on the window [first, first + frames) of `rows`, with the fenced buffers of
    limit_window_cases.twin_window: a minimal-coverage copy padded with +inf, a destination of its own under GUARD, an exactly
    sized work buffer and an exactly sized outgoing state under guards.  The emitted frames go to `out`; returns the state."""
    nt, have, nch = rows.shape
    row_frames = have if row_frames is None else row_frames
    coefs = np.ascontiguousarray(coefs, dtype=np.float64)
    taps = coefs.shape[1]
    back, ahead = L - 1 + H + taps - 1, L - 1 + taps - 1
    b0, bn = W.coverage(first, frames, back, ahead, row_frames)
    fence = 64
    bmem = np.full(nt * (bn + pad) * nch + 2 * fence, np.inf, rows.dtype)
    buf = bmem[fence:len(bmem) - fence].reshape(nt, bn + pad, nch)
    buf[:, :bn] = rows[:, b0:b0 + bn]
    dmem = np.full(nt * (frames + pad) * nch + 2 * fence, W.GUARD, out.dtype)
    dst = dmem[fence:len(dmem) - fence].reshape(nt, frames + pad, nch)
    need = F.tracks_limit_release_window_work_doubles(nt, frames, taps, L, H, block)
    assert need == work_doubles(nt, frames, taps, L, H, block) and need > 0
    work = np.full(need + 3, W.GUARD)
    smem = np.full(nt * STATE + 2 * fence, W.GUARD)
    g = None if gain is None else np.ascontiguousarray(gain, dtype=np.float64)
    tab = np.ascontiguousarray(table, dtype=np.uint64)
    sin = None if state_in is None else np.ascontiguousarray(state_in, dtype=np.float64)
    before = None if sin is None else sin.copy()
    rc = F.lib().RRX_debug_tracks_limit_release_window_host(
        tab.ctypes.data, nt, nch, int(rows.dtype == np.float64), buf.ctypes.data, bn + pad, b0, bn, row_frames, first, frames,
        int(out.dtype == np.float64), dst.ctypes.data, frames + pad, None if g is None else g.ctypes.data, float(ceiling), coefs.ctypes.data,
        coefs.shape[0], taps, L, H, float(a), block, None if sin is None else sin.ctypes.data,
        smem[fence:].ctypes.data if state_out else None, red.ctypes.data, lim.ctypes.data, work.ctypes.data, need)
    assert rc == 0, rc
    assert np.all(work[need:] == W.GUARD)
    assert np.all(smem[:fence] == W.GUARD) and np.all(smem[len(smem) - fence:] == W.GUARD)
    assert before is None or np.array_equal(before.view(np.uint64), sin.view(np.uint64))
    assert np.all(dst[:, frames:] == W.GUARD) and np.all(dmem[:fence] == W.GUARD) and np.all(dmem[len(dmem) - fence:] == W.GUARD)
    for t, (of, n) in enumerate(W.clamped(table, row_frames)):
        lo, hi = max(of, first), min(of + n, first + frames)
        inside = np.zeros(frames, bool)
        if hi > lo:
            inside[lo - first:hi - first] = True
            out[t, lo:hi] = dst[t, lo - first:hi - first]
        assert np.all(dst[t, :frames][~inside] == W.GUARD), (t, first, frames)
    return smem[fence:fence + nt * STATE].reshape(nt, STATE).copy() if state_out else None
