"""numpy restatement of RRX_limit_release_device's arithmetic (include/ratelib_amd.h) on top of limit_model.py: everything up to
the window minimum m is limit_model's, then the release as a block scan -- every block summarised from nothing, a serial carry
over the summaries, every block run again from its start state -- and limit_model's box, fmin and product on q in place of m.
The summary and the run are vectorised over (stream, block) and loop over the position inside a block; every step is a
whole-array fp64 operation with one rounding: numpy fuses nothing.  serial() is the plain recursion the blocked form is NOT
bit-equal to."""
import math

import numpy as np

import limit_model as M
from limit_model import BS1770, ONE, bits, planted, same_samples  # noqa: F401  (the tests take them from here)

MIN_BLOCK, MAX_BLOCK = 64, 65536


def coef(release_ms, rate):
    return math.exp(-1.0 / (release_ms * 1e-3 * rate))


def work_doubles(nstreams, frames, taps, lookahead, block):
    n = nstreams * (2 * (frames + taps + lookahead) + 4 * (-(-(frames + lookahead - 1) // block) + 1))
    return n if n < 2 ** 60 else 0


def release(m, a, block):
    """q [ns, J] of the entries m [ns, J] under the pole a, in blocks of `block` entries counted from entry 0"""
    ns, J = m.shape
    a = np.float64(a)
    b = np.float64(1.0) - a
    nb = -(-J // block)
    if not nb:
        return m.copy()
    v = np.ones((ns, nb * block))        # (the padding behind entry J - 1 is never used: every update below is masked)
    v[:, :J] = m
    v = v.reshape(ns, nb, block)
    n = np.minimum(block, J - np.arange(nb) * block)      # entries of every block
    with np.errstate(all="ignore"):
        # summaries
        C, A, B = v[:, :, 0].copy(), np.full((ns, nb), a), b * v[:, :, 0]
        for t in range(1, block):
            live = (t < n)[None, :]
            u = b * v[:, :, t]
            C = np.where(live, np.fmin(v[:, :, t], a * C + u), C)
            A = np.where(live, a * A, A)
            B = np.where(live, a * B + u, B)
        # carry
        S = np.ones((ns, nb + 1))
        for i in range(nb):
            S[:, i + 1] = np.fmin(C[:, i], A[:, i] * S[:, i] + B[:, i])
        # run
        q = np.empty((ns, nb, block))
        p = S[:, :nb].copy()
        for t in range(block):
            u = b * v[:, :, t]
            p = np.fmin(v[:, :, t], a * p + u)
            q[:, :, t] = p
    return q.reshape(ns, nb * block)[:, :J]


def serial(m, a):
    """the plain recursion p = fmin(m_j, a * p + b * m_j) from 1.0, per row of m [ns, J]"""
    a = np.float64(a)
    b = np.float64(1.0) - a
    q = np.empty_like(m)
    p = np.ones(m.shape[0])
    with np.errstate(all="ignore"):
        for j in range(m.shape[1]):
            u = b * m[:, j]
            p = np.fmin(m[:, j], a * p + u)
            q[:, j] = p
    return q


def window_minima(x, coefs, ceiling, lookahead, hold, gain=None):
    """(g [ns, frames, nch], m [ns, frames + L - 1]) of limit_model.limit, restated from its steps"""
    coefs = np.asarray(coefs, dtype=np.float64)
    ns, frames, nch = x.shape
    L, H, D = int(lookahead), int(hold), coefs.shape[1] - 1
    c = np.float64(ceiling)
    with np.errstate(all="ignore"):
        g = x.astype(np.float64)
        if gain is not None:
            g = g * np.asarray(gain, dtype=np.float64)[:, None, None]
        lev = M.levels(g, coefs).view(np.float64)
        over = lev > c
        r = np.where(over, c / np.where(over, lev, 1.0), 1.0)
        padded = np.concatenate([np.ones((ns, L - 1 + H)), r, np.ones((ns, L - 1 + H))], axis=1)
        m = M.window_min(padded, L + H + D)[:, :frames + L - 1]
    return g, m


def smooth(g, q, lookahead, dst):
    """limit_model.limit's box, fmin, product and statistics on the entries q"""
    ns, frames, nch = g.shape
    L = int(lookahead)
    with np.errstate(all="ignore"):
        acc = np.zeros((ns, frames))
        for i in range(L - 1, -1, -1):
            acc = acc + q[:, L - 1 - i:L - 1 - i + frames]
        s = np.fmin(acc * (1.0 / float(L)), q[:, L - 1:L - 1 + frames])
        y = (g * s[:, :, None]).astype(dst)
    red = np.minimum(bits(s).min(axis=1), ONE) if frames else np.full(ns, ONE)
    return y, s, red, (s < 1.0).sum(axis=1).astype(np.uint64)


def limit_release(x, coefs, ceiling, L, H, a, block, gain=None, dst=np.float64):
    """What limit_model.limit returns -- (y, s, reduction bits, limited) -- of RRX_limit_release_device"""
    g, m = window_minima(x, coefs, ceiling, L, H, gain)
    return smooth(g, release(m, a, block), L, dst)
