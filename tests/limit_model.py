"""numpy restatement of RRX_limit_device's arithmetic (include/ratelib_amd.h): the gain, the detector's level over a stream's
channels (the descending serial sum of every phase and the sample's own magnitude, as maxima on bit patterns), the reduction each
detector frame demands, the window minimum, the box sum as a loop from the oldest window to the newest, the fmin and the product.
Every step is a whole-array fp64 operation with one rounding: numpy fuses nothing.  The filter table and the planted inputs are
true_peak_model's."""
import numpy as np

from true_peak_model import BS1770, bits, planted  # noqa: F401  (the tests take them from here)

MAX_LOOKAHEAD, MAX_HOLD = 1024, 4096
ONE = np.float64(1.0).view(np.uint64)


def work_doubles(nstreams, frames, taps, lookahead):
    n = nstreams * 2 * (frames + taps + lookahead)
    return n if n < 2 ** 60 else 0


def levels(g, coefs):
    """lev[F] as uint64 bit patterns [nstreams, frames + taps - 1] of the gained frames g [nstreams, frames, nch]"""
    phases, taps = coefs.shape
    ns, frames, nch = g.shape
    halo = taps - 1
    evals = frames + halo
    ext = np.concatenate([np.zeros((ns, halo, nch)), g, np.zeros((ns, halo, nch))], axis=1)
    lev = np.zeros((ns, evals, nch), dtype=np.uint64)
    for p in range(phases):
        acc = np.zeros((ns, evals, nch), dtype=np.float64)
        for k in range(taps - 1, -1, -1):
            prod = coefs[p, k] * ext[:, halo - k:halo - k + evals, :]
            acc = acc + prod
        lev = np.maximum(lev, bits(np.fabs(acc)))
    lev = np.maximum(lev, bits(np.fabs(ext[:, halo:halo + evals, :])))  # a[F]: +0.0 behind the last frame
    return lev.max(axis=2)


def window_min(r, width):
    """min over [i, i + width) of every row of r [ns, n], for i in [0, n - width]: doubling, exact in any order"""
    w, a = 1, r
    while 2 * w <= width:
        a = np.minimum(a[:, :a.shape[1] - w], a[:, w:])
        w *= 2
    rest = width - w
    n = r.shape[1] - width + 1
    return np.minimum(a[:, :n], a[:, rest:rest + n])


def limit(x, coefs, ceiling, lookahead, hold, gain=None, dst=np.float64):
    """x: float32 / float64 [nstreams, frames, nch]; coefs: float64 [phases, taps]; gain: None or float64 [nstreams].  Returns
    (y [nstreams, frames, nch] of dtype dst, s [nstreams, frames], reduction bits [nstreams], limited [nstreams]): the statistics
    of this call alone, from a reduction preset to 1.0."""
    coefs = np.asarray(coefs, dtype=np.float64)
    taps = coefs.shape[1]
    ns, frames, nch = x.shape
    L, H, D = int(lookahead), int(hold), taps - 1
    c = np.float64(ceiling)
    with np.errstate(all="ignore"):
        g = x.astype(np.float64)
        if gain is not None:
            g = g * np.asarray(gain, dtype=np.float64)[:, None, None]
        lev = levels(g, coefs).view(np.float64)                       # [ns, frames + D]
        over = lev > c                                                # (a NaN fails)
        r = np.where(over, c / np.where(over, lev, 1.0), 1.0)
        # m[k], k in [-(L-1), frames), covers F in [k - H, k + L - 1 + D]: pad r with 1.0 so that index 0 is F = -(L-1) - H
        front, width = L - 1 + H, L + H + D
        padded = np.concatenate([np.ones((ns, front)), r, np.ones((ns, L - 1 + H))], axis=1)
        m = window_min(padded, width)[:, :frames + L - 1]             # m[:, j] is m[k = j - (L-1)]
        acc = np.zeros((ns, frames))
        for i in range(L - 1, -1, -1):                                # m[n - i] is column n + (L-1) - i
            acc = acc + m[:, L - 1 - i:L - 1 - i + frames]
        s = np.fmin(acc * (1.0 / float(L)), m[:, L - 1:L - 1 + frames])
        y = (g * s[:, :, None]).astype(dst)
    red = np.minimum(bits(s).min(axis=1), ONE) if frames else np.full(ns, ONE)
    return y, s, red, (s < 1.0).sum(axis=1).astype(np.uint64)


def same_samples(got, want):
    """bit for bit, a NaN where the model has a NaN"""
    u = np.uint64 if want.dtype == np.float64 else np.uint32
    g, w = np.ascontiguousarray(got).view(u), np.ascontiguousarray(want).view(u)
    nan = np.isnan(want)
    return got.dtype == want.dtype and np.array_equal(g[~nan], w[~nan]) and bool(np.isnan(got[nan]).all())
