"""numpy restatement of RRX_true_peak_device's arithmetic (include/ratelib_amd.h): the gain, the history in front of the call (a
state, or +0.0), the descending serial sum of every phase, the flushed tail, the two maxima on bit patterns and the state handed
on.  Every sum is a loop over k of whole-array fp64 operations -- a product, then a sum, one rounding each: numpy fuses nothing --
and every maximum is taken on uint64 views, so a NaN (sign cleared by fabs) lies above +inf and stays."""
import numpy as np

MAX_PHASES, MAX_TAPS = 8, 16
P0 = (14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68)
P1 = (-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155)
BS1770 = np.array([P0, P1, P1[::-1], P0[::-1]], dtype=np.float64) / 8192.0  # [4, 12], exact: numerators over a power of two


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def true_peak(x, coefs, gain=None, flush=True, state=None):
    """x: float32 / float64 [nstreams, frames, nch]; coefs: float64 [phases, taps]; gain: None or float64 [nstreams]; state: None
    (the history is +0.0) or float64 [nstreams, nch, 16] with entry j the gained sample j + 1 frames before frame 0 of x.
    Returns (true_peak, peak, state_out): the maxima of this call alone as uint64 bit patterns [nstreams, nch] (the caller
    accumulates with np.maximum), and the state after the last real frame, float64 [nstreams, nch, 16]."""
    coefs = np.asarray(coefs, dtype=np.float64)
    phases, taps = coefs.shape
    ns, frames, nch = x.shape
    halo = taps - 1
    with np.errstate(all="ignore"):
        g = x.astype(np.float64)
        if gain is not None:
            g = g * np.asarray(gain, dtype=np.float64)[:, None, None]
        hist = np.zeros((ns, halo, nch), dtype=np.float64)  # hist[:, halo - 1 - j] is the sample j + 1 frames back
        if state is not None:
            for j in range(halo):
                hist[:, halo - 1 - j, :] = state[:, :, j]
        evals = frames + (halo if flush and frames else 0)
        ext = np.concatenate([hist, g, np.zeros((ns, evals - frames, nch), dtype=np.float64)], axis=1)
        tp = np.zeros((ns, evals, nch), dtype=np.uint64)
        for p in range(phases):
            acc = np.zeros((ns, evals, nch), dtype=np.float64)
            for k in range(taps - 1, -1, -1):
                prod = coefs[p, k] * ext[:, halo - k:halo - k + evals, :]
                acc = acc + prod
            tp = np.maximum(tp, bits(np.fabs(acc)))
    tpk = tp.max(axis=1) if evals else np.zeros((ns, nch), dtype=np.uint64)
    pk = bits(np.fabs(g)).max(axis=1) if frames else np.zeros((ns, nch), dtype=np.uint64)
    state_out = np.zeros((ns, nch, MAX_TAPS), dtype=np.float64)
    real = ext[:, :halo + frames, :]
    for j in range(halo):
        state_out[:, :, j] = real[:, real.shape[1] - 1 - j, :]
    return tpk, pk, state_out


def as_double(b):
    return np.ascontiguousarray(b, dtype=np.uint64).view(np.float64)


def planted(rng, shape, dtype):
    """noise with the values that break careless arithmetic planted in it: 0, +-1, -0.0, +-inf, float32 denormals, and a NaN in the
    LAST channel of the last stream only (so that the neighbour channels can be checked exactly)"""
    x = (rng.standard_normal(shape) * 0.5).astype(dtype)
    ns, frames, nch = shape
    special = [0.0, 1.0, -1.0, -0.0, np.inf, -np.inf, 1e-40, -3e-42, 1.4e-45]
    flat = x.reshape(-1)
    if flat.size >= 4 * len(special):
        where = rng.choice(flat.size, size=len(special), replace=False)
        with np.errstate(all="ignore"):
            flat[where] = np.array(special, dtype=np.float64).astype(dtype)
    if frames >= 3:
        x[ns - 1, frames // 2, nch - 1] = np.nan
    return x
