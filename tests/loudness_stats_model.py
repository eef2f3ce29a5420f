"""A numpy restatement of the loudness meter's arithmetic that include/ratelib_amd.h makes part of the ABI
(RRX_loudness_blocks_device, RRX_loudness_gate_groups_device, RRX_loudness_range_groups_device): the sliding block powers and
their maximum, the gate over the pooled blocks of groups of streams, and the gated percentiles.  Every rounding is one whole-array
operation (numpy fuses nothing); the serial sums are np.cumsum, as in loudness_model.gate, and the selection is np.sort."""
import numpy as np


def gate_thresholds(abs_lufs=-70.0, rel_lu=-10.0):
    return 10.0 ** ((abs_lufs + 0.691) / 10.0), 10.0 ** (rel_lu / 10.0)


def count(n, L, P, stride=None):
    nb = 0 if n < L else (n - L) // P + 1
    return nb if stride is None else min(nb, stride)


def blocks(energy, hop, L, P, hops=None, weights=None, stride=None):
    """RRX_loudness_blocks_device on energy [nstreams, nch, nhops]: (z, nblocks, max) -- z is a list of one array per stream,
    nblocks[s] long; `stride` clamps the block counts as blocks_stride does when d_blocks is given"""
    ns, nch, nh = energy.shape
    inv = np.float64(1.0) / (np.float64(L) * np.float64(hop))
    zs, nbs, top = [], np.zeros(ns, np.uint64), np.zeros(ns)
    for s in range(ns):
        n = nh if hops is None else min(int(hops[s]), nh)
        nb = count(n, L, P, stride)
        first = np.arange(nb) * P
        e = energy[s]
        with np.errstate(invalid="ignore", over="ignore"):
            q = e[:, first]
            for i in range(1, L):
                q = q + e[:, first + i]
            acc = np.zeros(nb)
            for ch in range(nch):
                acc = acc + (q[ch] if weights is None else np.float64(weights[ch]) * q[ch])
            z = acc * inv
            above = z[z > 0.0]  # from +0.0, `if (z > m) m = z`: the largest z above 0, NaNs skipped
        zs.append(z)
        nbs[s] = nb
        top[s] = above.max() if above.size else 0.0
    return zs, nbs, top


def _serial(values):
    """the serial ascending sum from +0.0"""
    return np.cumsum(values)[-1] if len(values) else np.float64(0.0)


def _stage(zs, group, ngroups, abs_threshold, t):
    """one stage of the gate: per stream over its passing blocks, then per group over its member streams ascending.
    t: None (the absolute gate alone) or T per group.  (sums [ngroups], counts [ngroups], the passing blocks per stream)"""
    sums, counts, passing = np.zeros(ngroups), np.zeros(ngroups, np.uint64), []
    for s, z in enumerate(zs):
        g = int(group[s])
        if not 0 <= g < ngroups:
            passing.append(z[:0])
            continue
        with np.errstate(invalid="ignore"):
            m = z > abs_threshold
            if t is not None:
                m = m & (z > t[g])
        passing.append(z[m])
        sums[g] = sums[g] + _serial(z[m])
        counts[g] += np.uint64(m.sum())
    return sums, counts, passing


def threshold(s1, n1, rel_factor):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float64(rel_factor) * (s1 / n1.astype(np.float64))


def gate_groups(zs, group, ngroups, abs_threshold=None, rel_factor=None):
    """RRX_loudness_gate_groups_device on the blocks of `blocks` above: [ngroups, 4] = S2, N2, S1, N1"""
    if abs_threshold is None:
        abs_threshold, rel_factor = gate_thresholds()
    s1, n1, _ = _stage(zs, group, ngroups, abs_threshold, None)
    s2, n2, _ = _stage(zs, group, ngroups, abs_threshold, threshold(s1, n1, rel_factor))
    return np.stack([s2, n2.astype(np.float64), s1, n1.astype(np.float64)], axis=1)


def range_groups(zs, group, ngroups, abs_threshold=None, rel_factor=None, low=10, high=95):
    """RRX_loudness_range_groups_device: [ngroups, 4] = P_low, P_high, N2, T"""
    if abs_threshold is None:
        abs_threshold, rel_factor = gate_thresholds(-70.0, -20.0)
    s1, n1, _ = _stage(zs, group, ngroups, abs_threshold, None)
    t = threshold(s1, n1, rel_factor)
    _, _, passing = _stage(zs, group, ngroups, abs_threshold, t)
    out = np.zeros((ngroups, 4))
    out[:, 3] = t
    for g in range(ngroups):
        members = [passing[s] for s in range(len(zs)) if int(group[s]) == g]
        pool = np.sort(np.concatenate(members)) if members else np.zeros(0)
        n = pool.size
        if n:
            out[g, 0] = pool[((n - 1) * low + 50) // 100]
            out[g, 1] = pool[((n - 1) * high + 50) // 100]
        out[g, 2] = n
    return out


def lufs(result):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(result[:, 1] > 0, -0.691 + 10.0 * np.log10(result[:, 0] / np.maximum(result[:, 1], 1.0)), -np.inf)


def power_lufs(z):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(z)


def range_lu(result):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(result[:, 2] > 0, 10.0 * np.log10(np.where(result[:, 2] > 0, result[:, 1], 1.0) / np.where(result[:, 2] > 0, result[:, 0], 1.0)), 0.0)


def as_rows(zs, stride, fill):
    """the blocks as the [nstreams, stride] buffer the calls exchange, `fill` where nothing is written"""
    out = np.full((len(zs), stride), fill)
    for s, z in enumerate(zs):
        out[s, :len(z)] = z
    return out
