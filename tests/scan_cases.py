"""The case table of the packed meter calls (RRX_tracks_true_peak_packed_device / RRX_tracks_loudness_packed_device), shared by
tests/test_scan_api.py (the host twins, no device) and tests/test_gpu_scan.py (the kernels): sources of the four formats as they
are stored, their exact float64 values, tables, and the yardstick -- a one-stream RRX_debug_true_peak_host /
RRX_debug_loudness_host call per track on a float64 array of the exact conversion (first_frame = 0, no state, flush)."""
import os
import re

import numpy as np

import foo_dsp_resampler_amd as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RR_OK, RR_EXTUNINIT, RR_INVPARAM = 0, 5, 6
KINDS = {"f32": F.RRX_FMT_FLOAT, "s16": F.RRX_FMT_S16, "s24": F.RRX_FMT_S24_3, "s32": F.RRX_FMT_S32}
BITS = {"s16": 15, "s24": 23, "s32": 31}
BS1770 = np.array(F.TRUE_PEAK_FILTERS["bs1770"][2]).reshape(4, 12)
FILTERS = {"bs1770": BS1770, "3x5": np.random.default_rng(3).standard_normal((3, 5))}
KW48 = np.array(F.k_weighting(48000), dtype=np.float64)
HOPS = (16, 17, 33)  # around the pass kernel's 16-frame tile


def lds_doubles():
    """kTpLdsDoubles of csrc/true_peak.hpp: the doubles of the true-peak kernel's LDS tile"""
    text = open(os.path.join(ROOT, "foo_dsp_resampler_amd", "csrc", "true_peak.hpp")).read()
    return int(re.search(r"kTpLdsDoubles\s*=\s*(\d+)", text).group(1))


def tile_frames(nch, taps):
    """frames of one LDS tile (true_peak.hip, launch_src): what the halo leaves of kTpLdsDoubles"""
    return (lds_doubles() - (taps - 1) * nch) // nch


def lengths(taps):
    """track lengths: shorter than the filter, the stereo tile's seams and the seam of the second tile, one of about 5000"""
    fpt = tile_frames(2, taps)
    return [0, 1, taps - 2, fpt, fpt + 1, 2 * fpt + 1, 5003]


def hop_lengths(hop):
    """under one hop, exactly four hops, four hops and hop - 1 frames; a track without frames and a long one beside them"""
    return [hop - 1, 4 * hop, 4 * hop + hop - 1, 0, 1531]


def integers(kind, rng, shape):
    """random integer samples of the format's whole range, its two ends planted"""
    b = BITS[kind]
    v = rng.integers(-(1 << b), 1 << b, size=shape, dtype=np.int64)
    flat = v.reshape(-1)
    if flat.size >= 4:
        flat[rng.integers(0, flat.size)] = (1 << b) - 1
        flat[rng.integers(0, flat.size)] = -(1 << b)
    return v


def store(kind, v):
    """samples v [frames, nch] -- int64 for the integer formats, float for f32 -- as they are stored (s24: uint8 [frames, nch * 3],
    little endian) and their exact float64 values"""
    if kind == "f32":
        raw = np.ascontiguousarray(v, dtype=np.float32)
        return raw, raw.astype(np.float64)
    v = np.asarray(v, dtype=np.int64)
    exact = v.astype(np.float64) * 2.0 ** -BITS[kind]  # (an int of at most 32 bits and a power of two: exact)
    if kind == "s16":
        return np.ascontiguousarray(v.astype(np.int16)), exact
    if kind == "s32":
        return np.ascontiguousarray(v.astype(np.int32)), exact
    u = (v & 0xFFFFFF).astype(np.uint32)
    raw = np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=-1).astype(np.uint8)
    return np.ascontiguousarray(raw.reshape(v.shape[0], v.shape[1] * 3)), exact


def source(kind, lens, nch, seed):
    """tracks of `lens` frames laid end to end: (raw as stored, exact float64 [total, nch])"""
    rng = np.random.default_rng(seed)
    total = int(sum(lens))
    if kind == "f32":
        return store(kind, rng.standard_normal((total, nch)) * 0.5)
    return store(kind, integers(kind, rng, (total, nch)))


def table_of(lens):
    """packed_plan's table with the output side filled in as well (out_first = 0, out_frames = frames): the same entries then
    describe float64 rows that hold the tracks, for the row forms"""
    t = F.packed_plan(lens).array()
    t[:, 4] = t[:, 1]
    return t


def gains(n):
    return np.linspace(0.5, 1.7, n)


def ptr(a):
    return None if a is None else a.ctypes.data


def host_true_peak(kind, raw, table, nch, max_frames, gain=None, coefs=BS1770, src_total=None, tp=None, pk=None):
    """RRX_debug_tracks_true_peak_packed_host: (rc, true peak bits [n, nch], peak bits [n, nch])"""
    n = table.shape[0]
    coefs = np.ascontiguousarray(coefs, dtype=np.float64)
    tp = np.zeros((n, nch), np.uint64) if tp is None else tp
    pk = np.zeros((n, nch), np.uint64) if pk is None else pk
    total = raw.shape[0] if src_total is None else src_total
    table = np.ascontiguousarray(table, dtype=np.uint64)
    rc = F.lib().RRX_debug_tracks_true_peak_packed_host(ptr(table), n, nch, KINDS[kind], ptr(raw), total, max_frames, ptr(gain), ptr(coefs),
                                                        coefs.shape[0], coefs.shape[1], ptr(tp), ptr(pk))
    return rc, tp, pk


GUARD = 777.25


def host_loudness(kind, raw, table, nch, max_frames, hop, gain=None, coefs=KW48, src_total=None, stride=None):
    """RRX_debug_tracks_loudness_packed_host: (rc, energy [n, nch, stride] over GUARD, hops [n])"""
    n = table.shape[0]
    stride = max_frames // hop if stride is None else stride
    energy = np.full((n, nch, max(stride, 1)), GUARD)
    hops = np.full(n, 99, np.uint64)
    need = n * nch * (max_frames // hop) * 4
    work = np.zeros(max(need, 1))
    total = raw.shape[0] if src_total is None else src_total
    table = np.ascontiguousarray(table, dtype=np.uint64)
    rc = F.lib().RRX_debug_tracks_loudness_packed_host(ptr(table), n, nch, KINDS[kind], ptr(raw), total, max_frames, ptr(gain), ptr(coefs), hop,
                                                       ptr(energy), stride, ptr(hops), ptr(work), need)
    return rc, energy, hops


def ref_true_peak(exact, cuts, nch, gain=None, coefs=BS1770):
    """the yardstick: a one-stream RRX_debug_true_peak_host call per track on the float64 values; cuts = [(first, frames)]"""
    coefs = np.ascontiguousarray(coefs, dtype=np.float64)
    tp, pk = np.zeros((len(cuts), nch), np.uint64), np.zeros((len(cuts), nch), np.uint64)
    for t, (first, frames) in enumerate(cuts):
        x = np.ascontiguousarray(exact[first:first + frames])
        g = None if gain is None else np.ascontiguousarray(gain[t:t + 1])
        rc = F.lib().RRX_debug_true_peak_host(1, ptr(x), frames * nch, 1, frames, nch, ptr(g), 0, ptr(coefs), coefs.shape[0], coefs.shape[1], 1,
                                              None, None, tp[t:t + 1].ctypes.data, pk[t:t + 1].ctypes.data)
        assert rc == RR_OK
    return tp, pk


def ref_loudness(exact, cuts, nch, hop, stride, gain=None, coefs=KW48):
    """the yardstick: a one-stream RRX_debug_loudness_host call per track; energies beyond a track's hops stay GUARD"""
    energy = np.full((len(cuts), nch, max(stride, 1)), GUARD)
    hops = np.zeros(len(cuts), np.uint64)
    for t, (first, frames) in enumerate(cuts):
        k = min(frames // hop, stride)
        hops[t] = k
        if not k:
            continue
        x = np.ascontiguousarray(exact[first:first + k * hop])
        g = None if gain is None else np.ascontiguousarray(gain[t:t + 1])
        e = np.zeros((nch, k))
        work = np.zeros(nch * k * 4)
        rc = F.lib().RRX_debug_loudness_host(1, ptr(x), k * hop * nch, 1, k * hop, nch, ptr(g), 0, ptr(coefs), hop, None, None, ptr(e), k, ptr(work),
                                             work.size)
        assert rc == RR_OK
        energy[t, :, :k] = e
    return energy, hops


def cuts_of(table, src_total, max_frames):
    """the clamp of the header, restated: first = min(src_first, src_total), frames = min(frames, src_total - first, max_frames)"""
    out = []
    for e in np.asarray(table, dtype=np.uint64):
        first = min(int(e[0]), src_total)
        out.append((first, min(int(e[1]), src_total - first, max_frames)))
    return out
