"""The numpy model of gapless albums (include/ratelib_amd_album.h), written from the header's rules and nothing else: the plan's four
formulas in Python integers, and the rows of the stage pass frame by frame.  What the model cannot state -- the LPC extension of an
edge without a link -- it marks, and the tests take those frames from tracks_stage_device, whose frames they are by contract."""
import ctypes as C
from math import gcd

import numpy as np

import foo_dsp_resampler_amd as F

NONE = F.RRX_LINK_NONE
UNTOUCHED = np.float32(777.25)            # what the twin's buffer holds where it writes nothing


def ceil_div(a, b):
    return -(-a // b)


def plan_model(fs, fo, lengths, groups, **kw):
    """(table [n, 6], links [n, 2], row_frames, out_row_cap, src_total, dst_total) as Python integers"""
    n_add, n_drop, _, _ = F.edge_geometry(fs, fo)
    g = gcd(fs, fo)
    r1, r2 = fs // g, fo // g
    table, links = [], []
    src = dst = row = 0
    t0, n = 0, len(lengths)
    while t0 < n:
        t1 = t0 + 1
        if groups[t0] >= 0:
            while t1 < n and groups[t1] == groups[t0]:
                t1 += 1
        A = sum(lengths[t0:t1])
        album = groups[t0] >= 0 and A > 64
        album_out = F.track_geometry(fs, fo, A, **kw)[3] if album else 0
        S = 0
        for t in range(t0, t1):
            if not album:
                lead, ext, out_first, out_frames = F.track_geometry(fs, fo, lengths[t], **kw)
                back = ahead = NONE
            else:
                ph = S % r1
                lead = n_add + ph
                ext = lengths[t] + 2 * lead
                out_first = n_drop + ceil_div(ph * r2, r1)
                end = ceil_div((S + lengths[t]) * r2, r1) if t + 1 < t1 else album_out
                out_frames = max(end - ceil_div(S * r2, r1), 0)
                back = S if t > t0 else NONE
                ahead = A - S - lengths[t] if t + 1 < t1 else NONE
            table.append((src, lengths[t], lead, out_first, out_frames, dst))
            links.append((back, ahead))
            src, dst, S, row = src + lengths[t], dst + out_frames, S + lengths[t], max(row, ext)
        t0 = t1
    return table, links, row, row * fo // fs + 2, src, dst


def to_float(x, fmt):
    """a packed source as the float32 samples the rows hold: x = (float)((double)s * 2^-bits), one rounding"""
    if fmt == F.RRX_FMT_FLOAT:
        return np.asarray(x, np.float32)
    if fmt == F.RRX_FMT_S24_3:
        b = np.asarray(x, np.uint8).reshape(x.shape[0], -1, 3).astype(np.int32)
        s = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
        s = np.where(s >= 1 << 23, s - (1 << 24), s)
        return (s.astype(np.float64) * 2.0 ** -23).astype(np.float32)
    bits = 15 if fmt == F.RRX_FMT_S16 else 31
    return (np.asarray(x).astype(np.float64) * 2.0 ** -bits).astype(np.float32)


def pack_s24(s):
    """int32 samples in [-2^23, 2^23) [frames, nch] as packed little-endian bytes [frames, nch * 3]"""
    u = (np.asarray(s, np.int64) & 0xFFFFFF).astype(np.uint32)
    b = np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=-1).astype(np.uint8)
    return b.reshape(s.shape[0], -1)


def stage_model(table, links, src, row_frames):
    """(rows float32 [n, row_frames, nch], written bool [n, row_frames]): `src` is the packed source as float32 [src_total, nch].
    The clamps are those of RRX_tracks_stage_device (ratelib_amd.h), the linked edges the rule of ratelib_amd_album.h; the frames
    of an edge without a link are not written (False)."""
    S, nch = src.shape
    n, R = len(table), int(row_frames)
    rows = np.zeros((n, R, nch), np.float32)
    written = np.ones((n, R), bool)
    for t, (e, ln) in enumerate(zip(table, links)):
        src_first, frames, lead = int(e[0]), int(e[1]), int(e[2])
        lead = min(lead, R)
        frames = min(frames, R - lead)
        fwd = min(lead, R - lead - frames)
        first = min(src_first, S)
        have = min(frames, S - first)
        rows[t, lead:lead + have] = src[first:first + have]
        back, ahead = int(ln[0]), int(ln[1])
        if back == NONE:
            written[t, :lead] = False
        else:
            b = min(lead, back, first)
            rows[t, lead - b:lead] = src[first - b:first]
        if ahead == NONE:
            written[t, lead + frames:lead + frames + fwd] = False
        elif have == frames:
            a = min(fwd, ahead, S - first - frames)
            rows[t, lead + frames:lead + frames + a] = src[first + frames:first + frames + a]
    return rows, written


def table_array(table):
    return np.array([[int(v) for v in e] for e in table], dtype=np.uint64).reshape(len(table), 6)


def links_array(links):
    return np.array([[int(v) for v in e] for e in links], dtype=np.uint64).reshape(len(links), 2)


def twin(fs, fo, table, links, packed, fmt, nch, src_total, row_frames, win=None, stride=None, rc=False):
    """RRX_debug_tracks_stage_album_host on host arrays: the window buffer [n, stride, nch], holding UNTOUCHED where nothing was
    written.  `links` None: the call without links.  `rc`: return the call's code instead of asserting it."""
    tab = np.ascontiguousarray(table_array(table))
    lnk = None if links is None else np.ascontiguousarray(links_array(links))
    wf, wn = (0, row_frames) if win is None else win
    stride = wn if stride is None else stride
    out = np.full((len(tab), max(stride, 1), nch), UNTOUCHED, np.float32)
    packed = np.ascontiguousarray(packed)
    if not packed.size:
        packed = np.zeros(16, packed.dtype)
    code = F.album.lib().RRX_debug_tracks_stage_album_host(fs, fo, tab.ctypes.data, None if lnk is None else lnk.ctypes.data, len(tab), nch, fmt,
                                                           packed.ctypes.data, src_total, row_frames, wf, wn, out.ctypes.data, stride)
    if rc:
        return code
    assert code == 0, code
    return out[:, :stride]


def plan_raw(cfg, lengths, groups, ntracks=None, null=()):
    """RRX_tracks_plan_album through ctypes with any argument nulled: (code, table, links, the four outputs)"""
    n = len(lengths)
    fr = (C.c_size_t * max(n, 1))(*lengths)
    gr = (C.c_int * max(n, 1))(*groups)
    table, links = (F.RRXTrack * max(n, 1))(), (F.RRXTrackLink * max(n, 1))()
    v = [C.c_size_t(0xdead) for _ in range(4)]
    a = dict(config=C.byref(cfg) if cfg is not None else None, frames=fr, group=gr, table=table, links=links, row=C.byref(v[0]), cap=C.byref(v[1]),
             src=C.byref(v[2]), dst=C.byref(v[3]))
    for k in null:
        a[k] = None
    code = F.album.lib().RRX_tracks_plan_album(a["config"], a["frames"], a["group"], n if ntracks is None else ntracks, a["table"], a["links"],
                                               a["row"], a["cap"], a["src"], a["dst"])
    return code, table, links, [x.value for x in v]
