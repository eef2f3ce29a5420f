"""ctypes mirror of include/ratelib_amd_album.h: gapless albums in the ragged track path ("Gapless albums").

tracks_plan_album plans tracks of which some are cut from one master, tracks_stage_album_device and its window form stage them
from their neighbours.  The Resampler methods take the plan through `gapless=` (ratelib.py).  Same names, argument meaning and
error behaviour as the header; no signal processing and no fallback here either."""
import ctypes as C

import numpy as np

from . import ratelib as R

# every symbol include/ratelib_amd_album.h declares
ALBUM_SYMBOLS = ["RRX_tracks_plan_album", "RRX_tracks_stage_album_device", "RRX_tracks_stage_album_window_device",
                 "RRX_debug_tracks_stage_album_host"]
RRX_LINK_NONE = (1 << 64) - 1

_bound = False


class RRXTrackLink(C.Structure):
    """RRX_track_link (ratelib_amd_album.h): frames of the same album directly in front of and behind a track in the packed source"""
    _fields_ = [("back", C.c_ulonglong), ("ahead", C.c_ulonglong)]


def lib():
    """ratelib.lib() with the argument types of this header's calls (a library without them is an error, as everywhere)"""
    global _bound
    L = R.lib()
    if not _bound:
        P, vp, sz = C.POINTER, C.c_void_p, C.c_size_t
        L.RRX_tracks_plan_album.argtypes = [P(R.RRConfig), P(sz), P(C.c_int), C.c_int, P(R.RRXTrack), P(RRXTrackLink), P(sz), P(sz), P(sz), P(sz)]
        L.RRX_tracks_stage_album_device.argtypes = [C.c_int, vp, sz, sz, vp, vp, C.c_int, C.c_int, C.c_int, vp, sz, vp, sz]
        L.RRX_tracks_stage_album_window_device.argtypes = [C.c_int, vp, sz, sz, vp, vp, C.c_int, C.c_int, C.c_int, vp, sz, sz, sz, sz, vp, sz]
        L.RRX_debug_tracks_stage_album_host.argtypes = [sz, sz, vp, vp, C.c_int, C.c_int, C.c_int, vp, sz, sz, sz, sz, vp, sz]
        _bound = True
    return L


def available_symbols():
    L = R.lib()
    return [s for s in ALBUM_SYMBOLS if hasattr(L, s)]


class TracksAlbumPlan(R.TracksPlan):
    """RRX_tracks_plan_album's answer: a TracksPlan with `links` (a ctypes array of RRXTrackLink, one per track).
    `links_array()` is uint64 [ntracks, 2], `links_to_device(device)` uploads it (int64 [ntracks, 2]).  `subset(indices, pad)` is the
    batch table of some of the entries, in the order given, followed by `pad` zero-length entries: the packed source and
    destination stay the whole plan's (an entry is self-contained), row_frames is the subset's largest frames + 2 * lead."""

    def __init__(self, table, links, row_frames, out_row_cap, src_total, dst_total, rates):
        R.TracksPlan.__init__(self, table, row_frames, out_row_cap, src_total, dst_total)
        self.links, self.rates = links, rates

    def links_array(self):
        return np.frombuffer(self.links, dtype=np.uint64).reshape(len(self.links), 2).copy()

    def links_to_device(self, device):
        import torch
        return torch.from_numpy(self.links_array().view(np.int64)).to(device)

    def subset(self, indices, pad=0):
        indices = [int(i) for i in indices]
        n = len(indices) + int(pad)
        if n < 1:
            raise ValueError("a plan needs at least one track")
        table, links = (R.RRXTrack * n)(), (RRXTrackLink * n)()
        row = 0
        for k in range(n):
            if k < len(indices):
                e, ln = self.table[indices[k]], self.links[indices[k]]
                for f, _ in R.RRXTrack._fields_:
                    setattr(table[k], f, getattr(e, f))
                links[k].back, links[k].ahead = ln.back, ln.ahead
                row = max(row, int(e.frames + 2 * e.lead))
            else:
                links[k].back = links[k].ahead = RRX_LINK_NONE
        in_rate, out_rate = self.rates
        return TracksAlbumPlan(table, links, row, row * out_rate // in_rate + 2, self.src_total, self.dst_total, self.rates)


def _gapless_checked(gapless, ntracks):
    """the `gapless=` of a call: one int per track (negative: a single), as a list"""
    gapless = [int(v) for v in gapless]
    if len(gapless) != ntracks:
        raise ValueError("gapless is one group id per track: %d ids for %d tracks" % (len(gapless), ntracks))
    if any(not -(1 << 31) <= v < 1 << 31 for v in gapless):
        raise ValueError("a group id fits 32 signed bits")
    return gapless


def _tracks_plan_album(cfg, lengths, gapless):
    n = len(lengths)
    if n < 1:
        raise ValueError("a plan needs at least one track")
    if min(lengths) < 0:
        raise ValueError("track lengths are frame counts: none may be negative")
    gapless = _gapless_checked(gapless, n)
    fr = (C.c_size_t * n)(*[int(v) for v in lengths])
    gr = (C.c_int * n)(*gapless)
    table, links = (R.RRXTrack * n)(), (RRXTrackLink * n)()
    v = [C.c_size_t(0) for _ in range(4)]
    R._check(lib().RRX_tracks_plan_album(C.byref(cfg), fr, gr, n, table, links, *[C.byref(x) for x in v]), "RRX_tracks_plan_album")
    return TracksAlbumPlan(table, links, *[x.value for x in v], rates=(int(cfg.in_rate), int(cfg.out_rate)))


def tracks_plan_album(in_rate, out_rate, lengths, gapless, **kw):
    """Host-only: tracks_plan for tracks of which some are cut from one master (RRX_tracks_plan_album), as a TracksAlbumPlan.
    `gapless` is one group id per track: negative for a single, and consecutive tracks with one non-negative id are an album in
    play order.  Needs no GPU."""
    return _tracks_plan_album(R._config(in_rate, out_rate, **kw), list(lengths), gapless)


def _tracks_links(links, ntracks, dev):
    """the device copy of a plan's links: None, or a contiguous int64 tensor [ntracks, 2] on `dev`"""
    if links is None:
        return
    if str(links.dtype) != "torch.int64" or links.dim() != 2 or links.shape[1] != 2 or not links.is_cuda or not links.is_contiguous():
        raise TypeError("the links must be a contiguous int64 device tensor [ntracks, 2] (TracksAlbumPlan.links_to_device)")
    if links.shape[0] != ntracks:
        raise ValueError("the links have %d entries for %d tracks" % (links.shape[0], ntracks))
    if links.device != dev:
        raise TypeError("the links must be on %s" % (dev,))


def tracks_stage_album_device(packed, table, links, in_rate, out_rate, row_frames, out=None, stream=None):
    """tracks_stage_device with links (RRX_tracks_stage_album_device): `links` is the device copy of a plan's links
    (TracksAlbumPlan.links_to_device), or None for tracks_stage_device itself.  A linked edge of a row holds the neighbour's
    frames, copied from the packed source and converted like the track's own, with zeros where the album began inside the
    extension; an edge without a link is extrapolated, bit for bit as tracks_stage_device does it.  Everything else -- `packed`,
    `table`, the float32 rows returned, `out`, `stream`, "the call only enqueues" -- as there."""
    fmt, ntracks, nch, src_total = R._tracks_stage_source(packed, table)
    _tracks_links(links, ntracks, packed.device)
    out = R._tracks_stage_out(out, (ntracks, int(row_frames), nch), packed.device)
    packed = R._tracks_stage_pointer(packed)
    R._check(lib().RRX_tracks_stage_album_device(*R._where(packed.device, stream), int(in_rate), int(out_rate), table.data_ptr(), R._ptr(links),
                                                 ntracks, nch, fmt, packed.data_ptr(), src_total, R._ptr(out), int(row_frames)),
             "RRX_tracks_stage_album_device")
    return out


def tracks_stage_album_window_device(packed, table, links, in_rate, out_rate, row_frames, win_first, win_frames, out=None, stream=None):
    """tracks_stage_album_device on a window of the rows (RRX_tracks_stage_album_window_device), as tracks_stage_window_device is of
    tracks_stage_device: frames [win_first, win_first + win_frames) of every row, bit for bit; `out` and the return as there."""
    fmt, ntracks, nch, src_total = R._tracks_stage_source(packed, table)
    _tracks_links(links, ntracks, packed.device)
    row_frames, win_first, win_frames = R._tracks_window(row_frames, win_first, win_frames)
    if out is not None and (out.dim() != 3 or out.shape[1] < win_frames):
        raise TypeError("out must be a contiguous float32 tensor [%d, at least %d, %d] on %s" % (ntracks, win_frames, nch, packed.device))
    out = R._tracks_stage_out(out, (ntracks, win_frames if out is None else out.shape[1], nch), packed.device)
    packed = R._tracks_stage_pointer(packed)
    if not win_frames:  # (an empty tensor has no pointer, and there is nothing to do)
        return out
    R._check(lib().RRX_tracks_stage_album_window_device(*R._where(packed.device, stream), int(in_rate), int(out_rate), table.data_ptr(),
                                                        R._ptr(links), ntracks, nch, fmt, packed.data_ptr(), src_total, row_frames, win_first,
                                                        win_frames, R._ptr(out), out.shape[1]), "RRX_tracks_stage_album_window_device")
    return out
