"""Gapless albums by windows on the device (csrc/tracks_album.hip): tracks_stage_album_window_device against the whole rows of
tracks_stage_album_device, which tests/test_gpu_tracks_album.py holds to the model.  The bar is equality of bits, for windows of
1, 63 and tile - 1, tile, tile + 1 frames (the copy kernel's tile, csrc/tracks_album.hpp) at the row's ends, across every border of
a region, wholly inside an extension -- a linked one and an extrapolated one -- and wholly inside the zeros behind a short track."""
import functools

import numpy as np
import pytest

import album_cases as AC
import foo_dsp_resampler_amd as F
from test_gpu_tracks_album import FS, FO, INSIDE, SENTINEL, batch, on_device

pytestmark = pytest.mark.gpu

NCH = 2


@functools.lru_cache(maxsize=None)
def case(fmt, which):
    """(plan, packed source, device table, device links, whole rows as numpy) -- computed once, read-only"""
    lengths, groups = batch(NCH) if which == "tiles" else INSIDE
    plan = F.tracks_plan_album(FS, FO, lengths, groups)
    raw, _ = AC.source(fmt, plan.src_total, NCH, 4)
    packed = on_device(raw, 1 if fmt == F.RRX_FMT_S24_3 else 0)
    tab, lnk = plan.to_device("cuda"), plan.links_to_device("cuda")
    rows = F.tracks_stage_album_device(packed, tab, lnk, FS, FO, plan.row_frames).cpu().numpy()
    rows.setflags(write=False)
    return plan, packed, tab, lnk, rows


def windows(plan):
    """(first, frames) for every size, at the places the module docstring names"""
    R, tile = plan.row_frames, AC.tile_samples() // NCH
    e = plan.table[1]                                            # a linked row
    lead, end = int(e.lead), int(e.lead + e.frames)
    short_ext = int(plan.table[-1].frames + 2 * plan.table[-1].lead)   # the last row's track and extension end here: zeros behind
    out = set()
    for wn in (1, 63, tile - 1, tile, tile + 1):
        for wf in (0, 1, 100, lead - wn, lead - 1, lead, end - 1, end, end + 7, short_ext, short_ext + 5, R - wn):
            if 0 <= wf and wf + wn <= R:
                out.add((wf, wn))
    return sorted(out), lead, short_ext


@pytest.mark.parametrize("which", ["tiles", "inside"])
@pytest.mark.parametrize("fmt", AC.FORMATS)
def test_windows_are_the_rows_bit_for_bit(fmt, which):
    import torch
    plan, packed, tab, lnk, rows = case(fmt, which)
    n, R = len(plan), plan.row_frames
    wins, lead, short_ext = windows(plan)
    assert any(wf + wn <= lead for wf, wn in wins if wn == 63) and any(wf >= short_ext for wf, wn in wins if wn == 63)
    assert {wn for _, wn in wins} >= {1, 63} and (which != "tiles" or len({wn for _, wn in wins}) == 5)
    for wf, wn in wins:
        big = torch.full((n + 2, wn + 3, NCH), SENTINEL, dtype=torch.float32, device="cuda")
        got = F.tracks_stage_album_window_device(packed, tab, lnk, FS, FO, R, wf, wn, out=big[1:-1])
        assert got.data_ptr() == big[1:-1].data_ptr()
        host = big.cpu().numpy()
        assert (host[0] == SENTINEL).all() and (host[-1] == SENTINEL).all() and (host[1:-1, wn:] == SENTINEL).all(), (wf, wn, "written outside the window")
        assert np.array_equal(host[1:-1, :wn].view(np.uint32), rows[:, wf:wf + wn].view(np.uint32)), (fmt, which, wf, wn)


def test_windows_without_links_are_tracks_stage_window_device():
    plan, packed, tab, _, _ = case(F.RRX_FMT_S16, "tiles")
    R = plan.row_frames
    for wf, wn in ((0, 63), (2200, 4097), (R - 1, 1)):
        a = F.tracks_stage_album_window_device(packed, tab, None, FS, FO, R, wf, wn).cpu().numpy()
        b = F.tracks_stage_window_device(packed, tab, FS, FO, R, wf, wn).cpu().numpy()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (wf, wn)
    empty = F.tracks_stage_album_window_device(packed, tab, None, FS, FO, R, 5, 0)
    assert tuple(empty.shape) == (len(plan), 0, NCH)


def test_a_partition_into_windows_covers_the_rows():
    """windows of an odd size laid end to end: every frame of every row once, the same bits"""
    import torch
    plan, packed, tab, lnk, rows = case(F.RRX_FMT_S24_3, "tiles")
    R = plan.row_frames
    out = torch.full((len(plan), R, NCH), SENTINEL, dtype=torch.float32, device="cuda")
    step = 2999
    win = torch.empty((len(plan), step, NCH), dtype=torch.float32, device="cuda")
    for wf in range(0, R, step):
        wn = min(step, R - wf)
        F.tracks_stage_album_window_device(packed, tab, lnk, FS, FO, R, wf, wn, out=win)
        out[:, wf:wf + wn] = win[:, :wn]
    assert np.array_equal(out.cpu().numpy().view(np.uint32), rows.view(np.uint32))
