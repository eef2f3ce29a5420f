"""The gapless stage calls held to their stream contract under a busy stream (include/ratelib_amd_album.h: device, hip_stream and
"only enqueues" are RRX_tracks_stage_device_samples', word for word; DESIGN.md 12, "Stream order").  Each entry point runs once
behind the gates of tests/stream_gate.py, through the C ABI and through its wrapper, as tests/test_gpu_stream_order.py runs their
siblings: the inputs are produced on the caller's stream behind a kernel that keeps it busy, the null stream is kept busy too, and
the bar is equality of bits with the same call made on an idle device.  tests/test_tracks_album_api.py holds the list of cases to
the header."""
import numpy as np
import pytest
import torch

import album_cases as AC
import foo_dsp_resampler_amd as F
import stream_gate as G
from stream_order_cases import GUARD, Guarded, dev, ok, rng

pytestmark = pytest.mark.gpu

FS, FO = 44100, 48000
LENGTHS, GROUPS = [2300, 40, 65, 2400], [0, 0, 0, -1]     # linked rows (LPC-free), album edges and a single (both kernels have work)
WINDOW = (2180, 63)                                         # across the end of the first row's backward extension (frame 2205)


@pytest.fixture(scope="module")
def stream():
    return G.independent_stream()


@pytest.fixture(autouse=True)
def no_case_behind_a_gpu_error():
    """a case that left the device in error is the last one: nothing more is started on it"""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:
        pytest.exit("the GPU reported an error, no further case is started: %s" % e, returncode=3)


def case():
    plan = F.tracks_plan_album(FS, FO, LENGTHS, GROUPS)
    x = rng(77).integers(-20000, 20000, (plan.src_total, 2)).astype(np.int16)
    return plan, dev(x), plan.to_device("cuda"), plan.links_to_device("cuda")


def stage_rows(run):
    plan, packed, table, links = case()
    n, R, total = len(plan), plan.row_frames, plan.src_total
    g, lib, entry = Guarded(), F.album.lib(), "RRX_tracks_stage_album_device"
    F.ratelib._ensure_init()
    rows = g.out((n, R, 2), torch.float32)
    run(lambda s: ok(lib.RRX_tracks_stage_album_device(-1, s.cuda_stream, FS, FO, table.data_ptr(), links.data_ptr(), n, 2, F.RRX_FMT_S16,
                                                       packed.data_ptr(), total, rows.data_ptr(), R), entry), [packed, table, links], g.bigs, entry)
    g.check(entry)
    # every frame was written, and both launches had work: a neighbour's frames in a linked edge, an LPC extension that is not silence
    assert not bool((rows == GUARD).any()) and float(rows[1, :int(plan.table[1].lead)].abs().max()) > 0 and float(rows[0, :2205].abs().max()) > 0
    g.reset()                                        # the Python wrapper forwards its stream
    run(lambda s: F.tracks_stage_album_device(packed, table, links, FS, FO, R, out=rows, stream=s), [packed, table, links], g.bigs, entry)
    g.check(entry)


def stage_window(run):
    plan, packed, table, links = case()
    n, R, total = len(plan), plan.row_frames, plan.src_total
    wf, wn = WINDOW
    g, lib, entry = Guarded(), F.album.lib(), "RRX_tracks_stage_album_window_device"
    F.ratelib._ensure_init()
    win = g.out((n, wn + 2, 2), torch.float32)
    run(lambda s: ok(lib.RRX_tracks_stage_album_window_device(-1, s.cuda_stream, FS, FO, table.data_ptr(), links.data_ptr(), n, 2, F.RRX_FMT_S16,
                                                              packed.data_ptr(), total, R, wf, wn, win.data_ptr(), wn + 2), entry),
        [packed, table, links], g.bigs, entry)
    g.check(entry)
    assert bool((win[:, wn:] == GUARD).all()) and not bool((win[:, :wn] == GUARD).any())
    g.reset()
    run(lambda s: F.tracks_stage_album_window_device(packed, table, links, FS, FO, R, wf, wn, out=win, stream=s), [packed, table, links], g.bigs, entry)
    g.check(entry)


CASES = {"RRX_tracks_stage_album_device": stage_rows, "RRX_tracks_stage_album_window_device": stage_window}


def test_the_cases_are_the_header_s_stream_taking_entry_points():
    assert sorted(CASES) == AC.header_functions()[1] == sorted(AC.STREAM_WRAPPER_OF)


@pytest.mark.parametrize("entry", sorted(CASES))
def test_the_call_keeps_its_stream_contract(entry, stream):
    seen = []

    def run(enqueue, inputs, outputs, label):
        seen.append(label)
        G.gated(enqueue, inputs, outputs, stream, label=label)

    CASES[entry](run)
    assert seen == [entry, entry]                    # the C call and the wrapper
