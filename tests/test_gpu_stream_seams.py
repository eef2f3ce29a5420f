"""The output stage and the meters past their launch and chunk seams, on the device.  Every launcher that takes streams or tracks in
slices of 32768 (grid.y is a 16-bit count) -- finish.hip, the three of finish_shaped.hip, true_peak.hip, loudness.hip with its
carry kernel, launch_loudness_blocks, finish_typed and stage_typed of tracks.hip -- runs 32768 + 3 streams or tracks whose two
sides of the seam differ in samples, gain, state, hop count and table entry; RRX_loudness_gate_device, one workgroup a stream, runs the same count;
the two group kernels of loudness_stats.hip walk several of their 64- and 256-stream chunks, with chunks that hold no member of a
group and members without blocks at the chunk edges; and the 2^22 split of launch_streams, launch_sums and the range group loop is
crossed.  The inputs, the references and the caller are seam_cases.py's; the references are the numpy models over all streams
except where the docstring of a test says otherwise, and tests/test_stream_seams_api.py holds what is used instead to the models.
Everything is compared as bit patterns, every output starts as a guard pattern, and each test asserts that its case is not
trivial: the two sides differ and the statistics are alive on both.

Left out: the grid-stride loop of the blocks kernel -- gx is capped at 2^22 workgroups of 256 blocks, which takes more than 10^9
blocks in one stream."""
import time

import numpy as np
import pytest
import torch

import foo_dsp_resampler_amd as F
import loudness_stats_model as S
import seam_cases as K
from test_gpu_tracks import todays_row

pytestmark = pytest.mark.gpu
SUB = K.subset()


def equal_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def same_patterns(got, want):
    """uint64 patterns of doubles: equal, or a NaN in both (an infinite sample leaves NaNs in a filter's sums, and the interface
    promises that a NaN stays, not its payload)"""
    g, w = np.ascontiguousarray(got).view(np.float64), np.ascontiguousarray(want).view(np.float64)
    return g.shape == w.shape and bool(np.all((g.view(np.uint64) == w.view(np.uint64)) | (np.isnan(g) & np.isnan(w))))


# --------------------------------------------------------------------------------------------------------- the 32768 seam

@pytest.mark.parametrize("key", list(K.FINISH))
def test_finish_past_32768_streams(key):
    """f32-s16 and f64-s24 with 5 frames, measure-only with one, and 257 channels of 2 frames on the kernel with its channel table
    in LDS (lcm(4, 257) = 1028 > kSpanMax)"""
    got, want = K.finish_call(key, True), K.finish_model(key)
    assert (got[0] is None) == (want[0] is None) == (key == "measure")
    assert got[0] is None or np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert K.two_sides_differ(K.finish_input(key), K.gains(), want[1]) and (got[0] is None or K.two_sides_differ(want[0]))
    assert K.live_on_both_sides(want[1] > K.PEAK0) and K.live_on_both_sides(want[2] - K.CLIPPED0) and (want[1] > K.PEAK0).mean() > 0.9


@pytest.mark.parametrize("key", list(K.SHAPED))
def test_finish_shaped_past_32768_streams(key):
    """orders 9 and 4 (two kK instantiations), 9 frames from absolute frame 2 in segments of 4, a state per stream in and out"""
    got, want = K.shaped_call(key, True), K.shaped_model(key)
    for g, w, name in zip(got, want, ("bytes", "peak", "clipped", "state")):
        assert equal_bytes(g, w), name
    x, st = K.shaped_input(key)
    assert K.two_sides_differ(x, st, want[0], want[1], want[3]) and K.live_on_both_sides(want[2] - K.CLIPPED0) and K.live_on_both_sides(want[3])


@pytest.mark.parametrize("key", list(K.TRUE_PEAK))
def test_true_peak_past_32768_streams(key):
    """the BS.1770 template and the generic one with a state per stream in and out, and the direct kernel at its smallest shape
    (257 channels under 16 taps: nch * taps > 4096), which runs from frame 0 without states -- they are 16 doubles a channel"""
    got, want = K.tp_call(key, True), K.tp_model(key)
    assert np.array_equal(got[0], np.maximum(want[0], K.PEAK0)) and np.array_equal(got[1], np.maximum(want[1], K.PEAK0))
    assert (got[2] is None) == (key == "direct") and (got[2] is None or np.array_equal(K.bits(got[2]), K.bits(want[2])))
    x, st = K.tp_input(key)
    assert K.two_sides_differ(x, want[0], want[1]) and (st is None or K.two_sides_differ(st, want[2])) and (want[0] > K.PEAK0).all()


@pytest.mark.parametrize("double", [False, True], ids=["f32", "f64"])
def test_loudness_past_32768_streams(double):
    """3 whole hops of 3 frames and a remainder from the second hop of the stream on, a state per stream in and out: both pass
    kernels and the carry kernel"""
    (e, so), (we, ws) = K.loudness_call(double, True), K.loudness_model(double)
    assert np.array_equal(K.bits(e[:, :, 1:1 + K.L_HOPS]), K.bits(we)) and np.array_equal(K.bits(so), K.bits(ws))
    assert (e[:, :, 0] == K.GUARD).all() and (e[:, :, 1 + K.L_HOPS:] == K.GUARD).all()
    x, st = K.loudness_input(double)
    assert K.two_sides_differ(x, st, we, ws) and (we > 0).all()


def test_gate_over_32771_streams():
    got, want = K.gate_call(True), K.gate_model()
    assert np.array_equal(K.bits(got), K.bits(want))
    e, hops = K.hop_energies()
    assert K.two_sides_differ(e, hops, want[:, 2:])
    assert (want[:K.SLICE, 3] > want[:K.SLICE, 1]).any() and (want[:K.SLICE, 1] > 0).any() and (want[:K.SLICE, 3] == 0).any()
    assert want[K.SLICE, 3] == 0 and want[K.SLICE + 1, 3] == 1 and want[K.N - 1, 3] == 2 and want[K.N - 1, 1] == 1


@pytest.mark.parametrize("L,P", K.BLOCK_SHAPES)
def test_blocks_past_32768_streams(L, P):
    (b, nb, mx), (wb, wn, wm) = K.blocks_call(L, P, True), K.blocks_model(L, P)
    assert np.array_equal(K.bits(b), K.bits(wb)) and np.array_equal(nb, wn) and np.array_equal(K.bits(mx), K.bits(wm))
    none, nb, mx = K.blocks_call(L, P, True, blocks=False)            # d_blocks NULL
    assert none is None and np.array_equal(nb, wn) and np.array_equal(K.bits(mx), K.bits(wm))
    assert K.live_on_both_sides(wn) and K.live_on_both_sides(wn == 0) and K.two_sides_differ(K.block_hops())
    assert wm[K.N - 1] > 0 and wm[K.N - 1] != wm[K.N - 1 - K.SLICE] and wn[K.N - 1] != wn[K.N - 1 - K.SLICE]


def check_tracks(got, want, tab):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert K.two_sides_differ(tab[:, 3], tab[:, 4], tab[:, 5]) and K.live_on_both_sides(want[2] - K.CLIPPED0)
    empty = tab[:, 4] == 0
    assert K.live_on_both_sides(empty) and (want[1][empty] == K.PEAK0).all() and (want[1][~empty] > K.PEAK0).mean() > 0.9
    peaks = want[1].view(np.float64)
    assert not ((peaks > 1e29) & np.isfinite(peaks)).any()            # the huge frames around a slice are not the track's


@pytest.mark.parametrize("form,double,fmt", [("rows", False, F.RRX_FMT_S16), ("windows", True, F.RRX_FMT_S24_3)])
def test_tracks_finish_past_32768_tracks(form, double, fmt):
    """RRX_tracks_finish_device, and RRX_tracks_finish_window_device over two windows, on rows of 8 frames with slices of 0..5:
    the model of the uniform call on every track's slice (seam_cases.track_slices)"""
    check_tracks(K.tracks_finish_call(double, fmt, form), K.tracks_finish_model(double, fmt), K.track_table()[0])


@pytest.mark.parametrize("form,double,fmt,order", [("shaped", False, F.RRX_FMT_S16, 9), ("shaped-windows", True, F.RRX_FMT_S24_3, 4)])
def test_tracks_finish_shaped_past_32768_tracks(form, double, fmt, order):
    """RRX_tracks_finish_shaped_device, and the window form over two windows with its ping-ponged state.  Bytes and statistics
    against shaped_model over all tracks.  The state after the last window: against the host twin over all tracks, and against
    shaped_model on each track's own slice on the tracks around the seam and about 50 more"""
    got = K.tracks_finish_call(double, fmt, form, order)
    check_tracks(got, K.tracks_shaped_model(double, fmt, order), K.track_table()[0])
    if form == "shaped-windows":
        twin = K.tracks_finish_call(double, fmt, form, order, on_device=False)
        assert np.array_equal(K.bits(got[3]), K.bits(twin[3]))
        assert np.array_equal(K.bits(got[3][SUB]), K.bits(K.tracks_shaped_model(double, fmt, order, SUB)[3]))
        assert K.two_sides_differ(got[3][:, :, :order])


@pytest.mark.parametrize("double", [False, True], ids=["f32", "f64"])
def test_tracks_true_peak_and_loudness_past_32768_tracks(double):
    tab, _ = K.track_table()
    (tp, pk), (wtp, wpk) = K.tracks_true_peak_call(double), K.tracks_true_peak_model(double)
    assert same_patterns(tp, np.maximum(wtp, K.PEAK0)) and np.array_equal(pk, np.maximum(wpk, K.PEAK0))
    assert wtp[K.SLICE].all() and (wtp[K.SLICE] != wtp[0]).all() and (wtp[tab[:, 4] > 0] > K.PEAK0).mean() > 0.9 and (wtp[tab[:, 4] == 0] == 0).all()
    (e, hops), (we, wh) = K.tracks_loudness_call(double), K.tracks_loudness_model(double)
    assert np.array_equal(hops, wh) and wh[K.SLICE] == 2 and set(wh[:K.SLICE].tolist()) == {0, 1, 2}
    written = np.arange(K.T_ESTRIDE)[None, None, :] < wh[:, None, None]
    full = np.full(e.shape, K.GUARD)
    full[:, :, :2] = we
    assert K.same(e, np.where(written, full, K.GUARD)) and (we[wh == 2] > 0).mean() > 0.8
    assert np.isfinite(we[K.SLICE]).all() and (we[K.SLICE] != we[0]).all()


def test_tracks_stage_past_32768_tracks():
    """tracks_copy_kernel in two slices, and the LPC grid over 32771 * 2 * 2 workgroups: tracks of 0..70 frames of two channels at
    1000 -> 2000 Hz, where an extension is 50 frames, so that a row is 170 frames; five of every seven tracks are above the 64
    frames from which a track is extended.  The LPC extension has no numpy model, and today's buffers are two device calls a
    track.  So every row is held to the same call on the tracks before the seam and on those behind it, each a launch with
    t0 == 0, which tests/test_gpu_tracks.py holds to today's buffers; the tracks around the seam and about 50 more are held to
    today's buffers here"""
    fs, fo, nch = 1000, 2000, 2
    lengths = np.array([0, 70, 65, 69, 40, 66, 64])[np.arange(K.N) % 7]      # 70, 65 and 69 frames behind the seam
    plan = F.tracks_plan(fs, fo, lengths.tolist())
    R, tab = plan.row_frames, plan.array()
    assert R == 170 and K.two_sides_differ(lengths, tab[:, 0]) and int(tab[K.SLICE, 2]) == int(tab[K.N - 1, 2]) == 50
    x = (np.random.default_rng(13).standard_normal((int(lengths.sum()), nch)) * 0.3).astype(np.float32)
    packed, table = torch.from_numpy(x).cuda(), plan.to_device("cuda")
    buf = torch.full((16 + K.N * R + 16, nch), 123.0, dtype=torch.float32, device="cuda")
    rows = buf[16:16 + K.N * R].view(K.N, R, nch)
    F.tracks_stage_device(packed, table, fs, fo, R, out=rows)
    ref = torch.full((K.N, R, nch), 321.0, dtype=torch.float32, device="cuda")
    F.tracks_stage_device(packed, table[:K.SLICE].contiguous(), fs, fo, R, out=ref[:K.SLICE])
    F.tracks_stage_device(packed, table[K.SLICE:].contiguous(), fs, fo, R, out=ref[K.SLICE:])
    torch.cuda.synchronize()
    assert torch.equal(rows.view(torch.int32), ref.view(torch.int32))
    assert bool((buf[:16] == 123.0).all()) and bool((buf[-16:] == 123.0).all()) and torch.equal(packed, torch.from_numpy(x).cuda())
    got = rows.cpu().numpy()
    for t in SUB:
        a, n = int(tab[t, 0]), int(lengths[t])
        want = todays_row(x[a:a + n], fs, fo)
        assert want.shape[0] == n + (100 if n > 64 else 0)
        assert np.array_equal(got[t, :want.shape[0]].view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), t
        assert not got[t, want.shape[0]:].view(np.uint32).any(), t
    assert np.abs(got[K.SLICE, :50]).max() > 0 and np.abs(got[K.N - 1, 50 + 69:50 + 69 + 50]).max() > 0   # extensions behind the seam


# ------------------------------------------------------------------------------------------- the chunk loops of the meter

@pytest.mark.parametrize("ns", [64, 65, 129, 300])
def test_gate_groups_over_chunks_of_64_streams(ns):
    zs, group, ng = K.gate_groups_case(ns)
    rows, nb = K.rows_of(zs)
    for th in (S.gate_thresholds(), S.gate_thresholds(-30.0, -3.0)):
        want = S.gate_groups(zs, group, ng, *th)
        assert K.same(K.groups_call(rows, nb, group, ng, *th), want), th
    assert not K.bits(want[3]).any() and (want[[0, 1, 2, 4], 3] > 0).all() and np.isnan(zs[2]).any()
    if ns == 300:
        assert set(np.flatnonzero(group == 2) // 64) == {0, 4} and all(want[g, 3] > want[g, 1] > 0 for g in (0, 1, 2, 4))


def test_gate_and_range_over_300_scattered_groups():
    zs, group, ng = K.scattered_groups_case(700)
    rows, nb = K.rows_of(zs)
    want = S.gate_groups(zs, group, ng)
    assert K.same(K.groups_call(rows, nb, group, ng, *S.gate_thresholds()), want) and (want[:, 3] > want[:, 1]).sum() > 200
    want = S.range_groups(zs, group, ng)
    assert K.same(K.groups_call(rows, nb, group, ng, *S.gate_thresholds(-70.0, -20.0), percentiles=(10, 95)), want)
    assert ((want[:, 2] >= 2) & (want[:, 0] != want[:, 1])).sum() > 250


def test_300_one_stream_groups_have_the_bits_of_the_stream_gate_kernel():
    e, hops = K.hop_energies()
    d_e, d_h = torch.from_numpy(e[K.SLICE - 297:]).cuda(), torch.from_numpy(hops[K.SLICE - 297:].astype(np.int64)).cuda()
    want = F.loudness_gate_device(d_e, K.HOP, hops=d_h, weights=K.WEIGHTS.tolist())
    blocks, nblocks, _ = F.loudness_blocks_device(d_e, K.HOP, 4, 1, hops=d_h, weights=K.WEIGHTS.tolist())
    got = F.loudness_gate_groups_device(blocks, nblocks, torch.arange(300, dtype=torch.int32, device="cuda"), 300)
    assert tuple(got.shape) == (300, 4) and torch.equal(got.view(torch.int64), want.view(torch.int64))
    assert np.array_equal(K.bits(want.cpu().numpy()), K.bits(K.gate_model()[K.SLICE - 297:])) and int((got[:, 3] > got[:, 1]).sum()) > 5 and int((got[:, 3] == 0).sum()) > 5


@pytest.mark.parametrize("ns", [256, 257, 513, 700])
def test_range_groups_over_chunks_of_256_streams(ns):
    zs, group, ng = K.range_case(ns)
    rows, nb = K.rows_of(zs)
    for low, high in K.PCTS:
        want = S.range_groups(zs, group, ng, *K.RANGE_GATE, low=low, high=high)
        assert K.same(K.groups_call(rows, nb, group, ng, *K.RANGE_GATE, percentiles=(low, high)), want), (low, high)
        for g in [0, 1] + ([2] if ns > 512 else []):
            assert want[g, 2] >= 2 and (want[g, 0] != want[g, 1] or low == high), g
    assert nb[0] == 0 and nb[255] == 0 and nb[101] == 3000 and nb[ns - 1] == 0 and want[1, 2] > 3000 and want[3, 2] == 0
    if ns > 512:
        assert {int(s) // 256 for s in np.flatnonzero(group == 0)} == {0, 2} and nb[512] == 0


@pytest.mark.parametrize("name", ["duplicates", "lowest byte", "spread"])
def test_range_select_on_hard_multisets_over_three_chunks(name):
    values, a, r = K.hard_multisets()[name]
    zs, group, ng = K.over_three_chunks(values)
    rows, nb = K.rows_of(zs)
    for low, high in K.PCTS:
        want = S.range_groups(zs, group, ng, a, r, low=low, high=high)
        assert K.same(K.groups_call(rows, nb, group, ng, a, r, percentiles=(low, high)), want), (low, high)
        assert want[0, 2] == len(values) and (name == "duplicates" or low == high or want[0, 0] != want[0, 1])


# ------------------------------------------------------------------------------------------------------------- the 2^22 seams

def test_gate_groups_past_2_22_streams():
    """launch_streams: 2^22 + 3 streams of at most one block in 64 groups.  The reference is the vectorised restatement of the
    model for one-block streams, which the host module holds to the model and the host twin to it"""
    rows, nb, group = K.big_streams_case()
    th = S.gate_thresholds()
    want = K.gate_groups_one_block(rows, nb, group, 64, *th)
    t0 = time.perf_counter()
    got = K.groups_call(rows, nb, group, 64, *th)
    print("gate over 2^22 + 3 streams: %.2f s with the copies" % (time.perf_counter() - t0))
    assert np.array_equal(K.bits(got), K.bits(want))
    assert (want[:, 3] > want[:, 1]).all() and (want[:, 1] > 0).all() and rows[K.GRID_X, 0] != rows[0, 0] and (group >= 64).any()
    short = K.gate_groups_one_block(rows[:K.GRID_X], nb[:K.GRID_X], group[:K.GRID_X], 64, *th)
    assert not np.array_equal(short[group[K.GRID_X]], want[group[K.GRID_X]])     # the streams behind the seam count


def test_gate_and_range_past_2_22_groups():
    """launch_sums and the group loop of the range call: 3 streams in groups 0, 2^22 - 1 and 2^22 of 2^22 + 1; every other row
    must be the empty group's"""
    zs, group = K.big_groups_case()
    rows, nb = K.rows_of(zs)
    want = K.big_groups_model()
    t0 = time.perf_counter()
    got = K.groups_call(rows, nb, group, K.NG_BIG, *S.gate_thresholds())
    t1 = time.perf_counter()
    assert K.same(got, want) and all(want[g, 3] > want[g, 1] > 0 for g in group) and len({want[g, 0] for g in group}) == 3
    want = K.big_groups_model((10, 95))
    t2 = time.perf_counter()
    got = K.groups_call(rows, nb, group, K.NG_BIG, *S.gate_thresholds(-70.0, -20.0), percentiles=(10, 95))
    print("2^22 + 1 groups: gate %.2f s, range %.2f s with the copies" % (t1 - t0, time.perf_counter() - t2))
    assert K.same(got, want) and all(want[g, 2] >= 2 and want[g, 0] != want[g, 1] for g in group)
