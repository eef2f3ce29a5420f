"""The host side of tests/test_gpu_stream_seams.py: the inputs of seam_cases.py at 32768 + 3 streams or tracks, at several chunks
of the group kernels and at 2^22 + 3 streams / 2^22 + 1 groups, through the host twins (RRX_debug_*_host) against the numpy models.
The device tests compare with the models over all streams where a model is vectorised or its loop is short, and lean on a twin or
on a vectorised restatement where it is not; every twin and restatement they lean on is held to its model here, with the same
inputs, on the streams around the seam and about 50 more.  The conditions that keep those tests from passing emptily -- the two
sides of the seam differ, the statistics are alive on both, every group gates something -- are asserted on the models here and
again there.  CPU only; the twins are plain loops."""
import numpy as np
import pytest

import foo_dsp_resampler_amd as F
import loudness_stats_model as S
import seam_cases as K

SUB = K.subset()


def test_the_subset_lies_around_the_seam():
    assert {0, 1, K.SLICE - 2, K.SLICE - 1, K.SLICE, K.SLICE + 1, K.N - 1} <= set(SUB) and 50 <= len(SUB) <= 57 and K.N == 32771


@pytest.mark.parametrize("key", list(K.FINISH))
def test_finish_twin_equals_the_model(key):
    got, want = K.finish_call(key, False), K.finish_model(key, SUB)
    for g, w in zip(got, want):
        assert (g is None) == (w is None) and (g is None or np.array_equal(g[SUB], w))
    assert K.two_sides_differ(K.finish_input(key), K.gains(), got[1]) and K.live_on_both_sides(got[2] - K.CLIPPED0)
    assert K.live_on_both_sides(got[1] > K.PEAK0) and (got[1] > K.PEAK0).mean() > 0.9


@pytest.mark.parametrize("key", list(K.SHAPED))
def test_shaped_twin_equals_the_model(key):
    got, want = K.shaped_call(key, False), K.shaped_model(key, SUB)
    for g, w in zip(got, want):
        assert np.array_equal(np.ascontiguousarray(g[SUB]).view(np.uint8), np.ascontiguousarray(w).view(np.uint8))
    x, st = K.shaped_input(key)
    assert K.two_sides_differ(x, st, got[0], got[3]) and K.live_on_both_sides(got[2] - K.CLIPPED0)


@pytest.mark.parametrize("key", list(K.TRUE_PEAK))
def test_true_peak_twin_equals_the_model(key):
    got, want = K.tp_call(key, False), K.tp_model(key, SUB)
    assert np.array_equal(got[0][SUB], np.maximum(want[0], K.PEAK0)) and np.array_equal(got[1][SUB], np.maximum(want[1], K.PEAK0))
    if got[2] is not None:
        assert np.array_equal(K.bits(got[2][SUB]), K.bits(want[2]))
    assert K.two_sides_differ(K.tp_input(key)[0], got[0], got[1])


@pytest.mark.parametrize("double", [False, True], ids=["f32", "f64"])
def test_loudness_twin_equals_the_model(double):
    (e, so), (we, ws) = K.loudness_call(double, False), K.loudness_model(double)
    assert np.array_equal(K.bits(e[:, :, 1:1 + K.L_HOPS]), K.bits(we)) and np.array_equal(K.bits(so), K.bits(ws))
    assert (e[:, :, 0] == K.GUARD).all() and (e[:, :, 1 + K.L_HOPS:] == K.GUARD).all()
    x, st = K.loudness_input(double)
    assert K.two_sides_differ(x, st, we, ws) and (we > 0).all()


def test_gate_and_blocks_twins_equal_the_models():
    got, want = K.gate_call(False), K.gate_model()
    assert np.array_equal(K.bits(got), K.bits(want))
    e, hops = K.hop_energies()
    assert K.two_sides_differ(e, hops, want[:, 2:]) and hops[K.SLICE] != hops[0]
    assert (want[:K.SLICE, 3] > want[:K.SLICE, 1]).any() and (want[:K.SLICE, 1] > 0).any() and (want[:K.SLICE, 3] == 0).any()
    assert want[K.SLICE, 3] == 0 and want[K.SLICE + 1, 3] == 1 and want[K.N - 1, 3] == 2 and want[K.N - 1, 1] == 1   # behind the seam
    for L, P in K.BLOCK_SHAPES:
        (b, nb, mx), (wb, wn, wm) = K.blocks_call(L, P, False), K.blocks_model(L, P)
        assert np.array_equal(K.bits(b), K.bits(wb)) and np.array_equal(nb, wn) and np.array_equal(K.bits(mx), K.bits(wm))
        _, nb, mx = K.blocks_call(L, P, False, blocks=False)
        assert np.array_equal(nb, wn) and np.array_equal(K.bits(mx), K.bits(wm))
        assert K.live_on_both_sides(wn) and K.live_on_both_sides(wn == 0) and K.two_sides_differ(K.block_hops())
        assert wm[K.N - 1] > 0 and wm[K.N - 1] != wm[K.N - 1 - K.SLICE] and wn[K.N - 1] != wn[K.N - 1 - K.SLICE]


def test_track_table_and_rows():
    tab, total = K.track_table()
    assert K.two_sides_differ(tab[:, 3], tab[:, 4], tab[:, 5], K.track_rows(False))
    assert set(tab[:, 3].tolist()) == {0, 1, 2, 3} and set(tab[:, 4].tolist()) == set(range(6)) and int((tab[:, 3] + tab[:, 4]).max()) == K.ROW
    assert total == int(tab[-1, 5] + tab[-1, 4]) and sum(n for _, n in K.WINDOWS) == K.ROW


@pytest.mark.parametrize("double,fmt", [(False, F.RRX_FMT_S16), (True, F.RRX_FMT_S24_3)])
def test_the_models_on_padded_slices_equal_the_models_on_each_tracks_own_slice(double, fmt):
    """the references of the per-track device tests are the uniform models on slices padded with +0.0 to 5 frames; on the subset
    they must be the models of the one-stream calls the per-track forms are defined as, on each track's own frames"""
    tab, _ = K.track_table()
    x, g, nb = K.track_rows(double), K.gains(), K.FM.NBYTES[fmt] * K.T_NCH
    raw, pk, cl = K.tracks_finish_model(double, fmt)
    tp, tpk = K.tracks_true_peak_model(double)
    e, hops = K.tracks_loudness_model(double)
    for t in SUB:
        of, n, a = int(tab[t, 3]), int(tab[t, 4]), int(tab[t, 5]) * nb
        if not n:                                    # an empty track: no bytes, statistics and energies untouched
            assert (pk[t] == K.PEAK0).all() and (cl[t] == K.CLIPPED0).all() and not tp[t].any() and not tpk[t].any() and hops[t] == 0, t
            continue
        sl = np.ascontiguousarray(x[t:t + 1, of:of + n])
        o, p, c = K.FM.model(sl, fmt, g[t:t + 1], True, K.stream_seed(t, K.T_NCH), 0, np.full((1, K.T_NCH), K.PEAK0, np.uint64),
                             np.full((1, K.T_NCH), K.CLIPPED0, np.uint64))
        assert np.array_equal(raw[a:a + n * nb], o.reshape(-1)) and np.array_equal(pk[t], p[0]) and np.array_equal(cl[t], c[0]), t
        wtp, wpk, _ = K.TM.true_peak(sl, K.TM.BS1770, g[t:t + 1], True, None)
        assert K.same(tp[t].view(np.float64), wtp[0].view(np.float64)) and np.array_equal(tpk[t], wpk[0]), t
        with np.errstate(invalid="ignore"):
            we, _ = K.LM.hop_energies(K.LM.gained(sl, g[t:t + 1]), K.LM.K48, K.T_HOP)
        assert hops[t] == n // K.T_HOP == we.shape[2] and K.same(e[t, :, :we.shape[2]], we[0]), t


@pytest.mark.parametrize("double,fmt,order", [(False, F.RRX_FMT_S16, 9), (True, F.RRX_FMT_S24_3, 4)])
def test_shaped_window_twin_equals_the_model_per_track(double, fmt, order):
    """the twin of the window form over two windows, which the device test takes the state of every track from: bytes and
    statistics against the model over all tracks, and on the subset bytes, statistics and state against shaped_model.model on each
    track's own slice"""
    raw, pk, cl, st = K.tracks_finish_call(double, fmt, "shaped-windows", order, on_device=False)
    wraw, wpk, wcl = K.tracks_shaped_model(double, fmt, order)
    assert np.array_equal(raw, wraw) and np.array_equal(pk, wpk) and np.array_equal(cl, wcl)
    tab, _ = K.track_table()
    nb = K.FM.NBYTES[fmt] * K.T_NCH
    parts, spk, scl, sst = K.tracks_shaped_model(double, fmt, order, SUB)
    for i, t in enumerate(SUB):
        a = int(tab[t, 5]) * nb
        assert np.array_equal(raw[a:a + int(tab[t, 4]) * nb], parts[i]), t
    assert np.array_equal(pk[SUB], spk) and np.array_equal(cl[SUB], scl) and np.array_equal(K.bits(st[SUB]), K.bits(sst))
    assert K.two_sides_differ(st[:, :, :order]) and K.live_on_both_sides(cl - K.CLIPPED0)


# ------------------------------------------------------------------------------------------------------- the group kernels

def check_gate_conditions(results, populated):
    """every populated group has N1 > N2 > 0 in one case at least"""
    for g in populated:
        assert any(r[g, 3] > r[g, 1] > 0 for r in results), g


def test_gate_group_cases_gate_something_and_the_twin_equals_the_model():
    results = []
    for ns in (64, 65, 129, 300):
        zs, group, ng = K.gate_groups_case(ns)
        rows, nb = K.rows_of(zs)
        for th in (S.gate_thresholds(), S.gate_thresholds(-30.0, -3.0)):
            want = S.gate_groups(zs, group, ng, *th)
            assert K.same(K.groups_call(rows, nb, group, ng, *th, on_device=False), want)
            results.append(want)
        assert not K.bits(want[3]).any() and set(np.unique(group)) >= {-1, 0, 1, 2, 4, 5} and nb.max() > 64 > nb[nb < 64].max()
        last = (ns - 1) // 64 * 64
        assert (np.flatnonzero(group == 1) >= last).all() and all((group[a:a + 64] == 0).any() for a in range(0, ns - 1, 64))
    chunks = set(np.flatnonzero(group == 2) // 64)
    assert chunks == {0, 4}                          # (300 streams: nothing of group 2 in chunks 1 to 3)
    check_gate_conditions(results, (0, 1, 2, 4))
    zs, group, ng = K.scattered_groups_case(700)
    want = S.gate_groups(zs, group, ng)
    rows, nb = K.rows_of(zs)
    assert K.same(K.groups_call(rows, nb, group, ng, *S.gate_thresholds(), on_device=False), want)
    assert set(np.bincount(group).tolist()) == {2, 3} and (want[:, 3] > want[:, 1]).sum() > 200


def test_range_cases_select_something_and_the_twin_equals_the_model():
    for ns in (256, 257, 513, 700):
        zs, group, ng = K.range_case(ns)
        rows, nb = K.rows_of(zs)
        for low, high in K.PCTS:
            want = S.range_groups(zs, group, ng, *K.RANGE_GATE, low=low, high=high)
            assert K.same(K.groups_call(rows, nb, group, ng, *K.RANGE_GATE, percentiles=(low, high), on_device=False), want)
            for g in [0, 1] + ([2] if ns > 512 else []):
                assert want[g, 2] >= 2 and (want[g, 0] != want[g, 1] or low == high), (ns, g)
            assert want[3, 2] == 0
        assert nb[0] == 0 and nb[255] == 0 and nb[101] == 3000 and nb[ns - 1] == 0
    assert {int(s) // 256 for s in np.flatnonzero(group == 0)} == {0, 2} and nb[512] == 0
    for name, (values, a, r) in K.hard_multisets().items():
        zs, group, ng = K.over_three_chunks(values)
        rows, nb = K.rows_of(zs)
        for low, high in K.PCTS:
            want = S.range_groups(zs, group, ng, a, r, low=low, high=high)
            assert K.same(K.groups_call(rows, nb, group, ng, a, r, percentiles=(low, high), on_device=False), want), name
            assert want[0, 2] == len(values) and (name == "duplicates" or low == high or want[0, 0] != want[0, 1])
    zs, group, ng = K.scattered_groups_case(700)
    rows, nb = K.rows_of(zs)
    want = S.range_groups(zs, group, ng)
    assert K.same(K.groups_call(rows, nb, group, ng, *S.gate_thresholds(-70.0, -20.0), percentiles=(10, 95), on_device=False), want)
    assert ((want[:, 2] >= 2) & (want[:, 0] != want[:, 1])).sum() > 250


# ------------------------------------------------------------------------------------------------------------- the 2^22 seams

def test_the_one_block_restatement_equals_the_model_and_the_twin_equals_it_at_size():
    rows, nb, group = K.big_streams_case()
    th = S.gate_thresholds()
    for part in (slice(0, 700), slice(K.GRID_X - 350, K.GRID_X + 3)):
        zs = [rows[s, :int(nb[s])] for s in range(part.start, part.stop)]
        assert np.array_equal(K.bits(K.gate_groups_one_block(rows[part], nb[part], group[part], 64, *th)), K.bits(S.gate_groups(zs, group[part], 64, *th)))
    want = K.gate_groups_one_block(rows, nb, group, 64, *th)
    assert np.array_equal(K.bits(K.groups_call(rows, nb, group, 64, *th, on_device=False)), K.bits(want))
    assert (want[:, 3] > want[:, 1]).all() and (want[:, 1] > 0).all() and (want[:, 3] < np.bincount(group, minlength=67)[:64]).all()
    assert rows[K.GRID_X, 0] != rows[0, 0] and rows[K.GRID_X + 1, 0] != rows[1, 0] and (group >= 64).any()
    # the streams behind the seam count: without them group 0's sums are others
    short = K.gate_groups_one_block(rows[:K.GRID_X], nb[:K.GRID_X], group[:K.GRID_X], 64, *th)
    assert group[K.GRID_X] < 64 and nb[K.GRID_X] == 1 and not np.array_equal(short[group[K.GRID_X]], want[group[K.GRID_X]])


def test_twins_over_2_22_groups_equal_the_model():
    zs, group = K.big_groups_case()
    rows, nb = K.rows_of(zs)
    want = K.big_groups_model()
    assert K.same(K.groups_call(rows, nb, group, K.NG_BIG, *S.gate_thresholds(), on_device=False), want)
    assert all(want[g, 3] > want[g, 1] > 0 for g in group) and len({want[g, 0] for g in group}) == 3
    want = K.big_groups_model((10, 95))
    assert K.same(K.groups_call(rows, nb, group, K.NG_BIG, *S.gate_thresholds(-70.0, -20.0), percentiles=(10, 95), on_device=False), want)
    assert all(want[g, 2] >= 2 and want[g, 0] != want[g, 1] for g in group)
