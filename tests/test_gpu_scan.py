"""The packed meter calls on the device (RRX_tracks_true_peak_packed_device / RRX_tracks_loudness_packed_device; true_peak.hip,
loudness.hip) over the case table of scan_cases.py: against their host twins, against the row forms -- the existing kernels -- on
float64 rows that hold the exact conversion, past the grid.y split, on sources at odd byte offsets, and scan_tracks_pcm on top."""
import numpy as np
import pytest
import torch

import foo_dsp_resampler_amd as F
import scan_cases as S

pytestmark = pytest.mark.gpu


def bits(t):
    return t.contiguous().view(torch.int64).cpu().numpy().view(np.uint64)


def rows_of(exact, table, nch, dtype):
    """rows [ntracks, max frames, nch] of `dtype` holding the tracks from frame 0 on, zeros behind them, on the device"""
    most = max(int(table[:, 1].max()), 1)
    rows = np.zeros((table.shape[0], most, nch), dtype)
    for t, e in enumerate(table):
        rows[t, :int(e[1])] = exact[int(e[0]):int(e[0]) + int(e[1])]
    return torch.from_numpy(rows).cuda()


def d_table(table):
    return torch.from_numpy(np.ascontiguousarray(table).view(np.int64)).cuda()


def d_gain(gain):
    return None if gain is None else torch.from_numpy(gain).cuda()


def filter_of(coefs):
    return (coefs.shape[0], coefs.shape[1], coefs.reshape(-1))


@pytest.mark.parametrize("nch", [1, 2, 3])
@pytest.mark.parametrize("kind", list(S.KINDS))
def test_true_peak_equals_the_host_twin_and_the_row_form(kind, nch):
    for name, coefs in S.FILTERS.items():
        lens = S.lengths(coefs.shape[1])
        raw, exact = S.source(kind, lens, nch, 10 * nch + len(name))
        table = S.table_of(lens)
        packed, tab = torch.from_numpy(raw).cuda(), d_table(table)
        rows64 = rows_of(exact, table, nch, np.float64)
        for gain in (None, S.gains(len(lens))):
            rc, want_tp, want_pk = S.host_true_peak(kind, raw, table, nch, max(lens), gain, coefs)
            assert rc == S.RR_OK
            tp, pk = F.tracks_true_peak_packed_device(packed, tab, gain=d_gain(gain), filter=filter_of(coefs), max_frames=max(lens))
            assert np.array_equal(bits(tp), want_tp) and np.array_equal(bits(pk), want_pk), (name, gain is not None)
            rtp, rpk = F.tracks_true_peak_device(rows64, tab, gain=d_gain(gain), filter=filter_of(coefs))
            assert torch.equal(tp.view(torch.int64), rtp.view(torch.int64)) and torch.equal(pk.view(torch.int64), rpk.view(torch.int64)), name
            if kind == "f32":  # the float32 packed form against the row form on float32 rows
                ftp, fpk = F.tracks_true_peak_device(rows_of(exact, table, nch, np.float32), tab, gain=d_gain(gain), filter=filter_of(coefs))
                assert torch.equal(tp.view(torch.int64), ftp.view(torch.int64)) and torch.equal(pk.view(torch.int64), fpk.view(torch.int64)), name


@pytest.mark.parametrize("hop", S.HOPS)
@pytest.mark.parametrize("nch", [1, 2, 3])
@pytest.mark.parametrize("kind", list(S.KINDS))
def test_loudness_equals_the_host_twin_and_the_row_form(kind, nch, hop):
    lens = S.hop_lengths(hop)
    raw, exact = S.source(kind, lens, nch, 100 * nch + hop)
    table = S.table_of(lens)
    packed, tab = torch.from_numpy(raw).cuda(), d_table(table)
    rows64 = rows_of(exact, table, nch, np.float64)
    stride = max(lens) // hop
    for gain in (None, S.gains(len(lens))):
        rc, want_e, want_h = S.host_loudness(kind, raw, table, nch, max(lens), hop, gain)
        assert rc == S.RR_OK
        energy = torch.full((len(lens), nch, stride), S.GUARD, dtype=torch.float64, device="cuda")
        e, hops = F.tracks_loudness_packed_device(packed, tab, gain=d_gain(gain), coefs=S.KW48, hop=hop, max_frames=max(lens), energy=energy)
        assert e is energy and list(hops.cpu().numpy()) == list(want_h) == [0, 4, 4, 0, 1531 // hop]
        assert np.array_equal(bits(e), want_e.view(np.uint64)), gain is not None  # GUARD beyond every track's hops included
        renergy = torch.full((len(lens), nch, stride), S.GUARD, dtype=torch.float64, device="cuda")
        re, rhops = F.tracks_loudness_device(rows64, tab, gain=d_gain(gain), coefs=S.KW48, hop=hop, energy=renergy)
        assert torch.equal(hops, rhops) and torch.equal(e.view(torch.int64), re.view(torch.int64))
        if kind == "f32":
            fenergy = torch.full((len(lens), nch, stride), S.GUARD, dtype=torch.float64, device="cuda")
            fe, fhops = F.tracks_loudness_device(rows_of(exact, table, nch, np.float32), tab, gain=d_gain(gain), coefs=S.KW48, hop=hop, energy=fenergy)
            assert torch.equal(hops, fhops) and torch.equal(e.view(torch.int64), fe.view(torch.int64))


@pytest.mark.parametrize("kind", list(S.KINDS))
def test_the_direct_form_with_342_channels(kind):
    """nch * taps = 342 * 12 > kTpLdsDoubles: no tile fits, the kernel reads its taps from the source"""
    nch, lens = 342, [20, 0, 7]
    assert nch * 12 > S.lds_doubles() >= (nch - 1) * 12
    raw, exact = S.source(kind, lens, nch, 5)
    table = S.table_of(lens)
    gain = S.gains(3)
    rc, want_tp, want_pk = S.host_true_peak(kind, raw, table, nch, 20, gain)
    assert rc == S.RR_OK
    tp, pk = F.tracks_true_peak_packed_device(torch.from_numpy(raw).cuda(), d_table(table), gain=d_gain(gain), max_frames=20)
    assert np.array_equal(bits(tp), want_tp) and np.array_equal(bits(pk), want_pk)
    rtp, rpk = F.tracks_true_peak_device(rows_of(exact, table, nch, np.float64), d_table(table), gain=d_gain(gain))
    assert torch.equal(tp.view(torch.int64), rtp.view(torch.int64)) and torch.equal(pk.view(torch.int64), rpk.view(torch.int64))


def test_non_finite_float32_samples_give_the_row_forms_bit_patterns():
    nch, lens, hop = 3, [300, 40, 2100], 16
    rng = np.random.default_rng(8)
    x = (rng.standard_normal((sum(lens), nch)) * 0.5).astype(np.float32)
    x[150, 1], x[310, 0], x[320, 2], x[2000, 1] = np.nan, np.inf, -np.inf, -np.nan
    table = S.table_of(lens)
    packed, tab, rows = torch.from_numpy(x).cuda(), d_table(table), rows_of(x, table, nch, np.float32)
    tp, pk = F.tracks_true_peak_packed_device(packed, tab, max_frames=max(lens))
    rtp, rpk = F.tracks_true_peak_device(rows, tab)
    assert torch.equal(tp.view(torch.int64), rtp.view(torch.int64)) and torch.equal(pk.view(torch.int64), rpk.view(torch.int64))
    assert torch.isnan(tp[0, 1]) and torch.isnan(pk[0, 1]) and torch.isinf(pk[1, 0]) and torch.isinf(pk[1, 2]) and torch.isfinite(tp[0, 0])
    e, hops = F.tracks_loudness_packed_device(packed, tab, coefs=S.KW48, hop=hop, max_frames=max(lens))
    re, rhops = F.tracks_loudness_device(rows, tab, coefs=S.KW48, hop=hop)
    assert torch.equal(hops, rhops) and torch.equal(e.view(torch.int64), re.view(torch.int64))
    assert torch.isnan(e[0, 1]).any() and torch.isfinite(e[0, 0]).all()


def many_tracks():
    """32768 + 3 tracks of 0 to 5 frames: one more launch than grid.y holds"""
    n, nch = 32768 + 3, 2
    lens = [(t * 7 + 3) % 6 for t in range(n)]
    assert sorted(set(lens[-3:])) != [0] and max(lens) == 5
    raw, exact = S.source("s16", lens, nch, 77)
    return n, nch, lens, raw, exact, S.table_of(lens)


def test_true_peak_past_the_grid_split():
    n, nch, lens, raw, exact, table = many_tracks()
    rc, want_tp, want_pk = S.host_true_peak("s16", raw, table, nch, 5)
    assert rc == S.RR_OK
    tp, pk = F.tracks_true_peak_packed_device(torch.from_numpy(raw).cuda(), d_table(table), max_frames=5)
    assert np.array_equal(bits(tp), want_tp) and np.array_equal(bits(pk), want_pk)
    ref_tp, ref_pk = S.ref_true_peak(exact, S.cuts_of(table, raw.shape[0], 5)[-3:], nch)  # the last three, by the one-stream call
    assert np.array_equal(bits(tp)[-3:], ref_tp) and np.array_equal(bits(pk)[-3:], ref_pk) and ref_pk.any()


def test_loudness_past_the_grid_split():
    n, nch, lens, raw, exact, table = many_tracks()
    rc, want_e, want_h = S.host_loudness("s16", raw, table, nch, 5, 2)
    assert rc == S.RR_OK
    energy = torch.full((n, nch, 2), S.GUARD, dtype=torch.float64, device="cuda")
    e, hops = F.tracks_loudness_packed_device(torch.from_numpy(raw).cuda(), d_table(table), coefs=S.KW48, hop=2, max_frames=5, energy=energy)
    assert np.array_equal(hops.cpu().numpy().astype(np.uint64), want_h) and list(want_h[-3:]) == [v // 2 for v in lens[-3:]]
    assert np.array_equal(bits(e), want_e.view(np.uint64))
    ref_e, _ = S.ref_loudness(exact, S.cuts_of(table, raw.shape[0], 5)[-3:], nch, 2, 2)
    assert np.array_equal(bits(e)[-3:], ref_e.view(np.uint64))


@pytest.mark.parametrize("off", [1, 2, 3])
def test_s24_source_at_odd_byte_offsets_inside_a_larger_allocation(off):
    """the source is a view `off` bytes into an allocation filled with 0x7F: read as samples, those bytes are close to full scale
    and would raise every peak of these quiet tracks"""
    nch, hop, lens = 1, 16, [0, 1, 10, 2037, 70, 333]
    rng = np.random.default_rng(off)
    raw, exact = S.store("s24", rng.integers(-(1 << 12), 1 << 12, size=(sum(lens), nch)))
    table = S.table_of(lens)
    big = torch.full((raw.size + 64,), 0x7F, dtype=torch.uint8, device="cuda")
    view = big[off:off + raw.size].view(raw.shape)
    view.copy_(torch.from_numpy(raw).cuda())
    assert view.data_ptr() % 4 == off and view.is_contiguous()
    rc, want_tp, want_pk = S.host_true_peak("s24", raw, table, nch, max(lens))
    tp, pk = F.tracks_true_peak_packed_device(view, d_table(table), max_frames=max(lens))
    assert rc == S.RR_OK and np.array_equal(bits(tp), want_tp) and np.array_equal(bits(pk), want_pk)
    assert 0.0 < float(pk.max()) <= 2.0 ** -11
    rc, want_e, want_h = S.host_loudness("s24", raw, table, nch, max(lens), hop)
    e, hops = F.tracks_loudness_packed_device(view, d_table(table), coefs=S.KW48, hop=hop, max_frames=max(lens))
    assert rc == S.RR_OK and np.array_equal(hops.cpu().numpy().astype(np.uint64), want_h)
    want_e[want_e == S.GUARD] = 0.0  # (the call's own energy tensor is zeroed, not guarded)
    assert np.array_equal(bits(e), want_e.view(np.uint64))
    assert bool((big[:off] == 0x7F).all()) and bool((big[off + raw.size:] == 0x7F).all())


def test_scan_tracks_pcm_on_three_s16_tracks():
    rate, nch, hop = 48000, 2, 4800
    rng = np.random.default_rng(1)
    n = np.arange(2 * rate)
    sine = np.zeros((n.size, nch), np.int64)
    sine[:, 0] = np.rint(32767 * np.sin(2 * np.pi * 997.0 * n / rate)).astype(np.int64)  # full scale on the left, silence on the right
    others = [np.rint(rng.standard_normal((rate + 123, nch)) * 3000).astype(np.int64), np.rint(rng.standard_normal((70001, nch)) * 900).astype(np.int64)]
    stored = [S.store("s16", v) for v in [sine] + others]
    tracks = [torch.from_numpy(raw).cuda() for raw, _ in stored]
    album = [0, 1, 1]
    out = F.scan_tracks_pcm(tracks, rate, album=album)
    assert tuple(out["true_peak"].shape) == (3, nch) and tuple(out["peak"].shape) == (3, nch) and tuple(out["integrated"].shape) == (3,)

    lens = [raw.shape[0] for raw, _ in stored]
    table = S.table_of(lens)
    exact = np.concatenate([ex for _, ex in stored])
    rows64, tab = rows_of(exact, table, nch, np.float64), d_table(table)
    rtp, rpk = F.tracks_true_peak_device(rows64, tab)
    energy, hops = F.tracks_loudness_device(rows64, tab, rate=rate)
    want = F.loudness_meter_device(energy, hop, hops, None, album, 2)
    assert set(want) <= set(out) and {"integrated", "momentary_max", "short_term_max", "range", "group_integrated", "group_range"} <= set(want)
    for key, value in want.items():
        assert torch.equal(out[key].view(torch.int64), value.view(torch.int64)), key
    assert torch.equal(out["true_peak"].view(torch.int64), rtp.view(torch.int64)) and torch.equal(out["peak"].view(torch.int64), rpk.view(torch.int64))
    assert torch.equal(out["group_true_peak"], torch.stack([rtp[0].max(), rtp[1:].max()]))
    assert torch.equal(out["group_peak"], torch.stack([rpk[0].max(), rpk[1:].max()]))
    assert torch.equal(out["track_gain_db"], -18.0 - want["integrated"]) and torch.equal(out["album_gain_db"], -18.0 - want["group_integrated"])
    lufs = out["integrated"].cpu().numpy()
    print("integrated %r, true peak %r" % (lufs.tolist(), out["true_peak"].cpu().numpy().tolist()))
    assert abs(lufs[0] - -3.01) <= 0.1  # BS.1770's calibration: a full-scale 997 Hz sine on one channel
    assert float(out["peak"][0, 0]) == 32767 / 32768 and float(out["peak"][0, 1]) == 0.0
    assert abs(float(out["group_integrated"][0]) - lufs[0]) < 1e-9 and lufs[2] < float(out["group_integrated"][1]) < lufs[1]
