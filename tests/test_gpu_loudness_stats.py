"""The loudness meter on the device (RRX_loudness_blocks_device / RRX_loudness_gate_groups_device /
RRX_loudness_range_groups_device, loudness_stats.hip) against the numpy restatement of its arithmetic in loudness_stats_model.py, as
bit patterns and with every buffer under guards: blocks across workgroup tiles and clamps, the gate over interleaved, empty and
whole-library groups and its one-stream identity with RRX_loudness_gate_device, the radix select at its pass and tile boundaries,
the meter on the energies of a real track batch, and the album form of the normalising conversion."""
import ctypes as C

import numpy as np
import pytest
import torch

import foo_dsp_resampler_amd as F
import loudness_stats_model as S

pytestmark = pytest.mark.gpu
GUARD = 777.25
NGUARD = 12345
SHAPES = [(1, 1), (4, 1), (30, 1), (30, 10), (3, 2), (5, 7)]
W6 = [1.0, 1.0, 1.0, 0.0, 1.41, 1.41]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """equal bit patterns, or NaN in both: the T of an empty group is 0 / 0, whose sign is the processor's"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def vp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def blocks_device(energy, hop, L, P, hops=None, weights=None, stride=None, blocks=True, nblocks=True, top=True):
    """RRX_loudness_blocks_device through the C ABI on energy [nstreams, nch, nhops] (numpy): (blocks [nstreams, stride] with the
    guard value where nothing was written, nblocks, max) as numpy, None for an output not asked for; all outputs under guards"""
    ns, nch, nh = energy.shape
    stride = max(S.count(nh, L, P), 1) if stride is None else stride
    d_e = dev(energy)
    d_b = torch.full((ns * stride + 3,), GUARD, dtype=torch.float64, device="cuda")
    d_n = torch.full((ns + 2,), NGUARD, dtype=torch.int64, device="cuda")
    d_m = torch.full((ns + 2,), GUARD, dtype=torch.float64, device="cuda")
    d_h, d_w = dev(hops, np.int64), dev(weights, np.float64)
    F.ratelib._ensure_init()
    torch.cuda.synchronize()
    rc = F.lib().RRX_loudness_blocks_device(-1, None, vp(d_e), nh, ns, nch, nh, vp(d_h), vp(d_w), hop, L, P, vp(d_b) if blocks else None,
                                            stride if blocks else 0, vp(d_n) if nblocks else None, vp(d_m) if top else None)
    assert rc == 0
    torch.cuda.synchronize()
    b, n, m = d_b.cpu().numpy(), d_n.cpu().numpy(), d_m.cpu().numpy()
    assert np.all(b[ns * stride:] == GUARD) and np.all(n[ns:] == NGUARD) and np.all(m[ns:] == GUARD)
    if not blocks:
        assert np.all(b == GUARD)
    if not nblocks:
        assert np.all(n == NGUARD)
    if not top:
        assert np.all(m == GUARD)
    return (b[:ns * stride].reshape(ns, stride) if blocks else None, n[:ns].astype(np.uint64) if nblocks else None, m[:ns] if top else None)


def groups_device(rows, nblocks, group, ngroups, abs_threshold, rel_factor, percentiles=None):
    """the gate (percentiles None) or the range call through the C ABI on blocks [nstreams, stride] (numpy): [ngroups, 4]; the
    blocks must come back unchanged, result and work lie under guards"""
    ns, stride = rows.shape
    need = F.lib().RRX_loudness_groups_work_doubles(ns, ngroups)
    d_b = dev(rows)
    d_n, d_g = dev(np.asarray(nblocks, dtype=np.uint64).view(np.int64)), dev(group, np.int32)
    d_w = torch.full((need + 3,), GUARD, dtype=torch.float64, device="cuda")
    d_r = torch.full((ngroups * 4 + 2,), GUARD, dtype=torch.float64, device="cuda")
    F.ratelib._ensure_init()
    torch.cuda.synchronize()
    if percentiles is None:
        rc = F.lib().RRX_loudness_gate_groups_device(-1, None, vp(d_b), stride, ns, vp(d_n), vp(d_g), ngroups, abs_threshold, rel_factor, vp(d_r),
                                                     vp(d_w), need)
    else:
        rc = F.lib().RRX_loudness_range_groups_device(-1, None, vp(d_b), stride, ns, vp(d_n), vp(d_g), ngroups, abs_threshold, rel_factor,
                                                      percentiles[0], percentiles[1], vp(d_r), vp(d_w), need)
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(d_b.cpu().numpy()), bits(rows))
    assert bool((d_w[need:] == GUARD).all()) and bool((d_r[ngroups * 4:] == GUARD).all())
    return d_r[:ngroups * 4].view(ngroups, 4).cpu().numpy()


def energies(nch, seed, ns, nh):
    """hop energies with a quiet stretch the relative gate removes and one under the absolute gate"""
    rng = np.random.default_rng(seed)
    e = rng.uniform(1.0, 50.0, (ns, nch, nh))
    e[:, :, 100:220] *= 0.01
    e[:, :, 250:290] *= 1e-12
    return e


@pytest.mark.parametrize("L,P", SHAPES)
@pytest.mark.parametrize("nch", [1, 2, 6])
def test_blocks_kernel_equals_the_model_bit_for_bit(nch, L, P):
    """one stream per length: the lengths of the host test, 257 and 513 hops, and 257 blocks -- one more than a workgroup's tile"""
    hop = 4800
    hops = [0, L - 1, L, L + 1, L + P - 1, L + P, 300, 601, 257, 513, L + 256 * P]
    e = energies(nch, nch * 100 + L * 10 + P, len(hops), max(hops))
    weights = {1: [1.41], 2: [0.0, 1.41], 6: W6}[nch]
    for w in (None, weights):
        zs, nbs, top = S.blocks(e, hop, L, P, hops=hops, weights=w)
        b, nb, mx = blocks_device(e, hop, L, P, hops=hops, weights=w)
        assert np.array_equal(nb, nbs) and nb[-1] == 257
        assert np.array_equal(bits(b), bits(S.as_rows(zs, b.shape[1], GUARD)))
        assert np.array_equal(bits(mx), bits(top))
    _, nb1, mx1 = blocks_device(e, hop, L, P, hops=hops, weights=weights, blocks=False)  # d_blocks NULL: the maximum alone
    assert np.array_equal(nb1, nbs) and np.array_equal(bits(mx1), bits(top))
    _, _, mx2 = blocks_device(e, hop, L, P, hops=hops, weights=weights, blocks=False, nblocks=False)
    assert np.array_equal(bits(mx2), bits(top))
    b3, nb3, _ = blocks_device(e, hop, L, P, hops=hops, weights=weights, top=False)  # d_max NULL
    assert np.array_equal(bits(b3), bits(b)) and np.array_equal(nb3, nbs)
    zc, nbc, topc = S.blocks(e, hop, L, P, hops=hops, weights=weights, stride=50)  # blocks_stride smaller than nb
    bc, nc, mc = blocks_device(e, hop, L, P, hops=hops, weights=weights, stride=50)
    assert np.array_equal(nc, nbc) and nc.max() == 50
    assert np.array_equal(bits(bc), bits(S.as_rows(zc, 50, GUARD))) and np.array_equal(bits(mc), bits(topc))
    z1, n1, t1 = S.blocks(e, hop, L, P, weights=weights)  # without d_hops: nhops for all
    b1, nn1, m1 = blocks_device(e, hop, L, P, weights=weights)
    assert np.array_equal(nn1, n1) and np.array_equal(bits(b1), bits(S.as_rows(z1, b1.shape[1], GUARD))) and np.array_equal(bits(m1), bits(t1))


def test_blocks_with_a_nan_and_an_infinite_energy():
    e = energies(2, 11, 4, 700)
    e[1, 0, 300] = np.nan    # poisons the blocks it enters, which the maximum skips
    e[2, 1, 520] = np.inf    # +inf is a value: the maximum
    e[3] = 0.0               # silence: +0.0
    for L, P in ((4, 1), (30, 1), (30, 10)):
        zs, nbs, top = S.blocks(e, 4800, L, P)
        b, nb, mx = blocks_device(e, 4800, L, P)
        assert np.array_equal(nb, nbs) and np.array_equal(bits(b), bits(S.as_rows(zs, b.shape[1], GUARD))) and np.array_equal(bits(mx), bits(top))
        assert np.isnan(b[1]).any() and np.isfinite(mx[1]) and mx[1] > 0 and mx[2] == np.inf and bits(mx[3:])[0] == 0


_gate_case = {}


def gate_case():
    """7 streams of 2 channels and unequal length, their (4, 1) blocks from the model, computed once"""
    if not _gate_case:
        e = energies(2, 5, 7, 900)
        e[4, 1, 400] = np.nan
        hops = [900, 5, 300, 601, 517, 3, 258]
        zs, nbs, _ = S.blocks(e, 4800, 4, 1, hops=hops)
        _gate_case.update(e=e, hops=hops, zs=zs, nbs=nbs, rows=S.as_rows(zs, 897, GUARD))
    return _gate_case


@pytest.mark.parametrize("group,ngroups", [([2, 0, -1, 0, 2, 5, 1], 3), ([2, 0, -1, 0, 2, 5, 1], 4), ([0] * 7, 1), (list(range(7)), 7), ([3, 3, 3, 3, 3, 3, 3], 3)],
                         ids=["interleaved", "an-empty-group", "one-group", "own-groups", "nobody"])
def test_gate_over_groups_equals_the_model(group, ngroups):
    c = gate_case()
    for thresholds in (S.gate_thresholds(), S.gate_thresholds(-30.0, -3.0)):
        got = groups_device(c["rows"], c["nbs"], group, ngroups, *thresholds)
        want = S.gate_groups(c["zs"], group, ngroups, *thresholds)
        assert np.array_equal(bits(got), bits(want)), thresholds
    if ngroups == 4:
        assert not bits(got[3]).any()  # {+0.0, 0, +0.0, 0}
    if ngroups == 3 and group[0] == 2:
        assert 0 < got[1, 3] <= c["nbs"][6] and got[0, 3] > 0 and got[2, 3] > got[2, 1] > 0  # group 1 is the last stream alone
    # the same through the blocks kernel's own output, with nblocks beyond the rows read clamped to them
    b, nb, _ = blocks_device(c["e"], 4800, 4, 1, hops=c["hops"])
    big = np.where(nb == 897, np.uint64(2 ** 63), nb)
    assert np.array_equal(bits(groups_device(b, big, group, ngroups, *S.gate_thresholds())), bits(S.gate_groups(c["zs"], group, ngroups)))


def test_one_stream_groups_have_the_bits_of_the_stream_gate_kernel():
    c = gate_case()
    d_e, d_h = dev(c["e"]), dev(c["hops"], np.int64)
    for weights in (None, [0.5, 1.41]):
        want = F.loudness_gate_device(d_e, 4800, hops=d_h, weights=weights)
        blocks, nblocks, _ = F.loudness_blocks_device(d_e, 4800, 4, 1, hops=d_h, weights=weights)
        got = F.loudness_gate_groups_device(blocks, nblocks, torch.arange(7, dtype=torch.int32, device="cuda"), 7)
        assert torch.equal(got.view(torch.int64), want.view(torch.int64))
        assert got[5, 3] == 0 and got[1, 3] == 2 and got[0, 1] > 0


def pooled(values, parts):
    """`values` cut into `parts` streams of unequal length, plus one foreign stream: (rows, nblocks, group)"""
    n = len(values)
    cuts = [0, n] if parts == 1 else [0, n // 5, n // 5 + n // 3, n]
    pieces = [values[a:b] for a, b in zip(cuts, cuts[1:])]
    pieces.insert(1, np.full(40, 1e30))  # in another group: never counted
    stride = max(max(len(p) for p in pieces), 1) + 2
    rows = np.full((len(pieces), stride), GUARD)
    for s, p in enumerate(pieces):
        rows[s, :len(p)] = p
    group = [0] * len(pieces)
    group[1] = 1
    return rows, [len(p) for p in pieces], group


PCTS = [(10, 95), (0, 100), (50, 50), (95, 10)]


def check_range(values, parts, abs_threshold, rel_factor, what):
    rows, nblocks, group = pooled(values, parts)
    zs = [rows[s, :nblocks[s]] for s in range(len(nblocks))]
    for low, high in PCTS:
        got = groups_device(rows, nblocks, group, 2, abs_threshold, rel_factor, percentiles=(low, high))
        want = S.range_groups(zs, group, 2, abs_threshold, rel_factor, low=low, high=high)
        assert same(got, want), (what, parts, low, high)
    return got


@pytest.mark.parametrize("parts", [1, 3])
@pytest.mark.parametrize("n2", [0, 1, 2, 255, 256, 257, 5000])
def test_range_select_equals_sorting(n2, parts):
    rng = np.random.default_rng(n2 + parts)
    got = check_range(rng.uniform(1.0, 2.0, n2), parts, 0.5, 0.1, n2)  # T is a tenth of the mean: every block passes
    assert got[0, 2] == n2 and got[1, 2] == 40
    if not n2:
        assert not bits(got[0, :3]).any()


@pytest.mark.parametrize("parts", [1, 3])
def test_range_select_on_hard_multisets(parts):
    rng = np.random.default_rng(parts)
    dup = np.where(rng.uniform(size=3000) < 0.9, 1.5, rng.uniform(1.0, 2.0, 3000))  # 90 % duplicates of one value
    assert check_range(dup, parts, 0.5, 0.1, "duplicates")[0, 2] == 3000
    low8 = (np.uint64(0x3FF8000000000000) + rng.integers(0, 256, 2000).astype(np.uint64)).view(np.float64)  # the last pass decides
    assert check_range(low8, parts, 0.5, 0.1, "lowest byte")[0, 2] == 2000
    spread = 2.0 ** rng.uniform(-150.0, 150.0, 2000)  # 300 binary orders of magnitude; no relative gate (T = 0)
    assert check_range(spread, parts, 0.0, 0.0, "spread")[0, 2] == 2000
    holed = rng.uniform(1.0, 2.0, 1000)
    holed[::7] = np.nan  # skipped
    assert check_range(holed, parts, 0.5, 0.1, "NaNs")[0, 2] == 1000 - len(holed[::7])
    top = holed.copy()
    top[501] = np.inf  # S1 is +inf: with a negative factor T is -inf and +inf is the largest member
    got = check_range(top, parts, 0.5, -1.0, "+inf")
    assert got[0, 2] == 1000 - len(holed[::7])
    rows, nblocks, group = pooled(top, parts)
    assert groups_device(rows, nblocks, group, 2, 0.5, -1.0, percentiles=(0, 100))[0, 1] == np.inf
    gated = np.concatenate([rng.uniform(1.0, 2.0, 700), rng.uniform(1e-3, 2e-3, 600), rng.uniform(1e-9, 2e-9, 300)])  # both gates at work
    rng.shuffle(gated)
    assert check_range(gated, parts, 1e-7, 0.01, "gated")[0, 2] == 700


def test_range_with_every_stream_as_its_own_group_and_with_all_in_one():
    c = gate_case()
    zs, nbs, _ = S.blocks(c["e"], 4800, 30, 10, hops=c["hops"])
    rows = S.as_rows(zs, 88, GUARD)
    thresholds = S.gate_thresholds(-70.0, -20.0)
    for group, ngroups in ((list(range(7)), 7), ([0] * 7, 1), ([2, 0, -1, 0, 2, 5, 1], 4)):
        got = groups_device(rows, nbs, group, ngroups, *thresholds, percentiles=(10, 95))
        assert same(got, S.range_groups(zs, group, ngroups, *thresholds)), group


def test_the_meter_on_the_energies_of_a_track_batch():
    """3 tracks of 0.4, 0.9 and 1.3 s at 8000 -> 16000: 4, 9 and 13 hops or one fewer -- none holds a 3 s block, so their short-term
    maximum is -inf and their range 0; the LUFS values pass through log10 on both sides and are compared to 1e-12 (64 ulp of a
    number below 64)"""
    gen = torch.Generator(device="cuda").manual_seed(3)
    tracks = [(torch.randn((n, 2), generator=gen, device="cuda") * 0.1).contiguous() for n in (3200, 7200, 10400)]
    r = F.Resampler(8000, 16000, nch=2, nstreams=3)
    plan, table, rows = r._convert_tracks_rows(tracks)
    energy, hops = F.tracks_loudness_device(rows, table, 16000)
    groups = [0, 0, 1]
    meter = F.loudness_meter_device(energy, 1600, hops=hops, groups=groups, ngroups=2)
    e, h = energy.cpu().numpy(), hops.cpu().numpy()
    assert all(a - 1 <= b <= a for a, b in zip((4, 9, 13), h))
    z4, _, m4 = S.blocks(e, 1600, 4, 1, hops=h)
    z30, _, m30 = S.blocks(e, 1600, 30, 10, hops=h)
    _, _, s30 = S.blocks(e, 1600, 30, 1, hops=h)
    want = {"integrated": S.lufs(S.gate_groups(z4, [0, 1, 2], 3)), "momentary_max": S.power_lufs(m4), "short_term_max": S.power_lufs(s30),
            "range": S.range_lu(S.range_groups(z30, [0, 1, 2], 3)), "group_integrated": S.lufs(S.gate_groups(z4, groups, 2)),
            "group_range": S.range_lu(S.range_groups(z30, groups, 2))}
    assert sorted(meter) == sorted(want)
    for name, w in want.items():
        got = meter[name].cpu().numpy()
        print(name, got.tolist(), w.tolist())
        with np.errstate(invalid="ignore"):  # (-inf against -inf)
            assert got.shape == w.shape and np.all((got == w) | (np.abs(got - w) <= 1e-12)), name
    assert np.all(want["short_term_max"] == -np.inf) and not want["range"].any() and np.isfinite(want["integrated"][1:]).all()
    # long enough for everything: 80 hops of the first track's energies, repeated
    long = energy[:1, :, :h[0]].repeat(3, 1, 80 // int(h[0]) + 1)[:, :, :80].contiguous() * torch.tensor([1.0, 0.1, 0.01], dtype=torch.float64, device="cuda")[:, None, None]
    meter = F.loudness_meter_device(long, 1600, groups=[0, 0, 0], ngroups=1)
    le = long.cpu().numpy()
    z4, _, m4 = S.blocks(le, 1600, 4, 1)
    z30, _, _ = S.blocks(le, 1600, 30, 10)
    _, _, s30 = S.blocks(le, 1600, 30, 1)
    for name, w in (("integrated", S.lufs(S.gate_groups(z4, [0, 1, 2], 3))), ("short_term_max", S.power_lufs(s30)), ("momentary_max", S.power_lufs(m4)),
                    ("range", S.range_lu(S.range_groups(z30, [0, 1, 2], 3))), ("group_integrated", S.lufs(S.gate_groups(z4, [0, 0, 0], 1))),
                    ("group_range", S.range_lu(S.range_groups(z30, [0, 0, 0], 1)))):
        got = meter[name].cpu().numpy()
        assert got.shape == w.shape and np.isfinite(w).all() and np.all(np.abs(got - w) <= 1e-12), name
    assert np.isfinite(meter["short_term_max"].cpu().numpy()).all() and float(meter["group_range"][0]) > 5.0


def test_convert_tracks_to_pcm_loudness_normalized_by_album():
    nch, target, ceiling = 2, -18.0, -1.0
    n = torch.arange(30000, device="cuda", dtype=torch.float64)
    quiet = (torch.sin(2 * np.pi * 997.0 * n / 48000)[:, None] * 0.05).float().repeat(1, nch).contiguous()
    loud = (torch.sin(2 * np.pi * 440.0 * n[:24000] / 48000)[:, None] * 0.2).float().repeat(1, nch).contiguous()
    other = (torch.sin(2 * np.pi * 220.0 * n[:20000] / 48000)[:, None] * 0.01).float().repeat(1, nch).contiguous()
    tracks = [quiet, loud, other]
    r = F.Resampler(48000, 44100, nch=nch, nstreams=4)  # one stream runs empty: in no album
    views, peak, clipped, gain, true_peak, lufs = r.convert_tracks_to_pcm_loudness_normalized(tracks, F.RRX_FMT_S16, target_lufs=target, max_dbtp=ceiling,
                                                                                            album=[0, 0, 1])
    assert len(views) == 3 and tuple(gain.shape) == (3,) and tuple(true_peak.shape) == (3, nch) and tuple(lufs.shape) == (3,)
    assert gain[0] == gain[1] and lufs[0] == lufs[1] and gain[2] != gain[0] and lufs[2] != lufs[0]
    # the same rows again (a handle's output is a function of its input): the measurements, the model, the formula, the bytes
    r.reset()
    plan, table, rows = r._convert_tracks_rows(tracks)
    energy, hops = F.tracks_loudness_device(rows, table, 44100)
    tp, pk = F.tracks_true_peak_device(rows, table)
    assert torch.equal(tp[:3], true_peak)
    m = torch.maximum(tp, pk).amax(1).cpu().numpy()
    zs, _, _ = S.blocks(energy.cpu().numpy(), 4410, 4, 1, hops=hops.cpu().numpy())
    res = S.gate_groups(zs, [0, 0, 1, -1], 2)
    blocks, nblocks, _ = F.loudness_blocks_device(energy, 4410, 4, 1, hops=hops)
    d_res = F.loudness_gate_groups_device(blocks, nblocks, [0, 0, 1, -1], 2)
    assert np.array_equal(bits(d_res.cpu().numpy()), bits(res))
    album_lufs = S.lufs(res)
    lu, gg = lufs.cpu().numpy(), gain.cpu().numpy()
    print("album lufs %r, the tracks' %r, gain %r" % (album_lufs.tolist(), lu.tolist(), gg.tolist()))
    assert np.all(np.abs(lu - album_lufs[[0, 0, 1]]) <= 1e-12)
    most = np.array([max(m[0], m[1]), m[2]])
    want = F.loudness_normalizing_gain(torch.from_numpy(album_lufs), torch.from_numpy(res[:, 1].copy()), torch.from_numpy(most), target, ceiling).numpy()
    assert np.allclose(gg, want[[0, 0, 1]], rtol=1e-12, atol=0)
    d_gain = F.loudness_normalizing_gain(F.integrated_lufs(d_res), d_res[:, 1], torch.from_numpy(most).cuda(), target, ceiling)
    assert torch.equal(d_gain[[0, 0, 1]], gain)
    alone = S.lufs(S.gate_groups(zs, [0, 1, 2, -1], 3))
    assert alone[1] - alone[0] > 6.0 and alone[0] < album_lufs[0] < alone[1]  # the album lies between its tracks: their difference survives
    full = torch.ones(4, dtype=torch.float64, device="cuda")
    full[:3] = gain
    pcm, pk3, cl3 = F.tracks_finish_device(rows, table, F.RRX_FMT_S16, plan.dst_total, gain=full)
    for t, e in enumerate(plan.table[:3]):
        assert torch.equal(views[t], pcm[int(e.dst_first):int(e.dst_first + e.out_frames)])
    assert torch.equal(pk3[:3], peak) and torch.equal(cl3[:3], clipped)
    # album=None: the call as it was, issued by hand from the functions it was made of
    r.reset()
    v0, p0, c0, g0, t0, l0 = r.convert_tracks_to_pcm_loudness_normalized(tracks, F.RRX_FMT_S16, target_lufs=target, max_dbtp=ceiling)
    one = F.loudness_gate_device(energy, 4410, hops=hops)
    g1 = F.loudness_normalizing_gain(F.integrated_lufs(one), one[:, 1], torch.maximum(tp, pk).amax(1), target, ceiling)
    pcm1, p1, c1 = F.tracks_finish_device(rows, table, F.RRX_FMT_S16, plan.dst_total, gain=g1)
    assert torch.equal(g0, g1[:3]) and torch.equal(l0, F.integrated_lufs(one)[:3]) and torch.equal(t0, tp[:3])
    assert torch.equal(p0, p1[:3]) and torch.equal(c0, c1[:3])
    for t, e in enumerate(plan.table[:3]):
        assert torch.equal(v0[t], pcm1[int(e.dst_first):int(e.dst_first + e.out_frames)])
    assert g0[0] != g0[1]
    with pytest.raises(ValueError):
        r.convert_tracks_to_pcm_loudness_normalized(tracks, F.RRX_FMT_S16, album=[0, 0])
    with pytest.raises(ValueError):
        r.convert_tracks_to_pcm_loudness_normalized(tracks, F.RRX_FMT_S16, album=[0, -1, 0])
