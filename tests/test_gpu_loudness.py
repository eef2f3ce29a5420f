"""The loudness measurement on the device (RRX_loudness_device / RRX_tracks_loudness_device / RRX_loudness_gate_device,
loudness.hip) against the numpy restatement of its arithmetic in loudness_model.py, as bit patterns: hops across workgroups, tiles
and channel chunks, strides and unaligned rows under guard values, guarded energy and work buffers, chunked calls with ping-ponged
states, the per-track call with right and wrong tables, the gate, and the normalising conversion built on them."""
import ctypes as C

import numpy as np
import pytest
import torch

import foo_dsp_resampler_amd as F
import loudness_model as M

pytestmark = pytest.mark.gpu
GUARD = 777.25


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def device(x, hop, coefs=M.K48, gain=None, first_frame=0, state=None, energy=None, pad=0, off=0):
    """RRX_loudness_device through the C ABI on x [nstreams, frames, nch]: rows `pad` frames apart beyond their length, the first
    one `off` samples into a buffer filled with a guard value, which must come back unchanged; the energy buffer has two more hops
    per channel than the call owns and the work buffer three more doubles, all under guards.  (energy [nstreams, nch, first_hop +
    n + 2] as numpy, state_out)"""
    ns, frames, nch = x.shape
    n, first_hop = frames // hop, first_frame // hop
    stride = frames + pad
    tdt = torch.float64 if x.dtype == np.float64 else torch.float32
    buf = torch.full((off + ns * stride * nch + 8,), GUARD, dtype=tdt, device="cuda")
    rows = buf[off:off + ns * stride * nch].view(ns, stride, nch)
    rows[:, :frames] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    before = buf.clone()
    need = F.lib().RRX_loudness_work_doubles(ns, nch, frames, hop)
    d_work = torch.full((need + 3,), GUARD, dtype=torch.float64, device="cuda")
    d_e = torch.from_numpy(np.full((ns, nch, first_hop + n + 2), GUARD) if energy is None else energy).cuda()
    d_g = None if gain is None else torch.from_numpy(np.ascontiguousarray(gain, dtype=np.float64)).cuda()
    d_si = None if state is None else torch.from_numpy(np.ascontiguousarray(state)).cuda()
    d_so = torch.full((ns, nch, 4), GUARD, dtype=torch.float64, device="cuda")
    co = np.ascontiguousarray(coefs, dtype=np.float64)
    F.ratelib._ensure_init()
    torch.cuda.synchronize()
    src = buf.data_ptr() + off * buf.element_size()  # (rows.data_ptr(), which an empty view does not have)
    rc = F.lib().RRX_loudness_device(-1, None, int(x.dtype == np.float64), C.c_void_p(src), stride, ns, frames, nch,
                                     None if d_g is None else C.c_void_p(d_g.data_ptr()), first_frame, co.ctypes.data, hop,
                                     None if d_si is None else C.c_void_p(d_si.data_ptr()), C.c_void_p(d_so.data_ptr()),
                                     C.c_void_p(d_e.data_ptr()), d_e.shape[2], C.c_void_p(d_work.data_ptr()), need)
    assert rc == 0
    torch.cuda.synchronize()
    view = torch.int64 if tdt == torch.float64 else torch.int32
    assert torch.equal(buf.view(view), before.view(view))
    assert bool((d_work[need:] == GUARD).all())
    return d_e.cpu().numpy(), d_so.cpu().numpy()


def check(x, hop, gain, want_e, want_s, what, **kw):
    """one call on x against the model's energies [nstreams, nch, n] and end state"""
    n = x.shape[1] // hop
    e, so = device(x, hop, gain=gain, **kw)
    if not x.shape[1]:
        assert np.all(e == GUARD) and np.all(so == GUARD), what  # frames == 0 touches nothing
        return
    assert np.array_equal(bits(e[:, :, :n]), bits(want_e[:, :, :n])), what
    assert np.all(e[:, :, n:] == GUARD), what
    assert np.array_equal(bits(so), bits(want_s)), what


@pytest.mark.parametrize("hop", [1, 7, 48, 4410])
@pytest.mark.parametrize("ns,nch", [(1, 1), (1, 2), (3, 3), (2, 6)])
def test_kernels_equal_the_model_bit_for_bit(ns, nch, hop):
    """float32 under a gain and float64 without one, at every length of the host test: the model runs once on the longest, and a
    call on a prefix has its first hops and the state behind them"""
    rng = np.random.default_rng(ns * 1000 + nch * 100 + hop)
    longest = 37 * hop + 5
    x32 = (rng.standard_normal((ns, longest, nch)) * 0.3).astype(np.float32)
    x64 = rng.standard_normal((ns, longest, nch)) * 0.3
    gain = np.linspace(0.5, 1.7, ns)
    e, s = M.hop_energies(np.concatenate([M.gained(x32, gain), x64]), M.K48, hop, every_state=True)
    for frames in (0, hop - 1, hop, 4 * hop - 1, 4 * hop, longest):
        n = frames // hop
        check(np.ascontiguousarray(x32[:, :frames]), hop, gain, e[:ns], s[:ns, :, n], (frames, "float32"), pad=3)
        check(np.ascontiguousarray(x64[:, :frames]), hop, None, e[ns:], s[ns:, :, n], (frames, "float64"))


_cases = {}


def case(ns, nch, nhops, hop):
    """an input of this shape (5 frames behind the last whole hop) and the model's answers for it, computed once"""
    key = (ns, nch, nhops, hop)
    if key not in _cases:
        rng = np.random.default_rng(sum(key))
        x = (rng.standard_normal((ns, nhops * hop + 5, nch)) * 0.3).astype(np.float32)
        gain = np.linspace(0.5, 1.7, ns)
        _cases[key] = (x, gain) + M.hop_energies(M.gained(x, gain), M.K48, hop)
    return _cases[key]


# 300 hops of 2 channels: 600 lanes a stream, three workgroups, the last one partly filled; 33 channels: waves and workgroups that
# straddle hops; hops of 70001 frames: 4376 register tiles, the last one of one frame; 257 channels: more channels than a workgroup
@pytest.mark.parametrize("ns,nch,nhops,hop", [(3, 2, 300, 48), (2, 33, 40, 7), (1, 1, 2, 70001), (2, 257, 5, 48)])
def test_shapes_that_cross_workgroups_tiles_and_chunks(ns, nch, nhops, hop):
    x, gain, e, s = case(ns, nch, nhops, hop)
    check(x, hop, gain, e, s, (ns, nch, nhops, hop))


@pytest.mark.parametrize("off", [1, 2, 3])
def test_rows_off_a_16_byte_boundary_under_guards(off):
    for key in ((3, 2, 300, 48), (2, 33, 40, 7)):
        x, gain, e, s = case(*key)
        check(x, key[3], gain, e, s, key + (off,), pad=2, off=off)
    x, gain, e, s = case(3, 2, 300, 48)
    x64 = x.astype(np.float64)  # (the float32 values as doubles: the same gained frames, the same bits)
    check(x64, 48, gain, e, s, ("double", off), pad=1, off=off)


def test_chunked_calls_with_ping_ponged_states_equal_one_call():
    ns, nch, nhops, hop = 3, 2, 300, 48
    x, gain, e, s = case(ns, nch, nhops, hop)
    for cuts in ([1], [0], [150, 150, 299], [7, 128, 129, 256]):  # equal edges: a call of hop - 1 frames, without a whole hop
        edges = [0] + [c * hop for c in cuts] + [x.shape[1]]
        energy = np.full((ns, nch, nhops + 2), GUARD)
        state = None
        for a, b in zip(edges, edges[1:]):
            chunk = np.ascontiguousarray(x[:, a:b] if b - a else x[:, a:a + hop - 1])
            energy, state = device(chunk, hop, gain=gain, first_frame=a, state=state, energy=energy)
        assert np.array_equal(bits(energy[:, :, :nhops]), bits(e)) and np.all(energy[:, :, nhops:] == GUARD), cuts
        assert np.array_equal(bits(state), bits(s)), cuts


def test_a_nan_poisons_its_channel_only():
    x, gain, e, s = case(3, 2, 300, 48)
    y = x.copy()
    y[1, 100 * 48 + 3, 1] = np.nan
    got, so = device(y, 48, gain=gain)
    assert np.isnan(got[1, 1, 100:300]).all() and np.isnan(so[1, 1]).all()
    got[1, 1, 100:300] = e[1, 1, 100:300]
    so[1, 1] = s[1, 1]
    assert np.array_equal(bits(got[:, :, :300]), bits(e)) and np.array_equal(bits(so), bits(s))


def test_the_python_calls():
    x, gain, e, s = case(3, 2, 300, 48)
    t = torch.from_numpy(x).cuda()
    g = torch.from_numpy(gain).cuda()
    energy, state = F.loudness_device(t, coefs=M.K48, hop=48, gain=g)
    assert tuple(energy.shape) == (3, 2, 300) and np.array_equal(bits(energy.cpu().numpy()), bits(e)) and np.array_equal(bits(state.cpu().numpy()), bits(s))
    e2, st = F.loudness_device(t[:, :4800].contiguous(), coefs=M.K48, hop=48, gain=g, energy=torch.zeros_like(energy))
    e2, st2 = F.loudness_device(t[:, 4800:].contiguous(), coefs=M.K48, hop=48, gain=g, first_frame=4800, state=st, energy=e2)
    assert st2 is not st and torch.equal(e2, energy) and torch.equal(st2, state)
    e48, _ = F.loudness_device(t[0], 4800)  # [frames, nch], the K-weighting of a rate, hops of rate // 10
    want, _ = M.hop_energies(M.gained(x[:1]), np.array(F.k_weighting(4800)), 480)
    assert np.array_equal(bits(e48.cpu().numpy()), bits(want))
    res = F.loudness_gate_device(energy, 48)
    assert np.array_equal(bits(res.cpu().numpy()), bits(M.gate(e, 48)))
    assert np.allclose(F.integrated_lufs(res).cpu().numpy(), M.lufs(M.gate(e, 48)), rtol=1e-14, atol=0)


def rows_under_guards(ntracks, row_frames, nch, seed):
    """random float32 rows [ntracks, row_frames, nch] inside a buffer with a guard row in front and behind"""
    buf = torch.full(((ntracks + 2) * row_frames * nch,), GUARD, dtype=torch.float32, device="cuda")
    rows = buf[row_frames * nch:(ntracks + 1) * row_frames * nch].view(ntracks, row_frames, nch)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    rows.copy_(torch.randn((ntracks, row_frames, nch), generator=gen, device="cuda") * 0.3)
    return buf, rows


def tracks_call(rows, table, hop, gain, energy_hops):
    """tracks_loudness_device with the energy and work buffers under guards: (energy [ntracks, nch, energy_hops], hops)"""
    ntracks, row_frames, nch = rows.shape
    need = F.lib().RRX_loudness_work_doubles(ntracks, nch, row_frames, hop)
    work = torch.full((need + 3,), GUARD, dtype=torch.float64, device="cuda")
    ebuf = torch.full((ntracks * nch * energy_hops + 4,), GUARD, dtype=torch.float64, device="cuda")
    energy = ebuf[:ntracks * nch * energy_hops].view(ntracks, nch, energy_hops)
    d_table = torch.from_numpy(np.ascontiguousarray(table).view(np.int64)).cuda()
    _, hops = F.tracks_loudness_device(rows, d_table, coefs=M.K48, hop=hop, gain=gain, energy=energy, work=work[:need] if need else work[:1])
    torch.cuda.synchronize()
    assert bool((work[need:] == GUARD).all()) and bool((ebuf[ntracks * nch * energy_hops:] == GUARD).all())
    return energy.cpu().numpy(), hops.cpu().numpy()


def check_tracks(rows, gain, hop, slices, energy, hops):
    x = rows.cpu().numpy()
    for t, (of, frames) in enumerate(slices):
        n = min(frames // hop, energy.shape[2])
        assert hops[t] == n, t
        want, _ = M.hop_energies(M.gained(x[t:t + 1, of:of + frames], None if gain is None else gain[t:t + 1].cpu().numpy()), M.K48, hop)
        assert np.array_equal(bits(energy[t, :, :n]), bits(want[0, :, :n])), t
        assert np.all(energy[t, :, n:] == GUARD), t  # energies at hops[t] and beyond are left untouched


def test_tracks_call_on_a_ragged_table():
    nch, hop = 2, 441
    lengths = [0, 300, 3000, 20000, 7000]  # a zero-length track, one shorter than a hop, tracks of unequal length
    plan = F.tracks_plan(44100, 48000, lengths)
    table = plan.array()
    buf, rows = rows_under_guards(len(lengths), plan.out_row_cap, nch, 1)
    before = buf.clone()
    gain = torch.linspace(0.5, 1.7, len(lengths), dtype=torch.float64, device="cuda")
    slices = [(int(e[3]), int(e[4])) for e in table]
    assert slices[0][1] == 0 and 0 < slices[1][1] < hop and slices[3][0] > 0  # (a row holds frames in front of its slice: not history)
    energy, hops = tracks_call(rows, table, hop, gain, plan.out_row_cap // hop)
    assert torch.equal(buf, before)
    assert hops[0] == 0 and hops[1] == 0 and hops[3] > hops[4] > hops[2] > 0
    check_tracks(rows, gain, hop, slices, energy, hops)
    d_table = plan.to_device("cuda")
    e64, h64 = F.tracks_loudness_device(rows.double(), d_table, coefs=M.K48, hop=hop, gain=gain)
    assert np.array_equal(h64.cpu().numpy(), hops)
    for t in range(len(lengths)):
        assert np.array_equal(bits(e64[t, :, :hops[t]].cpu().numpy()), bits(energy[t, :, :hops[t]]))


def test_a_wrong_table_gives_numbers_and_stays_inside_the_buffers():
    """out_first and out_frames beyond the row are clamped to it (tracks_slice) and the hop count to the energy rows: the guards
    around the rows, the energies and the work buffer stay as they are, and what comes back is the measurement of the clamped
    slices.  That is a clamp at work, not a fault provoked."""
    nch, row_frames, hop = 3, 500, 7
    buf, rows = rows_under_guards(4, row_frames, nch, 2)
    before = buf.clone()
    table = np.zeros((4, 6), np.uint64)
    table[0, 3:5] = (100, 10 ** 9)              # runs past the end of its row: clamped to [100, 500)
    table[1, 3:5] = (2 ** 63, 7)                # begins far outside: clamped to nothing
    table[2, 3:5] = (492, 2 ** 64 - 1)          # the sum would wrap: clamped to [492, 500), one hop
    table[3, 3:5] = (0, 500)                    # a right entry, with more hops (71) than the energy rows hold (60)
    energy, hops = tracks_call(rows, table, hop, None, 60)
    assert torch.equal(buf, before)
    assert list(hops) == [57, 0, 1, 60]
    check_tracks(rows, None, hop, [(100, 400), (500, 0), (492, 8), (0, 500)], energy, hops)


def test_gate_kernel_equals_the_model():
    rng = np.random.default_rng(4)
    e = rng.uniform(1.0, 50.0, (3, 6, 3000))
    e[:, :, 1000:2000] *= 0.01       # a quiet third the relative gate removes
    e[2, :, 2500:] *= 1e-12          # and a stretch under the absolute gate
    e[2, 4, 77] = np.nan             # four blocks to skip
    hops = np.array([1, 5, 3000])    # no block, two blocks, every tile of the kernel
    w = [1.0, 1.0, 1.0, 0.0, 1.41, 1.41]
    d_e = torch.from_numpy(e).cuda()
    d_h = torch.from_numpy(hops).cuda()
    for weights in (None, w):
        got = F.loudness_gate_device(d_e, 4800, hops=d_h, weights=weights).cpu().numpy()
        want = M.gate(e, 4800, hops=hops, weights=weights)
        assert np.array_equal(bits(got), bits(want)), weights
        assert not got[0].any() and got[1, 3] == 2 and 0 < got[2, 1] < got[2, 3] < 2997 - 4
    got = F.loudness_gate_device(d_e, 4800, weights=w).cpu().numpy()  # without d_hops: nhops for all
    assert np.array_equal(bits(got), bits(M.gate(e, 4800, weights=w)))
    got = F.loudness_gate_device(d_e, 4800, abs_lufs=-20.0, rel_lu=-3.0).cpu().numpy()
    assert np.array_equal(bits(got), bits(M.gate(e, 4800, None, None, *M.gate_thresholds(-20.0, -3.0))))


def test_convert_tracks_to_pcm_loudness_normalized():
    nch, target, ceiling = 2, -18.0, -1.0
    n = torch.arange(30000, device="cuda", dtype=torch.float64)
    quiet = (torch.sin(2 * np.pi * 997.0 * n / 48000)[:, None] * 0.05).float().repeat(1, nch).contiguous()         # about -26 LUFS: raised to the target
    loud = (torch.sin(2 * np.pi * 440.0 * n[:24000] / 48000)[:, None] * 0.02).float().repeat(1, nch).contiguous()
    loud[12000:12004] = 0.9                                                                                       # a click: the ceiling holds this one
    tracks = [quiet, loud, torch.zeros((9000, nch), device="cuda")]
    r = F.Resampler(48000, 44100, nch=nch, nstreams=3)
    views, peak, clipped, gain, true_peak, lufs = r.convert_tracks_to_pcm_loudness_normalized(tracks, F.RRX_FMT_S16, target_lufs=target, max_dbtp=ceiling)
    assert len(views) == 3 and tuple(gain.shape) == (3,) and tuple(true_peak.shape) == (3, nch) and tuple(lufs.shape) == (3,)
    assert gain.dtype == torch.float64 and lufs.dtype == torch.float64
    # the same rows again (a handle's output is a function of its input): the measurements, the formula, the bytes
    r.reset()
    plan, table, rows = r._convert_tracks_rows(tracks)
    energy, hops = F.tracks_loudness_device(rows, table, 44100)
    res = F.loudness_gate_device(energy, 4410, hops=hops)
    assert torch.equal(F.integrated_lufs(res)[:3], lufs)
    tp, pk = F.tracks_true_peak_device(rows, table)
    assert torch.equal(tp[:3], true_peak)
    m = torch.maximum(tp, pk).amax(1)
    assert torch.equal(F.loudness_normalizing_gain(F.integrated_lufs(res), res[:, 1], m, target, ceiling)[:3], gain)
    lu, mm, gg = lufs.cpu().numpy(), m.cpu().numpy(), gain.cpu().numpy()
    print("lufs %r, m %r, gain %r" % (lu.tolist(), mm[:3].tolist(), gg.tolist()))
    by_loudness, by_peak = 10.0 ** ((target - lu[:2]) / 20.0), 10.0 ** (ceiling / 20.0) / mm[:2]
    assert np.allclose(gg[:2], np.minimum(by_loudness, by_peak), rtol=1e-12, atol=0)
    assert by_loudness[0] < by_peak[0] and gg[0] > 1.0          # the quiet track reaches the target
    assert by_peak[1] < by_loudness[1]                          # the loud one is held by the ceiling
    assert lu[2] == -np.inf and gg[2] == 1.0 and not views[2].any()
    assert abs(lu[0] - -26.02) <= 0.1                           # 0.05 of full scale at 997 Hz on two channels: -3.01 - 26.02 + 3.01 LUFS
    pcm, pk3, cl3 = F.tracks_finish_device(rows, table, F.RRX_FMT_S16, plan.dst_total, gain=gain)
    for t, e in enumerate(plan.table):
        assert torch.equal(views[t], pcm[int(e.dst_first):int(e.dst_first + e.out_frames)])
    assert torch.equal(pk3[:3], peak) and torch.equal(cl3[:3], clipped) and not clipped.any()
    after = float(peak[1].max())                                # the sample peak after the gain lies under the ceiling (to one rounding)
    assert after <= 10.0 ** (ceiling / 20.0) * (1 + 1e-15)
