"""The true-peak pass on the device (RRX_true_peak_device / RRX_tracks_true_peak_device, true_peak.hip) against the numpy
restatement of its arithmetic in true_peak_model.py, as bit patterns: both kernel forms, tiles and halos across workgroups,
strides under guard values, unaligned rows, chunked calls with ping-ponged states, other filter shapes, the tie to the output
stage's peak, the per-track call, and the normalising conversion built on it.

Where a channel holds a NaN or +-inf, the filter's sums hold NaNs (inf - inf, 0 * inf); the interface promises "a NaN stays", not
a payload, so such a channel is checked for being a NaN and every other channel for its exact bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import foo_dsp_resampler_amd as F
import true_peak_model as M

pytestmark = pytest.mark.gpu
GUARD = 777.25
# nch * taps <= 4096 doubles and nch <= 1024 take the LDS form (true_peak.hpp).  With 12 taps 341 channels is the last count on it
# (a tile of ONE frame behind a halo of 11) and 342 the smallest on the direct form; 1025 is on the direct form for every filter.
SHAPES = [(1, 1, 1), (1, 2, 11), (1, 2, 12), (1, 2, 13), (3, 3, 4099), (2, 5, 1201), (2, 3, 70001), (2, 31, 1201), (2, 257, 301), (2, 341, 40),
          (2, 342, 40), (2, 1025, 40)]
# Several tiles per workgroup: tiles per row x streams >= 4096 (true_peak.hip, launch_src).  300 channels leave tiles of 2 frames,
# 190 + 11 frames to evaluate are 101 tiles a row, 41 streams make 4141: two tiles per workgroup, the last one of a row with one.
STEPS = (41, 300, 190)


def same(got, want, what):
    for g, w, name in zip(got, want, ("true peak", "peak", "state")):
        if w is None:
            continue
        g, w = np.ascontiguousarray(g).view(np.uint64), np.ascontiguousarray(w).view(np.uint64)
        nan = np.isnan(w.view(np.float64))
        assert np.array_equal(g[~nan], w[~nan]), (name,) + tuple(what)
        assert np.isnan(g.view(np.float64)[nan]).all(), (name, "NaN") + tuple(what)


def device(x, coefs=M.BS1770, gain=None, first_frame=0, flush=True, state=None, tp=None, pk=None, pad=0, off=0, want_state=True):
    """RRX_true_peak_device through the C ABI on x [nstreams, frames, nch]: rows `pad` frames apart beyond their length, the
    first one `off` samples into a buffer filled with a guard value, which must come back unchanged.  (true peak bits, peak bits,
    state_out) as numpy arrays; `tp` / `pk` (uint64 arrays) are accumulated into."""
    ns, frames, nch = x.shape
    coefs = np.ascontiguousarray(coefs, dtype=np.float64)
    stride = frames + pad
    tdt = torch.float64 if x.dtype == np.float64 else torch.float32
    buf = torch.full((off + ns * stride * nch + 8,), GUARD, dtype=tdt, device="cuda")
    rows = buf[off:off + ns * stride * nch].view(ns, stride, nch)
    rows[:, :frames] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    before = buf.clone()
    d_tp = torch.from_numpy((np.zeros((ns, nch), np.uint64) if tp is None else tp).view(np.int64).copy()).cuda()
    d_pk = torch.from_numpy((np.zeros((ns, nch), np.uint64) if pk is None else pk).view(np.int64).copy()).cuda()
    d_g = None if gain is None else torch.from_numpy(np.ascontiguousarray(gain, dtype=np.float64)).cuda()
    d_si = None if state is None else torch.from_numpy(np.ascontiguousarray(state)).cuda()
    d_so = torch.full((ns, nch, 16), GUARD, dtype=torch.float64, device="cuda") if want_state else None
    F.ratelib._ensure_init()
    torch.cuda.synchronize()
    rc = F.lib().RRX_true_peak_device(-1, None, int(x.dtype == np.float64), C.c_void_p(rows.data_ptr()), stride, ns, frames, nch,
                                      None if d_g is None else C.c_void_p(d_g.data_ptr()), first_frame, coefs.ctypes.data, coefs.shape[0],
                                      coefs.shape[1], 1 if flush else 0, None if d_si is None else C.c_void_p(d_si.data_ptr()),
                                      None if d_so is None else C.c_void_p(d_so.data_ptr()), C.c_void_p(d_tp.data_ptr()), C.c_void_p(d_pk.data_ptr()))
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int64 if tdt == torch.float64 else torch.int32), before.view(torch.int64 if tdt == torch.float64 else torch.int32))
    return (d_tp.cpu().numpy().view(np.uint64), d_pk.cpu().numpy().view(np.uint64), None if d_so is None else d_so.cpu().numpy())


_cases = {}


def case(shape, dtype=np.float32):
    """an input of this shape and the model's answers for it (gain per stream, flush on), computed once"""
    key = (shape, np.dtype(dtype).name)
    if key not in _cases:
        rng = np.random.default_rng(sum(shape) + (dtype == np.float64))
        x = M.planted(rng, shape, dtype)
        gain = np.linspace(0.5, 1.7, shape[0])
        _cases[key] = (x, gain, M.true_peak(x, M.BS1770, gain, True))
    return _cases[key]


@pytest.mark.parametrize("nstreams,nch,frames", SHAPES)
def test_kernel_equals_the_model_bit_for_bit(nstreams, nch, frames):
    shape = (nstreams, frames, nch)
    x, gain, want = case(shape)
    same(device(x, gain=gain), want, shape)
    same(device(x, gain=gain, pad=3, off=1), want, shape + ("strided, one sample off",))
    if nstreams * nch * frames < 100000:
        for dtype in (np.float32, np.float64):
            x2, _, _ = case(shape, dtype)
            for g in (None, 0.5, 1.7):
                for flush in (False, True):
                    g2 = None if g is None else np.full(nstreams, g)
                    same(device(x2, gain=g2, flush=flush), M.true_peak(x2, M.BS1770, g2, flush), shape + (dtype, g, flush))


def test_workgroups_that_take_several_tiles():
    ns, nch, frames = STEPS
    x = (np.random.default_rng(9).standard_normal((ns, frames, nch)) * 0.5).astype(np.float32)
    gain = np.linspace(0.5, 1.7, ns)
    same(device(x, gain=gain), M.true_peak(x, M.BS1770, gain, True), STEPS)


@pytest.mark.parametrize("off", [1, 2, 3])
def test_rows_off_a_16_byte_boundary_under_guards(off):
    for shape in ((2, 1201, 5), (2, 40, 342)):
        x, gain, want = case(shape)
        same(device(x, gain=gain, pad=2, off=off), want, shape + (off,))
    x, gain, want = case((2, 1201, 5), np.float64)
    same(device(x, gain=gain, pad=1, off=off), want, ("double", off))


@pytest.mark.parametrize("phases,taps,shape", [(3, 5, (2, 4099, 3)), (8, 16, (2, 4099, 3)), (3, 5, (2, 40, 819)), (3, 5, (2, 40, 820)),
                                               (8, 16, (2, 40, 256)), (8, 16, (2, 40, 257)), (1, 1, (2, 300, 2))])
def test_generic_filters_beside_bs1770(phases, taps, shape):
    """(3, 5) and (8, 16) on both kernel forms: 819 / 820 and 256 / 257 channels are their last / first counts on either side"""
    rng = np.random.default_rng(phases * 100 + taps)
    coefs = rng.standard_normal((phases, taps))
    x = M.planted(rng, shape, np.float32)
    gain = np.array([0.5, 1.7])
    for flush in (False, True):
        same(device(x, coefs, gain=gain, flush=flush), M.true_peak(x, coefs, gain, flush), (phases, taps, shape, flush))


@pytest.mark.parametrize("shape", [(2, 4099, 3), (2, 60, 342)])
def test_chunked_calls_with_ping_ponged_states_equal_one_call(shape):
    x, gain, want = case(shape)
    frames = shape[1]
    for cuts in ([1], [10], [11], [12], [frames // 2 + 3], [5, 9, 12, 30, frames - 4, frames - 1]):  # [5, 9): a chunk shorter than taps - 1
        edges = [0] + cuts + [frames]
        tp, pk = np.zeros(want[0].shape, np.uint64), np.zeros(want[0].shape, np.uint64)
        state = None
        for a, b in zip(edges, edges[1:]):
            tp, pk, state = device(np.ascontiguousarray(x[:, a:b]), gain=gain, first_frame=a, flush=b == frames, state=state, tp=tp, pk=pk)
        same((tp, pk, state), want, shape + (tuple(cuts),))
    assert not want[2][:, :, 11:].any()


def test_peak_is_finish_device_measure_only_peak_and_the_python_call():
    x, gain, want = case((3, 4099, 3))
    t = torch.from_numpy(x.copy()).cuda()
    g = torch.from_numpy(gain).cuda()
    tp, pk, state = F.true_peak_device(t, gain=g)
    _, ref, _ = F.finish_device(t, None, gain=g)
    same((tp.cpu().numpy(), pk.cpu().numpy(), state.cpu().numpy()), want, ("python",))
    ok = ~torch.isnan(ref)
    assert torch.equal(pk.view(torch.int64)[ok], ref.view(torch.int64)[ok]) and torch.equal(torch.isnan(pk), torch.isnan(ref))
    # accumulation, a scalar gain, chunks through the wrapper, a [frames, nch] tensor
    tp2, pk2, st = F.true_peak_device(t[:, :2000].contiguous(), gain=g, flush=False)
    tp2, pk2, st2 = F.true_peak_device(t[:, 2000:].contiguous(), gain=g, first_frame=2000, state=st, true_peak=tp2, peak=pk2)
    assert st2 is not st
    same((tp2.cpu().numpy(), pk2.cpu().numpy(), st2.cpu().numpy()), want, ("python, chunked",))
    one = F.true_peak_device(t[0], gain=0.5)
    m = M.true_peak(x[:1], M.BS1770, np.array([0.5]), True)
    same((one[0].cpu().numpy(), one[1].cpu().numpy(), one[2].cpu().numpy()), m, ("python, one stream",))


LENGTHS = [0, 1, 40, 65, 3000, 70001]


def rows_under_guards(ntracks, row_frames, nch, seed):
    """random float32 rows [ntracks, row_frames, nch] inside a buffer with a guard row in front and behind"""
    buf = torch.full(((ntracks + 2) * row_frames * nch,), GUARD, dtype=torch.float32, device="cuda")
    rows = buf[row_frames * nch:(ntracks + 1) * row_frames * nch].view(ntracks, row_frames, nch)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    rows.copy_(torch.randn((ntracks, row_frames, nch), generator=gen, device="cuda") * 0.5)
    return buf, rows


def test_tracks_call_equals_one_stream_calls_on_each_slice():
    nch = 2
    plan = F.tracks_plan(44100, 48000, LENGTHS)
    table = plan.array()
    buf, rows = rows_under_guards(len(LENGTHS), plan.out_row_cap, nch, 1)
    before = buf.clone()
    gain = torch.linspace(0.5, 1.7, len(LENGTHS), dtype=torch.float64, device="cuda")
    tp, pk = F.tracks_true_peak_device(rows, plan.to_device("cuda"), gain=gain)
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    for t, e in enumerate(table):
        of, n = int(e[3]), int(e[4])
        assert n > 0 or LENGTHS[t] == 0
        if not n:
            assert not tp[t].any() and not pk[t].any()
            continue
        assert of > 0 or LENGTHS[t] < 65  # (the longer tracks' rows hold frames in front of the slice: they must not act as history)
        one_tp, one_pk, _ = F.true_peak_device(rows[t, of:of + n].contiguous(), gain=gain[t:t + 1])
        assert torch.equal(tp[t].view(torch.int64), one_tp[0].view(torch.int64)), t
        assert torch.equal(pk[t].view(torch.int64), one_pk[0].view(torch.int64)), t
    # and against the model for the short ones, double rows included
    x = rows.cpu().numpy()
    tpd, pkd = F.tracks_true_peak_device(rows.double(), plan.to_device("cuda"), gain=gain)
    for t in (1, 2, 3, 4):
        of, n = int(table[t][3]), int(table[t][4])
        want = M.true_peak(x[t:t + 1, of:of + n], M.BS1770, gain[t:t + 1].cpu().numpy(), True)
        same((tp[t:t + 1].cpu().numpy(), pk[t:t + 1].cpu().numpy()), want[:2], ("track", t))
        same((tpd[t:t + 1].cpu().numpy(), pkd[t:t + 1].cpu().numpy()), want[:2], ("track, double rows", t))


def test_a_wrong_table_gives_numbers_and_stays_inside_the_rows():
    """out_first and out_frames beyond the row are clamped to it (tracks_slice): the guard rows around the buffer stay as they
    are, and what comes back is the measurement of the clamped slices.  That is a clamp at work, not a fault provoked."""
    nch, row_frames = 3, 500
    buf, rows = rows_under_guards(4, row_frames, nch, 2)
    before = buf.clone()
    table = np.zeros((4, 6), np.uint64)
    table[0, 3:5] = (100, 10 ** 9)              # runs past the end of its row: clamped to [100, 500)
    table[1, 3:5] = (2 ** 63, 7)                # begins far outside: clamped to nothing
    table[2, 3:5] = (499, 2 ** 64 - 1)          # the sum would wrap: clamped to [499, 500)
    table[3, 3:5] = (0, 500)                    # a right entry
    d_table = torch.from_numpy(table.view(np.int64)).cuda()
    tp, pk = F.tracks_true_peak_device(rows, d_table)
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    x = rows.cpu().numpy()
    for t, (of, n) in enumerate([(100, 400), (500, 0), (499, 1), (0, 500)]):
        if not n:
            assert not tp[t].any() and not pk[t].any()
            continue
        want = M.true_peak(x[t:t + 1, of:of + n], M.BS1770, None, True)
        same((tp[t:t + 1].cpu().numpy(), pk[t:t + 1].cpu().numpy()), want[:2], ("wrong table", t))


def test_convert_tracks_to_pcm_normalized():
    nch, target_dbtp = 2, -1.0
    target = 10.0 ** (target_dbtp / 20.0)
    gen = torch.Generator(device="cuda").manual_seed(3)
    n = torch.arange(3000, device="cuda", dtype=torch.float64)
    tone = torch.sin(2 * np.pi * n / 4 + np.pi / 4)[:, None].float().repeat(1, nch) * 0.3   # its peaks lie between the samples
    tracks = [tone.contiguous(), torch.zeros((1200, nch), device="cuda"), torch.randn((2000, nch), generator=gen, device="cuda") * 0.2]
    r = F.Resampler(44100, 48000, nch=nch, nstreams=3)
    views, peak, clipped, gain, true_peak = r.convert_tracks_to_pcm_normalized(tracks, F.RRX_FMT_S16, target_dbtp=target_dbtp)
    assert len(views) == 3 and tuple(gain.shape) == (3,) and tuple(true_peak.shape) == (3, nch) and gain.dtype == torch.float64
    assert float(gain[1]) == 1.0 and not views[1].any() and not true_peak[1].any()
    assert not clipped.any()
    # the same rows again (a handle's output is a function of its input), re-measured under the returned gain
    r.reset()
    plan, table, rows = r._convert_tracks_rows(tracks)
    tp2, pk2 = F.tracks_true_peak_device(rows, table, gain=gain)
    m0 = torch.maximum(*F.tracks_true_peak_device(rows, table)).amax(1)
    m2 = torch.maximum(tp2, pk2).amax(1)
    for t in (0, 2):
        assert float(gain[t]) == target / float(m0[t])
        rel = abs(float(m2[t]) - target) / target
        print("track %d: gain %.17g, re-measured peak %.17g, relative error %.3g" % (t, float(gain[t]), float(m2[t]), rel))
        assert rel <= 1e-12
    assert float(true_peak[0].max()) > 1.3 * float(tone.abs().max())  # the tone's true peak is well above its samples
    pcm, pk3, cl3 = F.tracks_finish_device(rows, table, F.RRX_FMT_S16, plan.dst_total, gain=gain)
    for t, e in enumerate(plan.table):
        assert torch.equal(views[t], pcm[int(e.dst_first):int(e.dst_first + e.out_frames)])
    assert torch.equal(pk3[:3], peak) and torch.equal(cl3[:3], clipped)
    # with shaping the same gain and other bytes
    r.reset()
    v2, _, _, gain2, tpk2 = r.convert_tracks_to_pcm_normalized(tracks, F.RRX_FMT_S16, target_dbtp=target_dbtp, shaping="wannamaker3", dither=True, seed=5)
    assert torch.equal(gain2, gain) and torch.equal(tpk2, true_peak) and not torch.equal(v2[0], views[0])
