"""The output stage on the device (RRX_finish_device, finish.hip) against the numpy restatement of its arithmetic in
finish_model.py: output bytes, peak bit patterns and clip counts, through strides, guard bytes and unaligned rows; the Python
wrappers; and the tie to the engine -- without gain and dither it is the integer handles' own quantiser."""
import numpy as np
import pytest
import torch

import foo_dsp_resampler_amd as F
import finish_model as M

pytestmark = pytest.mark.gpu
SEED = 0x1234567887654321
BIG = (2, 3, 70001)   # many workgroups, a channel phase that does not line up with them


def same(got, want, x, what):
    assert np.array_equal(got[0], want[0]), ("output bytes",) + what
    nanch = M.nan_channels(x)
    assert np.array_equal(got[1][~nanch], want[1][~nanch]), ("peak bit patterns",) + what
    assert np.isnan(got[1].view(np.float64)[nanch]).all(), ("peak of the NaN channel",) + what
    assert np.array_equal(got[2], want[2]), ("clip counts",) + what


@pytest.mark.parametrize("nstreams,nch,frames", [(s, c, n) for s, c in M.SHAPES for n in M.FRAMES] + [BIG])
def test_kernel_equals_the_model_bit_for_bit(nstreams, nch, frames):
    for fmt in M.FORMATS:
        for double in (False, True):
            for gain in M.GAINS:
                for dith in (False, True):
                    x, g, want = M.case(nstreams, frames, nch, fmt, double, gain, dith, SEED)
                    aligned = M.device(x, fmt, g, dith, SEED)
                    same(aligned, want, x, (fmt, double, gain, dith, "aligned"))
                    shifted = M.device(x, fmt, g, dith, SEED, src_off=1, dst_off=1, pad=2)
                    same(shifted, want, x, (fmt, double, gain, dith, "one sample off"))
                    assert np.array_equal(shifted[0], aligned[0])


@pytest.mark.parametrize("nch", [5, 31, 257])
def test_every_destination_phase_and_both_statistics_paths(nch):
    """every position of a row against the dword grid (packed 24 bit has four), and channel counts on both sides of the boundary
    between the statistics kept in registers and LDS (nch = 5, 31) and those sent straight to global memory (257: lcm(4, nch) > 1024)"""
    x = M.make_input(2, 1201, nch, F.RRX_FMT_S24_3, False)
    g = np.array([0.5, 1.7])
    for fmt in M.FORMATS:
        want = M.model(x, fmt, g, True, SEED, 77)
        for off in range(4):
            same(M.device(x, fmt, g, True, SEED, 77, src_off=off, dst_off=off, pad=1), want, x, (fmt, nch, off))


# A workgroup takes more than one step of its main loop once a call holds about 8.4 M samples (finish.hip, launch_typed: steps =
# row steps x streams / 4096), which every real track does.  Both shapes below give steps = 2: 128 row steps of 1024 samples x 64
# streams, and 129 row steps of 1020 samples (the largest multiple of lcm(4, 3) within 1024) x 64 streams, the last workgroup of
# a row with one step only.
LONG = [(64, 4, 32768), (64, 3, 43691)]
FIRST = 2 ** 40 + 12345


@pytest.mark.parametrize("fmt", [F.RRX_FMT_S16, F.RRX_FMT_S24_3])
@pytest.mark.parametrize("nstreams,nch,frames", LONG)
def test_workgroups_that_take_several_steps(nstreams, nch, frames, fmt):
    """the per-step frame advance, the start of a workgroup's first step and the statistics carried in registers across steps:
    dithered bytes (which depend on every sample's frame and channel), peak bits and clip counts against the model, with a first
    frame beyond 2^32, gains that clip about a third of the samples of the loudest streams, and rows that start one sample off
    the dword grid, so the steps start behind a head"""
    x = M.make_input(nstreams, frames, nch, F.RRX_FMT_S24_3, False)
    g = np.linspace(0.5, 3.0, nstreams)
    want = M.model(x, fmt, g, True, SEED, FIRST)
    assert int(want[2][-1].min()) > frames // 4 and int(want[2][0].max()) < 64     # the counts differ widely between the streams
    same(M.device(x, fmt, g, True, SEED, FIRST, pad=1, src_off=1, dst_off=1), want, x, (fmt, nstreams, nch, frames))


def test_measure_only_accumulation_and_chunks_through_the_python_call():
    x = M.make_input(3, 4099, 3, F.RRX_FMT_S32, False)
    t = torch.from_numpy(x.copy()).cuda()
    g = torch.tensor([0.5, 1.0, 1.7], dtype=torch.float64, device="cuda")
    want = M.model(x, F.RRX_FMT_S32, g.cpu().numpy(), True, SEED)
    out, pk, cl = F.finish_device(t, F.RRX_FMT_S32, gain=g, dither=True, seed=SEED)
    assert out.dtype == torch.int32 and tuple(out.shape) == x.shape and pk.dtype == torch.float64 and cl.dtype == torch.int64
    got = (out.cpu().numpy().view(np.uint8).reshape(3, 4099, 12), pk.cpu().numpy().view(np.uint64), cl.cpu().numpy().view(np.uint64))
    same(got, want, x, ("python",))
    # measure only: no output, the statistics of the writing call
    before = torch.cuda.memory_allocated()
    none, pk0, cl0 = F.finish_device(t, None, gain=g, dither=True, seed=SEED)
    assert none is None and torch.cuda.memory_allocated() - before <= 2 * 512   # the two statistics tensors, nothing else
    assert torch.equal(pk0.view(torch.int64)[~torch.isnan(pk0)], pk.view(torch.int64)[~torch.isnan(pk)]) and torch.equal(cl0, cl)
    assert torch.equal(torch.isnan(pk0), torch.isnan(pk))
    # the peak does not depend on the format; a scalar gain is one gain for every stream
    o16, pk16, _ = F.finish_device(t, F.RRX_FMT_S16, gain=0.5)
    o24, pk24, _ = F.finish_device(t, F.RRX_FMT_S24_3, gain=0.5)
    assert o16.dtype == torch.int16 and o24.dtype == torch.uint8 and tuple(o24.shape) == (3, 4099, 9)
    w16, wpk, _ = M.model(x, F.RRX_FMT_S16, np.full(3, 0.5))
    assert np.array_equal(o16.cpu().numpy().view(np.uint8).reshape(3, 4099, 6), w16)
    assert np.array_equal(o24.cpu().numpy(), M.model(x, F.RRX_FMT_S24_3, np.full(3, 0.5))[0])
    ok = ~M.nan_channels(x)
    assert np.array_equal(pk16.cpu().numpy().view(np.uint64)[ok], wpk[ok]) and torch.equal(pk16.view(torch.int64)[torch.from_numpy(ok).cuda()],
                                                                                          pk24.view(torch.int64)[torch.from_numpy(ok).cuda()])
    # two calls accumulate: chunks of one track, first_frame = the frames done so far
    a, pk2, cl2 = F.finish_device(t[:, :1001].contiguous(), F.RRX_FMT_S32, gain=g, dither=True, seed=SEED)
    b, pk2b, cl2b = F.finish_device(t[:, 1001:].contiguous(), F.RRX_FMT_S32, gain=g, dither=True, seed=SEED, first_frame=1001, peak=pk2, clipped=cl2)
    assert pk2b is pk2 and cl2b is cl2
    assert torch.equal(torch.cat([a, b], dim=1), out) and torch.equal(cl2, cl)
    assert np.array_equal(pk2.cpu().numpy().view(np.uint64)[ok], want[1][ok])
    # 2-D input: one stream
    o2, p2, c2 = F.finish_device(t[1], F.RRX_FMT_S32, gain=torch.tensor([0.5], dtype=torch.float64, device="cuda"), dither=True, seed=SEED)
    w2 = M.model(x[1:2], F.RRX_FMT_S32, np.array([0.5]), True, SEED)
    assert tuple(o2.shape) == (4099, 3) and tuple(p2.shape) == (1, 3)
    assert np.array_equal(o2.cpu().numpy().view(np.uint8).reshape(1, 4099, 12), w2[0]) and np.array_equal(c2.cpu().numpy().view(np.uint64), w2[2])
    with pytest.raises(TypeError):
        F.finish_device(t, F.RRX_FMT_S16, gain=torch.ones(3, device="cuda"))          # float32 gain
    with pytest.raises(TypeError):
        F.finish_device(t, F.RRX_FMT_S16, out=torch.empty((3, 4099, 3), dtype=torch.int32, device="cuda"))
    with pytest.raises(TypeError):
        F.finish_device(t.cpu(), F.RRX_FMT_S16, peak=pk)


def test_non_default_stream():
    x = M.make_input(2, 4099, 8, F.RRX_FMT_S16, True)
    want = M.model(x, F.RRX_FMT_S16, None, True, 5)
    side = torch.cuda.Stream()
    same(M.device(x, F.RRX_FMT_S16, None, True, 5, stream=side), want, x, ("side stream, C call",))
    t = torch.from_numpy(x.copy()).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        out, pk, cl = F.finish_device(t, F.RRX_FMT_S16, dither=True, seed=5, stream=side)
    side.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint8).reshape(2, 4099, 16), want[0])
    assert np.array_equal(cl.cpu().numpy().view(np.uint64), want[2])


@pytest.mark.parametrize("fmt,bits,dtype", [(F.RRX_FMT_S16, 15, np.int16), (F.RRX_FMT_S32, 31, np.int32)])
def test_it_is_the_integer_handles_quantiser(fmt, bits, dtype):
    """ratelib_amd.h: an integer handle's output equals that of an RRX_FMT_DOUBLE handle fed s * 2^-bits, quantised by the rule --
    which is this call without gain and dither"""
    rng = np.random.default_rng(11)
    s = rng.integers(-2 ** bits, 2 ** bits, (6000, 2), dtype=np.int64).astype(dtype)
    yi = F.Resampler(44100, 48000, nch=2, sample_format=fmt).process(s, chunk=2048)
    yd = F.Resampler(44100, 48000, nch=2, dtype=np.float64).process(s.astype(np.float64) * 2.0 ** -bits, chunk=2048)
    assert yi.shape == yd.shape and yi.dtype == dtype
    out, pk, cl = F.finish_device(torch.from_numpy(yd).cuda(), fmt)
    assert np.array_equal(out.cpu().numpy(), yi)
    assert int(cl.sum()) == int(((yd * 2.0 ** bits).round() > 2.0 ** bits - 1).sum() + ((yd * 2.0 ** bits).round() < -2.0 ** bits).sum())
    assert np.array_equal(pk.cpu().numpy()[0], np.abs(yd).max(axis=0))


def test_convert_track_to_pcm_device():
    from test_plugin_layer import music_like
    x = np.stack([music_like(5000, 2, 44100, 40 + s) for s in range(2)]).astype(np.float32)
    x *= 1.2 / np.abs(x).max()                                                          # overshoots full scale
    t = torch.from_numpy(x).cuda()
    y = F.Resampler(44100, 48000, nch=2, nstreams=2).convert_track_device(t)
    want = F.finish_device(y, F.RRX_FMT_S24_3, gain=0.9, dither=True, seed=3)
    got = F.Resampler(44100, 48000, nch=2, nstreams=2).convert_track_to_pcm_device(t, F.RRX_FMT_S24_3, gain=0.9, dither=True, seed=3)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert tuple(got[0].shape) == (2, y.shape[1], 6)
    m = M.model(y.cpu().numpy(), F.RRX_FMT_S24_3, np.full(2, 0.9), True, 3)
    assert np.array_equal(got[0].cpu().numpy(), m[0])
    assert np.array_equal(got[2].cpu().numpy().view(np.uint64), m[2]) and int(got[2].sum()) > 0
    assert np.array_equal(got[1].cpu().numpy().view(np.uint64), m[1])
