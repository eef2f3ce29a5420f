"""A library on ONE handle (Resampler.convert_library_to_pcm; DESIGN.md 11, "Libraries"): length-sorted batches, a reset between
them, row buffers reused -- against convert_tracks_to_pcm_device of every batch on a FRESH handle, which tests/test_gpu_tracks*.py
hold on their own.  The bar is equality of bytes, peaks and clip counts."""
import functools

import numpy as np
import pytest

import foo_dsp_resampler_amd as F
from test_plugin_layer import music_like

pytestmark = pytest.mark.gpu

FS, FO, NCH = 44100, 48000, 2
LENGTHS = [0, 40, 64, 65, 3000, 20011, 50000]
GAINS = [1.0, 0.5, 6.0, 1.0, 0.25, 6.0, 1.5]          # (6.0 on a track that peaks at 0.3 of full scale: clipped samples to count)
SEED = 0x1234567887654321
K = 0xBF58476D1CE4E5B9


@functools.lru_cache(maxsize=None)
def host_tracks():
    """seven stereo S16 tracks at half of full scale, read-only"""
    out = []
    for i, n in enumerate(LENGTHS):
        v = np.rint(music_like(n, NCH, FS, 70 + i).astype(np.float64) * 0.5 * 2.0 ** 15).astype(np.int16).reshape(n, NCH)
        v.setflags(write=False)
        out.append(v)
    return tuple(out)


def device_tracks():
    import torch
    t = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in host_tracks()]
    torch.cuda.synchronize()
    return t


def as_host(views, peak, clipped):
    import torch
    torch.cuda.synchronize()
    return [v.cpu().numpy().tobytes() for v in views], peak.cpu().numpy().copy(), clipped.cpu().numpy().copy()


@functools.lru_cache(maxsize=None)
def reference():
    """every batch of the 3-stream split on a fresh handle, finished with the batch's seed: per track, in the caller's order"""
    import torch
    tracks = device_tracks()
    tb = F.tracks_batches(FS, FO, LENGTHS, 3)
    assert tb.batches == [[6, 5, 4], [3, 2, 1], [0]]
    raw, peak, clipped = [None] * 7, np.zeros((7, NCH)), np.zeros((7, NCH), np.int64)
    for b, idx in enumerate(tb.batches):
        r = F.Resampler(FS, FO, nch=NCH, nstreams=3)
        gain = torch.tensor([GAINS[i] for i in idx], dtype=torch.float64, device="cuda")
        v, p, c = r.convert_tracks_to_pcm_device([tracks[i] for i in idx], F.RRX_FMT_S24_3, gain=gain, dither=True,
                                                 seed=(SEED + b * 3 * NCH * K) % 2 ** 64)
        v, p, c = as_host(v, p, c)
        r.close()
        for k, i in enumerate(idx):
            raw[i], peak[i], clipped[i] = v[k], p[k], c[k]
    assert [len(x) for x in raw] == [F.track_geometry(FS, FO, n)[3] * NCH * 3 for n in LENGTHS]
    assert clipped.sum() > 0 and clipped[0].sum() == 0 and peak[6].min() > 0
    return raw, peak, clipped


def library(nstreams, **kw):
    r = F.Resampler(FS, FO, nch=NCH, nstreams=nstreams)
    out = as_host(*r.convert_library_to_pcm(device_tracks(), F.RRX_FMT_S24_3, gain=GAINS, dither=True, seed=SEED, **kw))
    return r, out


def assert_same(got, want, what):
    for i in range(7):
        assert len(got[0][i]) == len(want[0][i]), (what, i)
        assert got[0][i] == want[0][i], (what, "bytes of track", i)
    assert np.array_equal(got[1], want[1]), what
    assert np.array_equal(got[2], want[2]), what


def test_library_equals_its_batches_on_fresh_handles():
    r, got = library(3)
    assert_same(got, reference(), "3 streams")
    # a second run on the same handle, which the first one left drained
    again = as_host(*r.convert_library_to_pcm(device_tracks(), F.RRX_FMT_S24_3, gain=GAINS, dither=True, seed=SEED))
    assert_same(again, reference(), "second run")
    r.close()


def test_library_bytes_do_not_depend_on_the_stream_count():
    r, got = library(2)
    assert_same(got, reference(), "2 streams")
    r.close()


def test_library_by_windows_gives_the_same_bytes():
    r, got = library(3, window=4096)
    assert_same(got, reference(), "windows of 4096")
    again = as_host(*r.convert_library_to_pcm(device_tracks(), F.RRX_FMT_S24_3, window=4096, gain=GAINS, dither=True, seed=SEED))
    assert_same(again, reference(), "windows, second run")
    r.close()


def test_library_on_a_handle_that_is_in_the_middle_of_a_stream():
    """a handle with frames pushed and not pulled: the first batch is preceded by a reset, too"""
    import torch
    r = F.Resampler(FS, FO, nch=NCH, nstreams=3)
    x = torch.full((3, 30000, NCH), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.push_device(x, 30000, stride=30000)
    assert r.available > 0
    got = as_host(*r.convert_library_to_pcm(device_tracks(), F.RRX_FMT_S24_3, gain=GAINS, dither=True, seed=SEED))
    assert_same(got, reference(), "after a push of NaN")
    r.close()
