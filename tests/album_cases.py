"""Cases shared by the gapless-album tests (tests/test_tracks_album_api.py on the host, tests/test_gpu_tracks_album*.py on the
device): rate pairs, albums, sources in the four formats, and the table of the header's stream-taking entry points."""
import os
import re

import numpy as np

import album_model as AM
import foo_dsp_resampler_amd as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = [(44100, 48000), (44100, 96000), (48000, 44100), (96000, 44100), (44100, 88200)]
FORMATS = [F.RRX_FMT_FLOAT, F.RRX_FMT_S16, F.RRX_FMT_S24_3, F.RRX_FMT_S32]

# (lengths, groups) of the planner tests.  n_add is 2205 at 44.1 kHz and 2400 at 48 kHz.
PLANS = {
    "ordinary": ([20011, 30000, 17003], [0, 0, 0]),
    "short-tracks": ([5000, 0, 1, 40, 64, 65, 3000], [3, 3, 3, 3, 3, 3, 3]),
    "first-shorter-than-n_add": ([700, 9000, 100, 4000], [1, 1, 1, 1]),
    "interleaved": ([3000, 4001, 5000, 70, 2999, 0, 6000, 1234, 40], [-1, 7, 7, -1, 2, 2, 2, -5, -1]),
    "tiny-album": ([20, 30, 14, 5000], [4, 4, 4, -1]),                 # 64 frames in all: planned as singles
    "album-of-one": ([5000, 300], [0, 1]),
}


def header_text():
    with open(os.path.join(ROOT, "include", "ratelib_amd_album.h")) as f:
        return f.read()


def header_functions(text=None):
    """(every function the header declares, those whose parameter list names hip_stream)"""
    text = re.sub(r"/\*.*?\*/", "", header_text() if text is None else text, flags=re.S)
    protos = re.findall(r"^[A-Za-z_][\w \t\*]*?[ \t\*](RRX_\w+)[ \t]*\(([^;{}]*)\)\s*;", text, re.M)
    return sorted(n for n, _ in protos), sorted(n for n, args in protos if "hip_stream" in args)


# the stream-taking entry points and the wrapper of foo_dsp_resampler_amd/album.py that takes `stream=` for each: one gated case each
# in tests/test_gpu_tracks_album_stream.py
STREAM_WRAPPER_OF = {"RRX_tracks_stage_album_device": "tracks_stage_album_device",
                     "RRX_tracks_stage_album_window_device": "tracks_stage_album_window_device"}


def tile_samples():
    """kAlbumTileSamples of csrc/tracks_album.hpp: the samples of a row that one workgroup of the copy kernel looks at"""
    text = open(os.path.join(ROOT, "foo_dsp_resampler_amd", "csrc", "tracks_album.hpp")).read()
    vals = {}
    for name in ("kAlbumThreads", "kAlbumSteps"):
        vals[name] = int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    assert re.search(r"constexpr int kAlbumTileSamples = kAlbumThreads \* 4 \* kAlbumSteps;", text)
    return vals["kAlbumThreads"] * 4 * vals["kAlbumSteps"]


def rng(*key):
    return np.random.default_rng([20260401] + [int(k) for k in key])


def source(fmt, frames, nch, *key):
    """a packed source of `frames` frames in `fmt`: (the array as it is stored, the same as float32 [frames, nch])"""
    r = rng(fmt, frames, nch, *key)
    if fmt == F.RRX_FMT_FLOAT:
        x = (r.standard_normal((frames, nch)) * 0.3).astype(np.float32)
        return x, x
    if fmt == F.RRX_FMT_S16:
        x = r.integers(-2 ** 15, 2 ** 15, (frames, nch)).astype(np.int16)
    elif fmt == F.RRX_FMT_S32:
        x = r.integers(-2 ** 31, 2 ** 31, (frames, nch)).astype(np.int32)
    else:
        x = AM.pack_s24(r.integers(-2 ** 23, 2 ** 23, (frames, nch)))
    return x, AM.to_float(x, fmt)


def signals(frames, fs):
    """the three signals of the continuity tests, one channel: noise at 0.25 rms, a 1 kHz and a 10 kHz tone at 0.5"""
    t = np.arange(frames, dtype=np.float64)
    return {"noise": (rng(1, frames).standard_normal(frames) * 0.25).astype(np.float32).reshape(-1, 1),
            "1kHz": (0.5 * np.sin(2 * np.pi * 1000.0 * t / fs)).astype(np.float32).reshape(-1, 1),
            "10kHz": (0.5 * np.sin(2 * np.pi * 10000.0 * t / fs)).astype(np.float32).reshape(-1, 1)}
