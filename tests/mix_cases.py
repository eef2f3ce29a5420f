"""The case table of the channel-mixing tests (tests/test_tracks_mix_api.py, tests/test_gpu_tracks_mix.py): channel pairs with their
matrices, source formats, track lengths around the copy kernel's LDS tile, and sources with the formats' extremes planted."""
import functools
import os
import re

import numpy as np

import foo_dsp_resampler_amd as F
from test_plugin_layer import music_like

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS, FO = 44100, 48000
FMTS = [F.RRX_FMT_FLOAT, F.RRX_FMT_S16, F.RRX_FMT_S24_3, F.RRX_FMT_S32]
FMT_IDS = {F.RRX_FMT_FLOAT: "f32", F.RRX_FMT_S16: "s16", F.RRX_FMT_S24_3: "s24", F.RRX_FMT_S32: "s32"}
BITS = {F.RRX_FMT_S16: 15, F.RRX_FMT_S24_3: 23, F.RRX_FMT_S32: 31}
BYTES = {F.RRX_FMT_FLOAT: 4, F.RRX_FMT_S16: 2, F.RRX_FMT_S24_3: 3, F.RRX_FMT_S32: 4, F.RRX_FMT_DOUBLE: 8}
# the extremes of tests/test_gpu_tracks_pcm.py, and for float32 the two zeros, full scale and the smallest denormal
PLANTED = {F.RRX_FMT_S16: [-2 ** 15, 2 ** 15 - 1],
           F.RRX_FMT_S24_3: [-2 ** 23, 2 ** 23 - 1, -1],
           F.RRX_FMT_S32: [-2 ** 31, 2 ** 31 - 1, 2 ** 24 + 1, 2 ** 24 + 3, 2 ** 25 + 2],
           F.RRX_FMT_FLOAT: [-0.0, 0.0, 1.0, -1.0, 2.0 ** -149]}


def _matrices():
    rng = np.random.default_rng(20240611)
    perm = np.zeros((3, 3))
    perm[0, 2] = perm[1, 0] = perm[2, 1] = 1.0               # a permutation: every other coefficient is "not connected"
    six = np.array([[0.31, -0.27, 0.5 ** 0.5, 0.0, 1.0 / 3.0, -0.125]])  # (6 -> 1): the LFE stays unconnected
    dense = rng.standard_normal((16, 16)) / 4.0
    assert (dense != 0).all()
    return {"2to1": F.mix_matrix("stereo_to_mono"), "1to2": F.mix_matrix("mono_to_stereo"), "6to2": F.mix_matrix("5.1_to_stereo"),
            "3to3": perm, "6to1": six, "16to16": dense}


MATRICES = _matrices()
PAIRS = list(MATRICES)


def tile_bytes():
    """kMixTileBytes of csrc/tracks_mix.hpp: the source bytes of one LDS tile of the copy kernels"""
    text = open(os.path.join(ROOT, "foo_dsp_resampler_amd", "csrc", "tracks_mix.hpp")).read()
    return int(re.search(r"kMixTileBytes\s*=\s*(\d+)", text).group(1))


def tile_frames(fmt, nch_src):
    """mix_tile_frames of csrc/tracks_mix.hpp: kMixTileBytes / (nch_src * bytes of a sample)"""
    return tile_bytes() // (nch_src * BYTES[fmt])


def lengths(fmt, nch_src):
    """both sides of the 64-frame LPC branch, both sides of prime_len (2205), and one frame under, at and over one tile and two
    tiles of the copy kernel; with 3-, 9- and 18-byte S24 frames the odd lengths make tracks begin at every byte offset mod 4"""
    t = tile_frames(fmt, nch_src)
    return (40, 65, 101, 2205, 2207, t - 1, t, t + 1, 2 * t - 1, 2 * t, 2 * t + 1)


def to_raw(values, fmt):
    """samples [frames, nch] (integers, or floats for RRX_FMT_FLOAT) -> the array the call takes"""
    if fmt == F.RRX_FMT_FLOAT:
        return np.ascontiguousarray(values, np.float32)
    if fmt == F.RRX_FMT_S16:
        return values.astype(np.int16)
    if fmt == F.RRX_FMT_S32:
        return values.astype(np.int32)
    u = (values & 0xffffff).astype(np.uint32)
    return np.stack([u & 0xff, (u >> 8) & 0xff, u >> 16], axis=-1).astype(np.uint8).reshape(values.shape[0], -1)


@functools.lru_cache(maxsize=None)
def tracks(fmt, nch, lens):
    """music_like at half of full scale (rounded, for the integer formats) as raw arrays, read-only.  The format's extremes are
    planted in the LPC base frames of the first track longer than prime_len and in the longest track: at its head, in its
    middle and at its end."""
    out = []
    first_long = min([n for n in lens if n > 2205], default=None)
    for i, n in enumerate(lens):
        x = music_like(n, nch, FS, 70 + i).astype(np.float64) * 0.5
        v = x.astype(np.float32) if fmt == F.RRX_FMT_FLOAT else np.rint(x * 2.0 ** BITS[fmt]).astype(np.int64)
        if n == max(lens) or n == first_long:
            flat = v.reshape(-1)
            p = PLANTED[fmt]
            for at in (7, flat.size // 2, flat.size // 2 + 101, flat.size - 9):
                flat[at:at + len(p)] = p
        raw = to_raw(v, fmt)
        raw.setflags(write=False)
        out.append(raw)
    return tuple(out)
