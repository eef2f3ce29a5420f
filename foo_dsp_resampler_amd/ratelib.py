"""ctypes mirror of include/ratelib.h + include/ratelib_amd.h (same names, argument meaning and
error behaviour as the reference's rate/ratelib.h:25-81)."""
import ctypes as C
import json
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
RR_BEST, RR_NORM = 0, 1

# every symbol the two public headers declare
EXPECTED_SYMBOLS = [
    "init_ratelib", "close_ratelib", "RR_open", "RR_flow", "RR_push", "RR_pull", "RR_drain", "RR_close", "RR_strerror",
    "RRX_open_batch", "RRX_open_batch_on", "RRX_device", "RRX_push_device", "RRX_pull_device", "RRX_flow_device", "RRX_push_strided", "RRX_pull_strided",
    "RRX_set_stream", "RRX_sync", "RRX_profile", "RRX_profile_read", "RRX_profile_report", "RRX_debug_fail_alloc",
    "RRX_debug_tile_walk", "RRX_debug_walk_start", "RRX_debug_window_start",
    "RRX_open_batch_fmt", "RRX_format", "RRX_push_double", "RRX_pull_double", "RRX_flow_double", "RRX_push_device_double",
    "RRX_pull_device_double", "RRX_flow_device_double",
    "RRX_push_samples", "RRX_pull_samples", "RRX_flow_samples", "RRX_push_device_samples", "RRX_pull_device_samples",
    "RRX_flow_device_samples",
    "RRX_lpc_extrapolate_device", "RRX_edge_geometry",
    "RRX_finish_device", "RRX_debug_finish_host",
    "RRX_finish_shaped_device", "RRX_debug_finish_shaped_host", "RRX_tracks_finish_shaped_device",
    "RRX_true_peak_device", "RRX_debug_true_peak_host", "RRX_tracks_true_peak_device",
    "RRX_limit_work_doubles", "RRX_limit_device", "RRX_tracks_limit_device", "RRX_debug_limit_host",
    "RRX_limit_release_work_doubles", "RRX_limit_release_device", "RRX_tracks_limit_release_device", "RRX_debug_limit_release_host",
    "RRX_loudness_device", "RRX_loudness_work_doubles", "RRX_debug_loudness_host", "RRX_tracks_loudness_device",
    "RRX_loudness_gate_device", "RRX_debug_loudness_gate_host",
    "RRX_loudness_blocks_device", "RRX_loudness_groups_work_doubles", "RRX_loudness_gate_groups_device", "RRX_loudness_range_groups_device",
    "RRX_debug_loudness_blocks_host", "RRX_debug_loudness_gate_groups_host", "RRX_debug_loudness_range_groups_host",
    "RRX_track_geometry", "RRX_tracks_plan", "RRX_tracks_stage_device", "RRX_tracks_finish_device",
    "RRX_tracks_stage_device_samples", "RRX_debug_tracks_load_host",
    "RRX_tracks_stage_window_device", "RRX_tracks_finish_window_device", "RRX_debug_tracks_window_cut",
    "RRX_tracks_finish_shaped_window_device", "RRX_debug_tracks_finish_shaped_window_host",
    "RRX_tracks_true_peak_packed_device", "RRX_debug_tracks_true_peak_packed_host",
    "RRX_tracks_loudness_packed_device", "RRX_debug_tracks_loudness_packed_host",
    "RRX_tracks_true_peak_window_device", "RRX_debug_tracks_true_peak_window_host", "RRX_tracks_loudness_window_work_doubles",
    "RRX_tracks_loudness_window_device", "RRX_debug_tracks_loudness_window_host",
    "RRX_limit_window_reach", "RRX_tracks_limit_window_work_doubles", "RRX_tracks_limit_window_device", "RRX_debug_tracks_limit_window_host",
    "RRX_tracks_limit_release_window_work_doubles", "RRX_tracks_limit_release_window_device", "RRX_debug_tracks_limit_release_window_host",
    "RRX_isamp_max", "RRX_available", "RRX_channels", "RRX_streams",
    "RRX_describe_plan", "RRX_describe_dispatch", "RRX_plan_table",
    "RRX_reset", "RRX_tracks_batches", "RRX_plan_cache_clear", "RRX_plan_cache_stats",
    "RRX_mix_device", "RRX_debug_mix_host", "RRX_tracks_stage_mix_device", "RRX_tracks_stage_mix_window_device", "RRX_debug_tracks_mix_host",
]
RRX_FMT_FLOAT, RRX_FMT_DOUBLE = 0, 1  # sample formats of a handle (ratelib_amd.h)
RRX_FMT_S16, RRX_FMT_S32 = 16, 32      # interleaved signed integer PCM (24-bit audio left-justified in S32)
RRX_FMT_S24_3 = 24                     # packed 3-byte PCM: a destination of finish_device and a source of tracks_stage_device, never a handle format
_FMT_DTYPE = {RRX_FMT_FLOAT: np.dtype(np.float32), RRX_FMT_DOUBLE: np.dtype(np.float64), RRX_FMT_S16: np.dtype(np.int16),
              RRX_FMT_S32: np.dtype(np.int32)}
_DTYPE_FMT = {d: f for f, d in _FMT_DTYPE.items()}
RRX_SHAPE_MAX_ORDER = 16
RRX_MIX_MAX_CH = 16


def _mix_matrices():
    h = 0.5 ** 0.5
    m = {"stereo_to_mono": [[0.5, 0.5]],
         "mono_to_stereo": [[1.0], [1.0]],
         "swap": [[0.0, 1.0], [1.0, 0.0]],
         "mid_side": [[0.5, 0.5], [0.5, -0.5]],
         "5.1_to_stereo": [[1.0, 0.0, h, 0.0, h, 0.0], [0.0, 1.0, h, 0.0, 0.0, h]],
         "7.1_to_stereo": [[1.0, 0.0, h, 0.0, h, 0.0, h, 0.0], [0.0, 1.0, h, 0.0, 0.0, h, 0.0, h]]}
    out = {}
    for k, v in m.items():
        out[k] = np.array(v, dtype=np.float64)
        out[k].setflags(write=False)
    return out


MIX_MATRICES = _mix_matrices()
"""Channel-mixing matrices (mix_device, tracks_stage_mix_device, `mix=`): float64 [nch_dst, nch_src], rows are output channels,
WAVE channel order (FL FR FC LFE BL BR [SL SR]).  "mid_side" is M = (L + R) / 2, S = (L - R) / 2.  The two surround downmixes are
ITU-R BS.775's: front at 1.0, centre and surrounds at sqrt(0.5), and the LFE NOT CONNECTED -- its coefficient is zero, and a zero
coefficient leaves the term out of the sum (ratelib_amd.h), so nothing the LFE holds reaches the output.  A full-scale source can
clip through them: mix_matrix(name, normalize=True)."""

NOISE_SHAPES = {
    "lipshitz5": (2.033, -2.165, 1.959, -1.590, 0.6149),
    "wannamaker3": (1.623, -0.982, 0.109),
    "wannamaker9": (2.412, -3.370, 3.937, -4.174, 3.353, -2.205, 1.281, -0.569, 0.0847),
}
"""Error-feedback filters for noise-shaped dither (finish_shaped_device, `shaping=`): the published 44.1 kHz designs -- Lipshitz's
5-tap improved E-weighted filter and Wannamaker's 3-tap and 9-tap F-weighted filters.  They spare the ear's most sensitive band
at 44.1 kHz only; for another rate the caller brings coefficients: wherever a name is accepted, so is any sequence of 1 to 16
finite floats."""

RRX_TP_MAX_PHASES, RRX_TP_MAX_TAPS = 8, 16
RRX_LIMIT_MAX_LOOKAHEAD, RRX_LIMIT_MAX_HOLD = 1024, 4096
RRX_LIMIT_RELEASE_MIN_BLOCK, RRX_LIMIT_RELEASE_MAX_BLOCK = 64, 65536
RRX_LIMIT_RELEASE_WIN_STATE = 8  # doubles of scan state per track between two windows (tracks_limit_release_window_device)
RRX_LOUDNESS_WIN_STATE = 16            # doubles per (track, channel) of tracks_loudness_window_device's state: S, Z, C, E, three zeros


def _bs1770():
    p0 = (14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68)
    p1 = (-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155)
    return 4, 12, tuple(v / 8192.0 for p in (p0, p1, p1[::-1], p0[::-1]) for v in p)


TRUE_PEAK_FILTERS = {"bs1770": _bs1770()}
"""Oversampling filters for true_peak_device (`filter=`) as (phases, taps, phases * taps coefficients, phase-major).  "bs1770" is
the 4 x 12 interpolator of ITU-R BS.1770-4 Annex 2, numerators over 8192: phases 2 and 3 are phases 1 and 0 reversed, the
interleaved prototype h[4k + p] = coefs[p][k] is symmetric, and the centre tap of phase 0 is 7964 / 8192, so the true peak of a
signal can lie under its sample peak.  Wherever a name is accepted, so is a tuple (phases, taps, coefficients) with 1..8 phases,
1..16 taps and finite floats: the library designs no filter."""


class RRConfig(C.Structure):
    """RR_config, rate/ratelib.h:53-63."""
    _fields_ = [("in_rate", C.c_size_t), ("out_rate", C.c_size_t), ("phase", C.c_double),
                ("bandwidth", C.c_double), ("allow_aliasing", C.c_int), ("quality", C.c_int)]


class WalkGeom(C.Structure):
    """RRX_walk_geom (ratelib_amd.h): geometry of a fused launch's polyphase stage, for RRX_debug_tile_walk."""
    _fields_ = [("at0", C.c_longlong), ("b_offset", C.c_longlong), ("B0", C.c_longlong)] + [
        (k, C.c_int) for k in ("V", "polyL", "step", "n", "KS", "qb_min", "qb_max", "two_round", "ra_end", "rb_start", "nsub", "Vs")]


class RRXTrack(C.Structure):
    """RRX_track (ratelib_amd.h): where one track of a ragged batch lies, all in frames."""
    _fields_ = [(k, C.c_ulonglong) for k in ("src_first", "frames", "lead", "out_first", "out_frames", "dst_first")]


class WalkStartWave(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("n", "g", "pc", "pend")]


class WalkStartRound(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("kb", "ke", "cnt", "b1", "b2")] + [("p0", C.c_int * 3), ("pend", C.c_int * 3), ("pad", C.c_int),
                                                                         ("wave", WalkStartWave * 4)]


class WalkStart(C.Structure):
    """RRX_walk_start (ratelib_amd.h): the start states of one block's tile walk, for RRX_debug_walk_start."""
    _fields_ = [("round", WalkStartRound * 2)]


class RRError(RuntimeError):
    def __init__(self, code, what):
        self.code = code
        super().__init__("%s failed: %d (%s)" % (what, code, lib().RR_strerror(code).decode()))


def lib_path():
    # RATELIB_AMD_SO: another in-tree build of the same library (kernel experiments: tools/build_variant.sh)
    return os.environ.get("RATELIB_AMD_SO") or os.path.join(HERE, "libratelib_amd.so")


_lib = None
_ALLOC_CB = C.CFUNCTYPE(None)


alloc_handler_calls = 0  # how often the library ran the registered allocation-failure handler (xmalloc.c:38-43)


def _alloc_failed():
    # The plugin's handler throws std::bad_alloc through the C frames; a Python callback cannot unwind C, so this one
    # only counts -- the failing call still returns RR_ENOMEM, which _check() raises as RRError.
    global alloc_handler_calls
    alloc_handler_calls += 1


_alloc_cb = _ALLOC_CB(_alloc_failed)
_inited = False


def _share_hip_runtime_with_torch():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so / libhsa-runtime64.so and load them by file
    name; a process that also loads /opt/rocm's copy ends up with two HSA runtimes and the second one
    finds no device.  Loading torch's copy first (same SONAME, libamdhip64.so.7) makes the dynamic
    linker bind libratelib_amd.so to it, so torch tensors and this engine share one runtime.  Without
    torch installed the system runtime is used."""
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.origin:
            return None
        p = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(p):
            return C.CDLL(p, mode=C.RTLD_GLOBAL)
    except Exception:
        pass
    return None


_hip_rt = None


def lib():
    """Load the shared library (raises if it has not been built: there is no fallback)."""
    global _lib, _hip_rt
    if _lib is None:
        p = lib_path()
        if not os.path.exists(p):
            raise RuntimeError("libratelib_amd.so is not built; run `python -m foo_dsp_resampler_amd.build`")
        _hip_rt = _share_hip_runtime_with_torch()
        L = C.CDLL(p)
        P = C.POINTER
        vp, sz, u64 = C.c_void_p, C.c_size_t, C.c_ulonglong
        L.init_ratelib.argtypes = [_ALLOC_CB]
        L.RR_open.argtypes = [P(RRConfig), C.c_int, P(vp)]
        L.RRX_open_batch.argtypes = [P(RRConfig), C.c_int, C.c_int, P(vp)]
        L.RRX_open_batch_on.argtypes = [P(RRConfig), C.c_int, C.c_int, C.c_int, P(vp)]
        L.RRX_device.argtypes = [vp]
        L.RRX_open_batch_fmt.argtypes = [P(RRConfig), C.c_int, C.c_int, C.c_int, C.c_int, P(vp)]
        L.RRX_format.argtypes = [vp]
        L.RRX_push_double.argtypes = [vp, vp, sz, sz]
        L.RRX_pull_double.argtypes = [vp, vp, sz, sz, P(sz)]
        L.RRX_flow_double.argtypes = [vp, vp, sz, vp, sz, sz, sz, P(sz), P(sz)]
        L.RRX_push_device_double.argtypes = [vp, vp, sz, sz]
        L.RRX_pull_device_double.argtypes = [vp, vp, sz, sz, P(sz)]
        L.RRX_flow_device_double.argtypes = [vp, vp, sz, vp, sz, sz, sz, P(sz), P(sz)]
        L.RRX_push_samples.argtypes = [vp, C.c_int, vp, sz, sz]
        L.RRX_pull_samples.argtypes = [vp, C.c_int, vp, sz, sz, P(sz)]
        L.RRX_flow_samples.argtypes = [vp, C.c_int, vp, sz, vp, sz, sz, sz, P(sz), P(sz)]
        L.RRX_push_device_samples.argtypes = [vp, C.c_int, vp, sz, sz]
        L.RRX_pull_device_samples.argtypes = [vp, C.c_int, vp, sz, sz, P(sz)]
        L.RRX_flow_device_samples.argtypes = [vp, C.c_int, vp, sz, vp, sz, sz, sz, P(sz), P(sz)]
        L.RR_push.argtypes = [vp, vp, sz]
        L.RR_pull.argtypes = [vp, vp, sz, P(sz)]
        L.RR_flow.argtypes = [vp, vp, vp, sz, sz, P(sz), P(sz)]
        L.RR_drain.argtypes = [vp]
        L.RR_close.argtypes = [P(vp)]
        L.RR_close.restype = None
        L.RR_strerror.argtypes = [C.c_int]
        L.RR_strerror.restype = C.c_char_p
        L.RRX_push_device.argtypes = [vp, vp, sz, sz]
        L.RRX_pull_device.argtypes = [vp, vp, sz, sz, P(sz)]
        L.RRX_flow_device.argtypes = [vp, vp, sz, vp, sz, sz, sz, P(sz), P(sz)]
        L.RRX_push_strided.argtypes = [vp, vp, sz, sz]
        L.RRX_pull_strided.argtypes = [vp, vp, sz, sz, P(sz)]
        L.RRX_set_stream.argtypes = [vp, vp]
        L.RRX_sync.argtypes = [vp]
        L.RRX_profile.argtypes = [vp, C.c_int]
        L.RRX_profile_read.argtypes = [vp, P(C.c_double), P(C.c_longlong), P(C.c_double), P(C.c_longlong)]
        L.RRX_profile_report.argtypes = [vp, C.c_char_p, sz]
        L.RRX_debug_fail_alloc.argtypes = [C.c_int]
        L.RRX_debug_fail_alloc.restype = None
        if hasattr(L, "RRX_debug_tile_walk"):  # (a RATELIB_AMD_SO build of an older tree, in A/B runs, has none)
            L.RRX_debug_tile_walk.argtypes = [P(WalkGeom), C.c_int, P(C.c_longlong), vp, sz]
            L.RRX_debug_tile_walk.restype = C.c_longlong
        if hasattr(L, "RRX_debug_walk_start"):  # (likewise)
            L.RRX_debug_walk_start.argtypes = [P(WalkGeom), C.c_int, P(WalkStart)]
        if hasattr(L, "RRX_debug_window_start"):  # (likewise)
            L.RRX_debug_window_start.argtypes = [P(WalkGeom), C.c_int, C.c_int, P(C.c_int), P(C.c_int), P(C.c_uint)]
        for n in ("RRX_isamp_max", "RRX_available"):
            getattr(L, n).argtypes = [vp]
            getattr(L, n).restype = sz
        L.RRX_channels.argtypes = [vp]
        L.RRX_streams.argtypes = [vp]
        L.RRX_describe_plan.argtypes = [P(RRConfig), C.c_char_p, sz]
        L.RRX_describe_dispatch.argtypes = [P(RRConfig), C.c_int, C.c_char_p, sz]
        L.RRX_plan_table.argtypes = [P(RRConfig), C.c_int, vp, sz, P(sz)]
        if hasattr(L, "RRX_lpc_extrapolate_device"):  # (as above: an older tree's build has none)
            L.RRX_lpc_extrapolate_device.argtypes = [C.c_int, vp, vp, sz, C.c_int, sz, C.c_int, C.c_int, sz, sz]
            L.RRX_edge_geometry.argtypes = [sz, sz, P(sz), P(sz), P(sz), P(sz)]
        if hasattr(L, "RRX_finish_device"):  # (as above)
            host = [C.c_int, vp, sz, C.c_int, vp, sz, C.c_int, sz, C.c_int, vp, C.c_int, u64, u64, vp, vp]
            L.RRX_finish_device.argtypes = [C.c_int, vp] + host
            L.RRX_debug_finish_host.argtypes = host
        if hasattr(L, "RRX_finish_shaped_device"):  # (as above)
            host = [C.c_int, vp, sz, C.c_int, vp, sz, C.c_int, sz, C.c_int, vp, C.c_int, u64, u64, vp, C.c_int, sz, vp, vp, vp, vp]
            L.RRX_finish_shaped_device.argtypes = [C.c_int, vp] + host
            L.RRX_debug_finish_shaped_host.argtypes = host
            L.RRX_tracks_finish_shaped_device.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, vp, sz, C.c_int, vp, sz, vp, C.c_int, u64,
                                                          vp, C.c_int, sz, vp, vp]
        if hasattr(L, "RRX_true_peak_device"):  # (as above)
            host = [C.c_int, vp, sz, C.c_int, sz, C.c_int, vp, u64, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
            L.RRX_true_peak_device.argtypes = [C.c_int, vp] + host
            L.RRX_debug_true_peak_host.argtypes = host
            L.RRX_tracks_true_peak_device.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, vp, sz, vp, vp, C.c_int, C.c_int, vp, vp]
        if hasattr(L, "RRX_limit_device"):  # (as above)
            host = [C.c_int, vp, sz, C.c_int, vp, sz, C.c_int, sz, C.c_int, vp, C.c_double, vp, C.c_int, C.c_int, sz, sz, vp, vp, vp, sz]
            L.RRX_limit_device.argtypes = [C.c_int, vp] + host
            L.RRX_debug_limit_host.argtypes = host
            L.RRX_tracks_limit_device.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, sz, vp, C.c_double, vp, C.c_int,
                                                  C.c_int, sz, sz, vp, vp, vp, sz]
            L.RRX_limit_work_doubles.argtypes = [C.c_int, sz, C.c_int, sz]
            L.RRX_limit_work_doubles.restype = sz
        if hasattr(L, "RRX_limit_release_device"):  # (as above)
            host = [C.c_int, vp, sz, C.c_int, vp, sz, C.c_int, sz, C.c_int, vp, C.c_double, vp, C.c_int, C.c_int, sz, sz, C.c_double, sz, vp, vp,
                    vp, sz]
            L.RRX_limit_release_device.argtypes = [C.c_int, vp] + host
            L.RRX_debug_limit_release_host.argtypes = host
            L.RRX_tracks_limit_release_device.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, sz, vp, C.c_double, vp,
                                                          C.c_int, C.c_int, sz, sz, C.c_double, sz, vp, vp, vp, sz]
            L.RRX_limit_release_work_doubles.argtypes = [C.c_int, sz, C.c_int, sz, sz]
            L.RRX_limit_release_work_doubles.restype = sz
        if hasattr(L, "RRX_loudness_device"):  # (as above)
            host = [C.c_int, vp, sz, C.c_int, sz, C.c_int, vp, u64, vp, sz, vp, vp, vp, sz, vp, sz]
            L.RRX_loudness_device.argtypes = [C.c_int, vp] + host
            L.RRX_debug_loudness_host.argtypes = host
            L.RRX_loudness_work_doubles.argtypes = [C.c_int, C.c_int, sz, sz]
            L.RRX_loudness_work_doubles.restype = sz
            L.RRX_tracks_loudness_device.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, vp, sz, vp, vp, sz, vp, sz, vp, vp, sz]
            host = [vp, sz, C.c_int, C.c_int, sz, vp, vp, sz, C.c_double, C.c_double, vp]
            L.RRX_loudness_gate_device.argtypes = [C.c_int, vp] + host
            L.RRX_debug_loudness_gate_host.argtypes = host
        if hasattr(L, "RRX_loudness_blocks_device"):  # (as above)
            host = [vp, sz, C.c_int, C.c_int, sz, vp, vp, sz, sz, sz, vp, sz, vp, vp]
            L.RRX_loudness_blocks_device.argtypes = [C.c_int, vp] + host
            L.RRX_debug_loudness_blocks_host.argtypes = host
            L.RRX_loudness_groups_work_doubles.argtypes = [C.c_int, C.c_int]
            L.RRX_loudness_groups_work_doubles.restype = sz
            host = [vp, sz, C.c_int, vp, vp, C.c_int, C.c_double, C.c_double, vp, vp, sz]
            L.RRX_loudness_gate_groups_device.argtypes = [C.c_int, vp] + host
            L.RRX_debug_loudness_gate_groups_host.argtypes = host
            host = [vp, sz, C.c_int, vp, vp, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, vp, vp, sz]
            L.RRX_loudness_range_groups_device.argtypes = [C.c_int, vp] + host
            L.RRX_debug_loudness_range_groups_host.argtypes = host
        if hasattr(L, "RRX_tracks_plan"):  # (as above)
            L.RRX_track_geometry.argtypes = [P(RRConfig), sz, P(sz), P(sz), P(sz), P(sz)]
            L.RRX_tracks_plan.argtypes = [P(RRConfig), P(sz), C.c_int, P(RRXTrack), P(sz), P(sz), P(sz), P(sz)]
            L.RRX_tracks_stage_device.argtypes = [C.c_int, vp, sz, sz, vp, C.c_int, C.c_int, vp, sz, vp, sz]
            L.RRX_tracks_finish_device.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, vp, sz, C.c_int, vp, sz, vp, C.c_int, u64, vp, vp]
        if hasattr(L, "RRX_tracks_stage_device_samples"):  # (as above)
            L.RRX_tracks_stage_device_samples.argtypes = [C.c_int, vp, sz, sz, vp, C.c_int, C.c_int, C.c_int, vp, sz, vp, sz]
            L.RRX_debug_tracks_load_host.argtypes = [C.c_int, vp, sz, sz, vp]
        if hasattr(L, "RRX_tracks_stage_window_device"):  # (as above)
            L.RRX_tracks_stage_window_device.argtypes = [C.c_int, vp, sz, sz, vp, C.c_int, C.c_int, C.c_int, vp, sz, sz, sz, sz, vp, sz]
            L.RRX_tracks_finish_window_device.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, vp, sz, sz, sz, sz, C.c_int, vp, sz, vp,
                                                          C.c_int, u64, vp, vp]
            L.RRX_debug_tracks_window_cut.argtypes = [P(RRXTrack), sz, sz, sz, C.c_int, sz, sz, P(u64), P(u64)]
        if hasattr(L, "RRX_tracks_finish_shaped_window_device"):  # (as above)
            host = [vp, C.c_int, C.c_int, C.c_int, vp, sz, sz, sz, sz, C.c_int, vp, sz, vp, C.c_int, u64, vp, C.c_int, sz, vp, vp, vp, vp]
            L.RRX_tracks_finish_shaped_window_device.argtypes = [C.c_int, vp] + host
            L.RRX_debug_tracks_finish_shaped_window_host.argtypes = host
        if hasattr(L, "RRX_tracks_true_peak_window_device"):  # (as above)
            host = [vp, C.c_int, C.c_int, C.c_int, vp, sz, sz, sz, sz, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]
            L.RRX_tracks_true_peak_window_device.argtypes = [C.c_int, vp] + host
            L.RRX_debug_tracks_true_peak_window_host.argtypes = host
            L.RRX_tracks_loudness_window_work_doubles.argtypes = [C.c_int, C.c_int, sz, sz]
            L.RRX_tracks_loudness_window_work_doubles.restype = sz
            host = [vp, C.c_int, C.c_int, C.c_int, vp, sz, sz, sz, sz, vp, vp, sz, vp, vp, vp, sz, vp, vp, sz]
            L.RRX_tracks_loudness_window_device.argtypes = [C.c_int, vp] + host
            L.RRX_debug_tracks_loudness_window_host.argtypes = host
        if hasattr(L, "RRX_tracks_true_peak_packed_device"):  # (as above)
            host = [vp, C.c_int, C.c_int, C.c_int, vp, sz, sz, vp, vp, C.c_int, C.c_int, vp, vp]
            L.RRX_tracks_true_peak_packed_device.argtypes = [C.c_int, vp] + host
            L.RRX_debug_tracks_true_peak_packed_host.argtypes = host
            host = [vp, C.c_int, C.c_int, C.c_int, vp, sz, sz, vp, vp, sz, vp, sz, vp, vp, sz]
            L.RRX_tracks_loudness_packed_device.argtypes = [C.c_int, vp] + host
            L.RRX_debug_tracks_loudness_packed_host.argtypes = host
        if hasattr(L, "RRX_tracks_limit_window_device"):  # (as above)
            host = [vp, C.c_int, C.c_int, C.c_int, vp, sz, sz, sz, sz, sz, sz, C.c_int, vp, sz, vp, C.c_double, vp, C.c_int, C.c_int, sz, sz,
                    vp, vp, vp, sz]
            L.RRX_tracks_limit_window_device.argtypes = [C.c_int, vp] + host
            L.RRX_debug_tracks_limit_window_host.argtypes = host
            L.RRX_limit_window_reach.argtypes = [C.c_int, sz, sz, P(sz), P(sz)]
            L.RRX_tracks_limit_window_work_doubles.argtypes = [C.c_int, sz, C.c_int, sz, sz]
            L.RRX_tracks_limit_window_work_doubles.restype = sz
        if hasattr(L, "RRX_tracks_limit_release_window_device"):  # (as above)
            host = [vp, C.c_int, C.c_int, C.c_int, vp, sz, sz, sz, sz, sz, sz, C.c_int, vp, sz, vp, C.c_double, vp, C.c_int, C.c_int, sz, sz,
                    C.c_double, sz, vp, vp, vp, vp, vp, sz]
            L.RRX_tracks_limit_release_window_device.argtypes = [C.c_int, vp] + host
            L.RRX_debug_tracks_limit_release_window_host.argtypes = host
            L.RRX_tracks_limit_release_window_work_doubles.argtypes = [C.c_int, sz, C.c_int, sz, sz, sz]
            L.RRX_tracks_limit_release_window_work_doubles.restype = sz
        if hasattr(L, "RRX_mix_device"):  # (as above)
            host = [C.c_int, vp, sz, C.c_int, sz, C.c_int, vp, sz, C.c_int, vp]
            L.RRX_mix_device.argtypes = [C.c_int, vp] + host
            L.RRX_debug_mix_host.argtypes = host
            L.RRX_tracks_stage_mix_device.argtypes = [C.c_int, vp, sz, sz, vp, C.c_int, C.c_int, C.c_int, vp, sz, C.c_int, vp, vp, sz]
            L.RRX_tracks_stage_mix_window_device.argtypes = [C.c_int, vp, sz, sz, vp, C.c_int, C.c_int, C.c_int, vp, sz, C.c_int, vp, sz, sz, sz,
                                                             vp, sz]
            L.RRX_debug_tracks_mix_host.argtypes = [C.c_int, vp, C.c_int, sz, sz, C.c_int, vp, vp]
        if hasattr(L, "RRX_reset"):  # (as above)
            L.RRX_reset.argtypes = [vp]
            L.RRX_tracks_batches.argtypes = [P(RRConfig), P(sz), C.c_int, C.c_int, P(C.c_int), P(sz), P(C.c_int), P(u64), P(u64)]
            L.RRX_plan_cache_clear.argtypes = []
            L.RRX_plan_cache_clear.restype = None
            L.RRX_plan_cache_stats.argtypes = [P(u64), P(u64), P(C.c_int)]
        _lib = L
    return _lib


def available_symbols():
    L = lib()
    return [s for s in EXPECTED_SYMBOLS if hasattr(L, s)]


def _config(in_rate, out_rate, phase=50.0, bandwidth=95.0, allow_aliasing=0, quality=RR_BEST):
    return RRConfig(int(in_rate), int(out_rate), float(phase), float(bandwidth), int(allow_aliasing), int(quality))


def describe_plan(in_rate, out_rate, **kw):
    """Host-only: the stage chain the planner builds (dict).  Needs no GPU."""
    cfg = _config(in_rate, out_rate, **kw)
    buf = C.create_string_buffer(1 << 16)
    n = lib().RRX_describe_plan(C.byref(cfg), buf, len(buf))
    if n < 0:
        raise RRError(-n, "RRX_describe_plan")
    return json.loads(buf.value.decode())


def describe_dispatch(in_rate, out_rate, nch, **kw):
    """Host-only: the kernel form of the first stage pair on `nch`-channel handles (dict; RRX_describe_dispatch).  Needs no GPU."""
    cfg = _config(in_rate, out_rate, **kw)
    buf = C.create_string_buffer(1 << 14)
    n = lib().RRX_describe_dispatch(C.byref(cfg), int(nch), buf, len(buf))
    if n < 0:
        raise RRError(-n, "RRX_describe_dispatch")
    return json.loads(buf.value.decode())


def plan_table(which, in_rate, out_rate, **kw):
    """Host-only: designed table (0/1: DFT-stage taps, 2: polyphase table) as float64 array."""
    cfg = _config(in_rate, out_rate, **kw)
    n = C.c_size_t(0)
    rc = lib().RRX_plan_table(C.byref(cfg), which, None, 0, C.byref(n))
    if rc:
        raise RRError(rc, "RRX_plan_table")
    out = np.empty(n.value, dtype=np.float64)
    if n.value:
        lib().RRX_plan_table(C.byref(cfg), which, out.ctypes.data, n.value, C.byref(n))
    return out


def edge_geometry(in_rate, out_rate):
    """Host-only: the plugin's edge geometry for a rate pair, (n_add, n_drop, prime_len, inbuf) in frames (RRX_edge_geometry):
    frames to extrapolate at each end of the input, frames to cut from each end of the output, base frames the extrapolator
    looks at, the plugin's staging buffer.  Needs no GPU."""
    v = [C.c_size_t(0) for _ in range(4)]
    _check(lib().RRX_edge_geometry(int(in_rate), int(out_rate), *[C.byref(x) for x in v]), "RRX_edge_geometry")
    return tuple(x.value for x in v)


# -- the shared preludes of the handle-free wrappers: every rule of a call shape is written once, here.  A wrapper is its own scalar
# -- checks, these, the early return for empty input, and one C call.  The parts that touch `is_cuda` / `device` are functions of their
# -- own, so that a wrapper refuses its scalars first.
def _where(dev, stream):
    """(device index, stream pointer), the two leading arguments of every *_device call: `stream` is a hipStream_t as an integer or a
    torch stream, None / 0 the default stream"""
    return -1 if dev.index is None else int(dev.index), getattr(stream, "cuda_stream", stream) or 0


def _ptr(t):
    """the pointer argument of an optional tensor: null when it was not passed.  (ctypes takes the integer of data_ptr() for a void
    pointer as it is, so a tensor that is always there is passed as t.data_ptr().)"""
    return None if t is None else t.data_ptr()


_FLOAT_FMT = {}  # (by dtype object: str() of a torch dtype costs more than the rest of the lookup)


def _float_fmt(dtype):
    """the RRX_FMT_* of a float32 or float64 dtype (torch's, or its name); None for any other"""
    if dtype not in _FLOAT_FMT:
        _FLOAT_FMT[dtype] = {"float32": RRX_FMT_FLOAT, "float64": RRX_FMT_DOUBLE}.get(str(dtype).rpartition(".")[2])
    return _FLOAT_FMT[dtype]


def _frames_shape(x):
    """a [frames, nch] or [nstreams, frames, nch] source: (shape, nstreams, frames, nch)"""
    shape = tuple(x.shape)
    if len(shape) not in (2, 3):
        raise ValueError("expected a [frames, nch] or [nstreams, frames, nch] tensor, got shape %r" % (shape,))
    return (shape,) + ((1,) + shape if len(shape) == 2 else shape)


def _float_frames(x, who):
    """_frames_shape of a contiguous float32 or float64 source, for the pass `who`: (shape, RRX_FMT_*, nstreams, frames, nch).
    Touches neither the device nor the pointer: _on_device does, behind the caller's scalar checks."""
    shape, nstreams, frames, nch = _frames_shape(x)
    fmt = _float_fmt(x.dtype)
    if fmt is None:
        raise TypeError("%s buffer: %s reads float32 or float64 frames" % (x.dtype, who))
    if not x.is_contiguous():
        raise ValueError("the tensor must be contiguous")
    return shape, fmt, nstreams, frames, nch


def _on_device(x, who):
    """the device of the source of the pass `who`; TypeError for anything that is not a device tensor"""
    if not getattr(x, "is_cuda", False):
        raise TypeError("%s works on device tensors: the frames must be in HBM" % who)
    return x.device


def _tracks_frames(t, name, middle):
    """the rows, window or halo buffer of a per-track call, a contiguous float32 or float64 device tensor [ntracks, `middle`, nch]
    that the messages call `name`: (RRX_FMT_*, ntracks, frames a row, nch)"""
    fmt = _float_fmt(t.dtype)
    if t.dim() != 3 or fmt is None or not t.is_cuda or not t.is_contiguous():
        raise TypeError("%s must be a contiguous float32 or float64 device tensor [ntracks, %s, nch]" % (name, middle))
    ntracks, stride, nch = t.shape
    return fmt, ntracks, stride, nch


def _gain(gain, n, dev):
    """the gain of a call on `n` streams or tracks: None, or a float64 tensor [n] on `dev` -- made from a float, checked otherwise"""
    import torch
    if gain is not None and not hasattr(gain, "data_ptr"):
        gain = torch.full((n,), float(gain), dtype=torch.float64, device=dev)
    if gain is not None:
        if gain.dtype != torch.float64 or tuple(gain.shape) != (n,) or gain.device != dev or not gain.is_contiguous():
            raise TypeError("gain must be a float, or a contiguous float64 tensor [%d] on %s" % (n, dev))
    return gain


def _pcm_out(out, dst_format, lead, nch, dev):
    """the destination of an output stage, `lead` + (nch,) samples of `dst_format` (packed 24 bit: nch * 3 bytes): allocated when
    not passed, checked otherwise.  dst_format None measures only and takes no `out`.  (`out=False`, the measure-only form of the
    shaped calls, is the caller's to turn into None.)"""
    import torch
    if dst_format is None:
        if out is not None:
            raise ValueError("dst_format=None measures only: there is nothing to write into `out`")
        return None
    odt, last = {RRX_FMT_S16: (torch.int16, nch), RRX_FMT_S32: (torch.int32, nch), RRX_FMT_S24_3: (torch.uint8, nch * 3)}[dst_format]
    oshape = lead + (last,)
    if out is None:
        return torch.empty(oshape, dtype=odt, device=dev)
    if out.dtype != odt or tuple(out.shape) != oshape or out.device != dev or not out.is_contiguous():
        raise TypeError("out must be a contiguous %s tensor %r on %s" % (odt, oshape, dev))
    return out


def _finish_stats(peak, clipped, n, nch, dev):
    """the two statistics of an output stage, float64 and int64 [n, nch]: allocated (zeroed) when not passed, accumulated into
    otherwise"""
    import torch
    stats = []
    for t, sdt, name in ((peak, torch.float64, "peak"), (clipped, torch.int64, "clipped")):
        if t is None:
            t = torch.zeros((n, nch), dtype=sdt, device=dev)
        elif t.dtype != sdt or tuple(t.shape) != (n, nch) or t.device != dev or not t.is_contiguous():
            raise TypeError("%s must be a contiguous %s tensor [%d, %d] on %s" % (name, sdt, n, nch, dev))
        stats.append(t)
    return stats


def _true_peak_stats(true_peak, peak, n, nch, dev):
    """the two result tensors of a true-peak call: float64 [n, nch], allocated (zeroed) when not passed"""
    import torch
    stats = []
    for t, name in ((true_peak, "true_peak"), (peak, "peak")):
        if t is None:
            t = torch.zeros((n, nch), dtype=torch.float64, device=dev)
        elif t.dtype != torch.float64 or tuple(t.shape) != (n, nch) or t.device != dev or not t.is_contiguous():
            raise TypeError("%s must be a contiguous float64 tensor [%d, %d] on %s" % (name, n, nch, dev))
        stats.append(t)
    return stats


def _stream_state(state, nstreams, nch, width, dev):
    """the state a chunked per-stream call takes: None, or float64 [nstreams, nch, width] on `dev`"""
    import torch
    if state is not None:
        if state.dtype != torch.float64 or tuple(state.shape) != (nstreams, nch, width) or state.device != dev or not state.is_contiguous():
            raise TypeError("state must be a contiguous float64 tensor [%d, %d, %d] on %s" % (nstreams, nch, width, dev))


def _state_pair(state, state_out, sshape, dev):
    """the state a per-track window call reads and the one it writes, each None or float64 `sshape` on `dev`, and never one tensor"""
    import torch
    for t, name in ((state, "state"), (state_out, "state_out")):
        if t is not None and (t.dtype != torch.float64 or tuple(t.shape) != sshape or t.device != dev or not t.is_contiguous()):
            raise TypeError("%s must be a contiguous float64 tensor %r on %s" % (name, sshape, dev))
    if state is not None and state_out is not None and state_out.data_ptr() == state.data_ptr():
        raise ValueError("the call must not read and write one state tensor")


def _seed_and_first(seed, first_frame, frames):
    seed, first_frame = int(seed), int(first_frame)
    if not (0 <= seed < 1 << 64 and 0 <= first_frame and first_frame + frames < 1 << 64):
        raise ValueError("seed and first_frame + frames must fit 64 unsigned bits")
    return seed, first_frame


def _first_frame(first_frame, frames):
    first_frame = int(first_frame)
    if not (0 <= first_frame and first_frame + frames < 1 << 64):
        raise ValueError("first_frame + frames must fit 64 unsigned bits")
    return first_frame


def _shaped_dst_format(dst_format):
    if dst_format not in (RRX_FMT_S16, RRX_FMT_S24_3, RRX_FMT_S32):
        raise ValueError("unknown dst_format %r (RRX_FMT_S16, RRX_FMT_S24_3 or RRX_FMT_S32; out=False measures only)" % (dst_format,))


def lpc_extrapolate_device(t, first, data_len, extra_bkwd, extra_fwd, order=32, stream=None):
    """LPC edge extrapolation in place on the device (RRX_lpc_extrapolate_device; lpc_extrapolate2 of lpc/lpc.h:27, bit for bit).

    `t` is a contiguous float32 device tensor [frames, nch] or [nstreams, frames, nch]; the base data are the `data_len` frames
    from frame `first` of every stream.  Frames [first - extra_bkwd, first) and [first + data_len, first + data_len + extra_fwd)
    are overwritten, nothing else.  `stream`: a hipStream_t as an integer or a torch stream (None / 0 = the default stream); the
    call only enqueues, and the ordering against work on other streams is the caller's (ratelib_amd.h)."""
    _, nstreams, frames, nch = _frames_shape(t)
    if not str(t.dtype).endswith("float32"):
        raise TypeError("%s buffer: the LPC extrapolator works on float32 frames only" % (t.dtype,))
    if not t.is_contiguous():
        raise ValueError("the tensor must be contiguous")
    first, data_len, extra_bkwd, extra_fwd = int(first), int(data_len), int(extra_bkwd), int(extra_fwd)
    if min(first, data_len, extra_bkwd, extra_fwd) < 0 or first < extra_bkwd or first + data_len + extra_fwd > frames:
        raise ValueError("frames [%d, %d) do not lie inside the tensor's %d frames"
                         % (first - extra_bkwd, first + data_len + extra_fwd, frames))
    _ensure_init()
    _check(lib().RRX_lpc_extrapolate_device(*_where(t.device, stream), t.data_ptr() + first * nch * 4, frames, nstreams,
                                            data_len, nch, int(order), extra_bkwd, extra_fwd), "RRX_lpc_extrapolate_device")


def finish_device(x, dst_format, gain=None, dither=False, seed=0, first_frame=0, out=None, peak=None, clipped=None, stream=None):
    """The output stage on the device (RRX_finish_device): gain, TPDF dither, quantisation to integer PCM, peak and clip count.

    `x` is a contiguous float32 or float64 device tensor [frames, nch] or [nstreams, frames, nch].  `dst_format` is RRX_FMT_S16
    (int16 out), RRX_FMT_S32 (int32), RRX_FMT_S24_3 (uint8 [..., frames, nch * 3]: packed little-endian 24 bit) or None: measure
    only, nothing is written and the statistics are those of the S32 quantiser.  `gain`: None, a float, or a float64 device
    tensor [nstreams].  `seed` / `first_frame` (64-bit unsigned) fix the dither: a track finished in chunks with first_frame =
    the frames done so far gets the bits of one call.  `out`, `peak` (float64 [nstreams, nch]) and `clipped` (int64
    [nstreams, nch]) are allocated (the statistics zeroed) when not passed; statistics that are passed are accumulated into.
    Returns (out, peak, clipped).  `stream` as in lpc_extrapolate_device: the call only enqueues."""
    shape, fmt, nstreams, frames, nch = _float_frames(x, "the output stage")
    if dst_format not in (None, RRX_FMT_S16, RRX_FMT_S24_3, RRX_FMT_S32):
        raise ValueError("unknown dst_format %r (RRX_FMT_S16, RRX_FMT_S24_3, RRX_FMT_S32 or None)" % (dst_format,))
    seed, first_frame = _seed_and_first(seed, first_frame, frames)
    dev = _on_device(x, "the output stage")
    gain = _gain(gain, nstreams, dev)
    out = _pcm_out(out, dst_format, shape[:-1], nch, dev)
    peak, clipped = _finish_stats(peak, clipped, nstreams, nch, dev)
    _ensure_init()
    _check(lib().RRX_finish_device(*_where(dev, stream), fmt, x.data_ptr(), frames, dst_format or 0, _ptr(out), frames, nstreams, frames, nch,
                                   _ptr(gain), 1 if dither else 0, seed, first_frame, peak.data_ptr(), clipped.data_ptr()), "RRX_finish_device")
    return out, peak, clipped


def _shaping(shaping, segment):
    """`shaping` (a name of NOISE_SHAPES or 1..16 finite floats) as a ctypes array of doubles, and `segment` checked"""
    coefs = NOISE_SHAPES.get(shaping) if isinstance(shaping, str) else shaping
    if coefs is None:
        raise ValueError("unknown noise shape %r (one of %s, or 1 to %d coefficients)" % (shaping, sorted(NOISE_SHAPES), RRX_SHAPE_MAX_ORDER))
    coefs = [float(v) for v in coefs]
    if not 1 <= len(coefs) <= RRX_SHAPE_MAX_ORDER or not all(np.isfinite(coefs)):
        raise ValueError("a noise shape is 1 to %d finite coefficients" % RRX_SHAPE_MAX_ORDER)
    segment = int(segment)
    if not 0 <= segment < 1 << 64:
        raise ValueError("segment is a frame count, or 0 for no restart")
    return (C.c_double * len(coefs))(*coefs), segment


def finish_shaped_device(x, dst_format, shaping, segment=65536, gain=None, dither=True, seed=0, first_frame=0, state=None, out=None, peak=None,
                         clipped=None, stream=None):
    """finish_device with noise-shaped dither (RRX_finish_shaped_device): the requantisation error of a channel's previous frames
    is fed back through the filter `shaping` -- a name of NOISE_SHAPES, or 1 to 16 finite floats -- and the error history of every
    channel restarts at every absolute frame that is a multiple of `segment` (0: never, one serial chain per channel).

    `x`, `gain`, `seed`, `first_frame`, `peak`, `clipped` and `stream` are finish_device's.  `dst_format` is RRX_FMT_S16,
    RRX_FMT_S24_3 or RRX_FMT_S32, never None: the statistics depend on the format.  `out=False` measures only.  `state`: None, or the
    float64 [nstreams, nch, 16] tensor an earlier call returned; a call that does not begin a segment needs it, and contiguous
    ascending calls that hand it on leave the bytes and statistics of one call.  Returns (out, peak, clipped, state): `state` is a
    NEW tensor, never the one passed in (the call must not read and write one buffer).  The call only enqueues."""
    import torch
    shape, fmt, nstreams, frames, nch = _float_frames(x, "the output stage")
    _shaped_dst_format(dst_format)
    coefs, segment = _shaping(shaping, segment)
    seed, first_frame = _seed_and_first(seed, first_frame, frames)
    if state is None and (first_frame % segment if segment else first_frame):
        raise ValueError("a call that begins inside a segment needs the state of the call before it")
    dev = _on_device(x, "the output stage")
    gain = _gain(gain, nstreams, dev)
    _stream_state(state, nstreams, nch, RRX_SHAPE_MAX_ORDER, dev)
    out = None if out is False else _pcm_out(out, dst_format, shape[:-1], nch, dev)
    peak, clipped = _finish_stats(peak, clipped, nstreams, nch, dev)
    # frames == 0 touches nothing, the state included: the state handed on is then the one that came in
    new_state = torch.zeros((nstreams, nch, RRX_SHAPE_MAX_ORDER), dtype=torch.float64, device=dev) if state is None or frames else state.clone()
    if not frames:  # (an empty tensor has no pointer, and there is nothing to do)
        return out, peak, clipped, new_state
    _ensure_init()
    _check(lib().RRX_finish_shaped_device(*_where(dev, stream), fmt, x.data_ptr(), frames, dst_format, _ptr(out), frames, nstreams, frames, nch,
                                          _ptr(gain), 1 if dither else 0, seed, first_frame, C.cast(coefs, C.c_void_p), len(coefs), segment,
                                          _ptr(state), new_state.data_ptr(), peak.data_ptr(), clipped.data_ptr()), "RRX_finish_shaped_device")
    return out, peak, clipped, new_state


def _true_peak_filter(filter):
    """`filter` (a name of TRUE_PEAK_FILTERS or (phases, taps, coefficients)) as (phases, taps, ctypes array of doubles)"""
    f = TRUE_PEAK_FILTERS.get(filter) if isinstance(filter, str) else filter
    if f is None:
        raise ValueError("unknown true-peak filter %r (one of %s, or (phases, taps, coefficients))" % (filter, sorted(TRUE_PEAK_FILTERS)))
    phases, taps, coefs = f
    phases, taps, coefs = int(phases), int(taps), [float(v) for v in np.asarray(coefs, dtype=np.float64).reshape(-1)]
    if not (1 <= phases <= RRX_TP_MAX_PHASES and 1 <= taps <= RRX_TP_MAX_TAPS and len(coefs) == phases * taps and all(np.isfinite(coefs))):
        raise ValueError("a true-peak filter is 1..%d phases x 1..%d taps of finite coefficients, phase-major" % (RRX_TP_MAX_PHASES, RRX_TP_MAX_TAPS))
    return phases, taps, (C.c_double * len(coefs))(*coefs)


def true_peak_device(x, gain=None, first_frame=0, filter="bs1770", flush=True, state=None, true_peak=None, peak=None, stream=None):
    """True peak and sample peak on the device (RRX_true_peak_device): per (stream, channel), the peak of the gained frames
    oversampled by the polyphase `filter` -- a name of TRUE_PEAK_FILTERS ("bs1770": 4x, ITU-R BS.1770-4 Annex 2) or (phases, taps,
    coefficients) -- and the peak of the gained samples themselves, which is finish_device's measure-only peak bit for bit.  The
    gain that normalises a track comes from max(true_peak, peak): either can be the larger one.

    `x`, `gain` and `stream` are finish_device's.  `flush`: evaluate the filter's tail behind the last frame too (the last chunk
    of a track, or a whole track).  `state`: None, or the float64 [nstreams, nch, 16] tensor the call before returned; a call with
    first_frame > 0 needs it, and contiguous ascending calls that hand it on, with flush on the last one only, leave the bits of
    one call.  `true_peak` / `peak` (float64 [nstreams, nch]) are allocated (zeroed) when not passed and accumulated into
    otherwise.  Returns (true_peak, peak, state_out): `state_out` is a NEW tensor, never the one passed in.  The call only
    enqueues."""
    import torch
    _, fmt, nstreams, frames, nch = _float_frames(x, "the true-peak pass")
    phases, taps, coefs = _true_peak_filter(filter)
    first_frame = _first_frame(first_frame, frames)
    if state is None and first_frame:
        raise ValueError("a call that does not begin the stream needs the state of the call before it")
    dev = _on_device(x, "the true-peak pass")
    gain = _gain(gain, nstreams, dev)
    _stream_state(state, nstreams, nch, RRX_TP_MAX_TAPS, dev)
    true_peak, peak = _true_peak_stats(true_peak, peak, nstreams, nch, dev)
    # frames == 0 touches nothing, the state included: the state handed on is then the one that came in
    if frames or state is None or not first_frame:
        new_state = torch.zeros((nstreams, nch, RRX_TP_MAX_TAPS), dtype=torch.float64, device=dev)
    else:
        new_state = state.clone()
    if not frames:  # (an empty tensor has no pointer, and there is nothing to do)
        return true_peak, peak, new_state
    _ensure_init()
    _check(lib().RRX_true_peak_device(*_where(dev, stream), fmt, x.data_ptr(), frames, nstreams, frames, nch, _ptr(gain), first_frame,
                                      C.cast(coefs, C.c_void_p), phases, taps, 1 if flush else 0, _ptr(state), new_state.data_ptr(),
                                      true_peak.data_ptr(), peak.data_ptr()), "RRX_true_peak_device")
    return true_peak, peak, new_state


class TracksPlan:
    """RRX_tracks_plan's answer: `table` (a ctypes array of RRXTrack, one per track), `row_frames` (length of the rows the handle
    is pushed from), `out_row_cap` (pitch of its output rows), `src_total` / `dst_total` (frames of the packed source /
    destination).  `array()` is the table as uint64 [ntracks, 6]; `to_device(device)` uploads it (int64 [ntracks, 6])."""

    links = None   # (album.TracksAlbumPlan: the links of a gapless plan)
    packed = None  # (a batch of convert_library_to_pcm(gapless=): the library's packed source, which its entries point into)

    def __init__(self, table, row_frames, out_row_cap, src_total, dst_total):
        self.table, self.row_frames, self.out_row_cap, self.src_total, self.dst_total = table, row_frames, out_row_cap, src_total, dst_total

    def __len__(self):
        return len(self.table)

    def array(self):
        return np.frombuffer(self.table, dtype=np.uint64).reshape(len(self.table), 6).copy()

    def to_device(self, device):
        import torch
        return torch.from_numpy(self.array().view(np.int64)).to(device)


def track_geometry(in_rate, out_rate, frames, **kw):
    """Host-only: (lead, ext_frames, out_first, out_frames) of one track of `frames` frames on a handle of its own
    (RRX_track_geometry).  Needs no GPU."""
    cfg = _config(in_rate, out_rate, **kw)
    v = [C.c_size_t(0) for _ in range(4)]
    _check(lib().RRX_track_geometry(C.byref(cfg), int(frames), *[C.byref(x) for x in v]), "RRX_track_geometry")
    return tuple(x.value for x in v)


def _tracks_plan(cfg, lengths):
    n = len(lengths)
    if n < 1:
        raise ValueError("a plan needs at least one track")
    if min(lengths) < 0:
        raise ValueError("track lengths are frame counts: none may be negative")
    fr = (C.c_size_t * n)(*[int(v) for v in lengths])
    table = (RRXTrack * n)()
    v = [C.c_size_t(0) for _ in range(4)]
    _check(lib().RRX_tracks_plan(C.byref(cfg), fr, n, table, *[C.byref(x) for x in v]), "RRX_tracks_plan")
    return TracksPlan(table, *[x.value for x in v])


def tracks_plan(in_rate, out_rate, lengths, **kw):
    """Host-only: the geometry of a ragged batch of tracks of `lengths` frames (RRX_tracks_plan), as a TracksPlan.  Needs no GPU."""
    return _tracks_plan(_config(in_rate, out_rate, **kw), list(lengths))


class PackedTable:
    """The device copy of a table for the packed meter calls, with what they need beside it: `tensor` (int64 [ntracks, 6]),
    `src_total` and `max_frames`.  What PackedPlan.to_device returns."""

    def __init__(self, tensor, src_total, max_frames):
        self.tensor, self.src_total, self.max_frames = tensor, int(src_total), int(max_frames)

    def __len__(self):
        return self.tensor.shape[0]


class PackedPlan:
    """packed_plan's answer: `table` (a ctypes array of RRXTrack with src_first as prefix sums, frames as the lengths and zeros
    elsewhere), `src_total` (frames of the packed source) and `max_frames` (the longest track).  `array()` is the table as uint64
    [ntracks, 6]; `to_device(device)` uploads it, as a PackedTable."""

    def __init__(self, table, src_total, max_frames):
        self.table, self.src_total, self.max_frames = table, src_total, max_frames

    def __len__(self):
        return len(self.table)

    def array(self):
        return np.frombuffer(self.table, dtype=np.uint64).reshape(len(self.table), 6).copy()

    def to_device(self, device):
        import torch
        return PackedTable(torch.from_numpy(self.array().view(np.int64)).to(device), self.src_total, self.max_frames)


def packed_plan(lengths):
    """Host-only: the table of a library at rest for tracks_true_peak_packed_device / tracks_loudness_packed_device -- tracks of
    `lengths` frames laid end to end -- as a PackedPlan.  A scan needs no rate pair and no handle (a table of tracks_plan works
    just as well: the packed calls read only its input side).  Needs no GPU and no library."""
    lengths = [int(v) for v in lengths]
    if len(lengths) < 1:
        raise ValueError("a plan needs at least one track")
    if min(lengths) < 0:
        raise ValueError("track lengths are frame counts: none may be negative")
    table = (RRXTrack * len(lengths))()
    first = 0
    for t, n in zip(table, lengths):
        t.src_first, t.frames = first, n
        first += n
    if first >= 1 << 60:
        raise ValueError("no source has 2^60 frames")
    return PackedPlan(table, first, max(lengths))


class TracksBatches:
    """RRX_tracks_batches' answer: `order` (the track indices by length descending, ties by index), `batches` (the same cut every
    `nstreams` tracks: a list of lists of indices), `row_frames` (per batch, what tracks_plan gives it), `resampled` (frames the
    handle resamples: nstreams rows per batch) and `useful` (the tracks' own extended frames).  `padding` = 1 - useful / resampled."""

    def __init__(self, order, nstreams, row_frames, resampled, useful):
        self.order, self.nstreams, self.row_frames, self.resampled, self.useful = order, nstreams, row_frames, resampled, useful
        self.batches = [order[k:k + nstreams] for k in range(0, len(order), nstreams)]

    def __len__(self):
        return len(self.batches)

    @property
    def padding(self):
        return 1.0 - self.useful / self.resampled if self.resampled else 0.0


def _tracks_batches(cfg, lengths, nstreams):
    n = len(lengths)
    if n < 1:
        raise ValueError("a library needs at least one track")
    if min(lengths) < 0:
        raise ValueError("track lengths are frame counts: none may be negative")
    nstreams = int(nstreams)
    fr = (C.c_size_t * n)(*[int(v) for v in lengths])
    order = (C.c_int * n)()
    rows = (C.c_size_t * (-(-n // max(nstreams, 1))))()
    nb = C.c_int(0)
    res, use = C.c_ulonglong(0), C.c_ulonglong(0)
    _check(lib().RRX_tracks_batches(C.byref(cfg), fr, n, nstreams, order, rows, C.byref(nb), C.byref(res), C.byref(use)), "RRX_tracks_batches")
    return TracksBatches(list(order), nstreams, list(rows)[:nb.value], res.value, use.value)


def tracks_batches(in_rate, out_rate, lengths, nstreams, **kw):
    """Host-only: a library of tracks of `lengths` frames as the batches of a handle of `nstreams` streams, longest first
    (RRX_tracks_batches), as a TracksBatches.  No split into batches of at most `nstreams` tracks resamples fewer frames.  Needs no GPU."""
    return _tracks_batches(_config(in_rate, out_rate, **kw), list(lengths), nstreams)


def plan_cache_clear():
    """Host-only: drop every plan of the process-wide plan cache and zero its counters (RRX_plan_cache_clear)."""
    lib().RRX_plan_cache_clear()


def plan_cache_stats():
    """Host-only: (hits, misses, entries) of the process-wide plan cache (RRX_plan_cache_stats)."""
    h, m, e = C.c_ulonglong(0), C.c_ulonglong(0), C.c_int(0)
    _check(lib().RRX_plan_cache_stats(C.byref(h), C.byref(m), C.byref(e)), "RRX_plan_cache_stats")
    return h.value, m.value, e.value


class _Scratch:
    """The float32 row and window buffers of a library conversion: each is taken once, at the first batch's size -- the longest,
    since the batches are sorted -- and handed to the later batches as views (the first call of a process spends 0.7 to 1.5 s
    allocating rows: DESIGN.md 11)."""

    def __init__(self):
        self.flat = {}

    def take(self, name, shape, device):
        import torch
        n = 1
        for v in shape:
            n *= int(v)
        f = self.flat.get(name)
        if f is None or f.numel() < n or f.device != device:
            f = self.flat[name] = torch.empty(max(n, 1), dtype=torch.float32, device=device)
        return f[:n].view(shape)


def _tracks_table(table, ntracks=None, dev=None):
    """the device copy of a plan's table: a contiguous int64 tensor [ntracks, 6], with `dev` on that device"""
    if str(table.dtype) != "torch.int64" or table.dim() != 2 or table.shape[1] != 6 or not table.is_cuda or not table.is_contiguous():
        raise TypeError("the table must be a contiguous int64 device tensor [ntracks, 6] (TracksPlan.to_device)")
    if ntracks is not None and table.shape[0] != ntracks:
        raise ValueError("the table has %d entries for %d rows" % (table.shape[0], ntracks))
    if dev is not None and table.device != dev:
        raise _table_elsewhere(dev)
    return table.shape[0]


def _table_elsewhere(dev):
    return TypeError("the table must be on %s" % (dev,))


def _tracks_src_format(dtype):
    """the RRX_FMT_* a packed source of this torch dtype is staged as, or None: uint8 means packed 3-byte S24"""
    return {"torch.float32": RRX_FMT_FLOAT, "torch.int16": RRX_FMT_S16, "torch.int32": RRX_FMT_S32, "torch.uint8": RRX_FMT_S24_3}.get(str(dtype))


def _tracks_stage_source(packed, table):
    """the packed source and the table of a stage call, checked: (RRX_FMT_*, ntracks, nch, src_total)"""
    fmt = _tracks_src_format(packed.dtype)
    if packed.dim() != 2 or fmt is None or not packed.is_cuda or not packed.is_contiguous():
        raise TypeError("packed must be a contiguous float32, int16 or int32 device tensor [frames, nch], or uint8 [frames, nch * 3]")
    ntracks = _tracks_table(table)
    src_total, nch = packed.shape
    if fmt == RRX_FMT_S24_3:
        if nch % 3 or not nch:
            raise ValueError("a uint8 source is packed 24-bit PCM [frames, nch * 3]; its last dimension is %d" % nch)
        nch //= 3
    if table.device != packed.device:
        raise _table_elsewhere(packed.device)
    return fmt, ntracks, nch, src_total


def _tracks_stage_out(out, shape, device):
    import torch
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if out.dtype != torch.float32 or tuple(out.shape) != shape or out.device != device or not out.is_contiguous():
        raise TypeError("out must be a contiguous float32 tensor %r on %s" % (shape, device))
    return out


def _tracks_stage_pointer(packed):
    """(nothing but zero-length tracks: the call still wants a pointer, and never reads through it)"""
    import torch
    _ensure_init()
    if not packed.shape[0]:
        return torch.zeros((1, packed.shape[1]), dtype=packed.dtype, device=packed.device)
    return packed


def tracks_stage_device(packed, table, in_rate, out_rate, row_frames, out=None, stream=None):
    """The stage pass of a ragged batch on the device (RRX_tracks_stage_device_samples): `packed` is a contiguous device tensor of
    tracks laid end to end -- float32, int16 (RRX_FMT_S16) or int32 (RRX_FMT_S32) [src_total, nch], or uint8 [src_total, nch * 3]
    (RRX_FMT_S24_3: packed little-endian 24 bit, the layout tracks_finish_device returns for that format) -- and `table` the device
    copy of a plan's table (TracksPlan.to_device).  Integer PCM is converted on load, x = s * 2^-15 / 2^-23 / 2^-31 rounded once
    to float32 (ratelib_amd.h), so no float32 copy of the source is needed.  Returns the rows the handle is pushed from, float32
    [ntracks, row_frames, nch] whatever the source is (`out`, or a new tensor): each track behind and in front of its own LPC
    extension, zeros behind it.  `stream` as in lpc_extrapolate_device: the call only enqueues."""
    fmt, ntracks, nch, src_total = _tracks_stage_source(packed, table)
    out = _tracks_stage_out(out, (ntracks, int(row_frames), nch), packed.device)
    packed = _tracks_stage_pointer(packed)
    _check(lib().RRX_tracks_stage_device_samples(*_where(packed.device, stream), int(in_rate), int(out_rate),
                                                 table.data_ptr(), ntracks, nch, fmt, packed.data_ptr(), src_total,
                                                 _ptr(out), int(row_frames)), "RRX_tracks_stage_device_samples")
    return out


def _tracks_window(row_frames, win_first, win_frames, win_stride=None):
    """the window of a window call, checked; `win_stride`: it lies in a tensor of that many frames a row"""
    row_frames, win_first, win_frames = int(row_frames), int(win_first), int(win_frames)
    if win_first < 0 or win_frames < 0 or win_first + win_frames > row_frames:
        raise ValueError("the window [%d, %d) does not lie inside rows of %d frames" % (win_first, win_first + win_frames, row_frames))
    if win_stride is not None and win_frames > win_stride:
        raise ValueError("a window of %d frames in a tensor of %d frames a row" % (win_frames, win_stride))
    return row_frames, win_first, win_frames


def tracks_stage_window_device(packed, table, in_rate, out_rate, row_frames, win_first, win_frames, out=None, stream=None):
    """tracks_stage_device on a window of the rows (RRX_tracks_stage_window_device): frames [win_first, win_first + win_frames) of
    every row, bit for bit what tracks_stage_device writes there, without the rows -- `row_frames` is their length, and no tensor
    of that size is made.  Returns float32 [ntracks, win_stride, nch] with win_stride >= win_frames: `out`, of which frames
    [0, win_frames) of every row are written and the rest is left alone, or a new tensor with win_stride == win_frames.  `packed`,
    `table` and `stream` as in tracks_stage_device; the call only enqueues."""
    fmt, ntracks, nch, src_total = _tracks_stage_source(packed, table)
    row_frames, win_first, win_frames = _tracks_window(row_frames, win_first, win_frames)
    if out is not None and (out.dim() != 3 or out.shape[1] < win_frames):
        raise TypeError("out must be a contiguous float32 tensor [%d, at least %d, %d] on %s" % (ntracks, win_frames, nch, packed.device))
    out = _tracks_stage_out(out, (ntracks, win_frames if out is None else out.shape[1], nch), packed.device)
    packed = _tracks_stage_pointer(packed)
    if not win_frames:  # (an empty tensor has no pointer, and there is nothing to do)
        return out
    _check(lib().RRX_tracks_stage_window_device(*_where(packed.device, stream), int(in_rate), int(out_rate),
                                                table.data_ptr(), ntracks, nch, fmt, packed.data_ptr(), src_total,
                                                row_frames, win_first, win_frames, _ptr(out), out.shape[1]),
           "RRX_tracks_stage_window_device")
    return out


def mix_matrix(name, normalize=False):
    """A matrix of MIX_MATRICES by name (a writable copy), or any array-like [nch_dst, nch_src] as float64.  normalize=True divides
    it by its largest row sum of magnitudes when that is above 1, so that a full-scale source cannot clip."""
    m = np.array(MIX_MATRICES[name] if isinstance(name, str) else name, dtype=np.float64)
    if normalize:
        worst = float(np.abs(m).sum(axis=1).max()) if m.size else 0.0
        if worst > 1.0:
            m = m / worst
    return m


def _mix_checked(matrix, nch_src=None, nch_dst=None):
    """the matrix of a mixing call: a name of MIX_MATRICES or an array [nch_dst, nch_src] -> contiguous float64; ValueError for a
    shape that does not fit"""
    if isinstance(matrix, str):
        if matrix not in MIX_MATRICES:
            raise ValueError("unknown mix %r (MIX_MATRICES: %s)" % (matrix, ", ".join(sorted(MIX_MATRICES))))
        matrix = MIX_MATRICES[matrix]
    m = np.ascontiguousarray(matrix, dtype=np.float64)
    if m.ndim != 2 or not 1 <= m.shape[0] <= RRX_MIX_MAX_CH or not 1 <= m.shape[1] <= RRX_MIX_MAX_CH:
        raise ValueError("a mix is a matrix [nch_dst, nch_src] of 1 to %d channels each, not shape %r" % (RRX_MIX_MAX_CH, m.shape))
    if not np.isfinite(m).all():
        raise ValueError("the mix has a coefficient that is not finite")
    if nch_src is not None and m.shape[1] != nch_src:
        raise ValueError("the mix takes %d channels and the source has %d" % (m.shape[1], nch_src))
    if nch_dst is not None and m.shape[0] != nch_dst:
        raise ValueError("the mix gives %d channels where %d are expected" % (m.shape[0], nch_dst))
    return m


def mix_device(rows, matrix, out=None, stream=None, frames=None):
    """A channel-mixing matrix on device-resident rows (RRX_mix_device): `rows` is a contiguous float32 or float64 device tensor
    [frames, nch_src] or [nstreams, frames, nch_src], `matrix` a name of MIX_MATRICES or an array [nch_dst, nch_src].  Every
    frame is mixed by the rule of ratelib_amd.h -- fp64 products and sums, each rounded on its own, a zero coefficient meaning
    "not connected" -- into `out` ([..., frames or more, nch_dst] of the same dtype, which must not overlap `rows`; allocated when
    not passed).  `frames` (default: all): only frames [0, frames) of every row are mixed, and nothing else of `out` is written.
    Returns `out`.  `stream` as in lpc_extrapolate_device: the call only enqueues."""
    import torch
    shape, nstreams, stride, nch_src = _frames_shape(rows)
    if rows.dtype not in (torch.float32, torch.float64):
        raise TypeError("%s buffer: mix_device reads float32 or float64 frames" % (rows.dtype,))
    if not getattr(rows, "is_cuda", False) or not rows.is_contiguous():
        raise TypeError("mix_device works on contiguous device tensors")
    m = _mix_checked(matrix, nch_src=nch_src)
    nch_dst = m.shape[0]
    frames = stride if frames is None else int(frames)
    if not 0 <= frames <= stride:
        raise ValueError("frames must be 0 to %d, not %d" % (stride, frames))
    dev = rows.device
    if out is None:
        out = torch.empty(shape[:-1] + (nch_dst,), dtype=rows.dtype, device=dev)
    elif (out.dtype != rows.dtype or out.dim() != len(shape) or out.shape[-1] != nch_dst or out.shape[-2] < frames or out.device != dev
          or not out.is_contiguous() or (len(shape) == 3 and out.shape[0] != nstreams)):
        raise TypeError("out must be a contiguous %s tensor [..., at least %d, %d] on %s" % (rows.dtype, frames, nch_dst, dev))
    if not frames or not nstreams:
        return out
    _ensure_init()
    _check(lib().RRX_mix_device(*_where(dev, stream), _float_fmt(rows.dtype), rows.data_ptr(), stride, nstreams, frames, nch_src, _ptr(out),
                                out.shape[-2], nch_dst, m.ctypes.data), "RRX_mix_device")
    return out


def tracks_stage_mix_device(packed, table, matrix, in_rate, out_rate, row_frames, out=None, stream=None):
    """tracks_stage_device with a channel mix on load (RRX_tracks_stage_mix_device): `packed` holds nch_src channels (for uint8,
    packed 24 bit, nch_src = shape[1] // 3), `matrix` is a name of MIX_MATRICES or an array [nch, nch_src], and the rows are
    float32 [ntracks, row_frames, nch] -- bit for bit those of tracks_stage_device on the float32 source whose frames are the
    mixed frames (ratelib_amd.h has the rule), LPC extensions included.  The source is read once, as it is stored.  `table`, `out`
    and `stream` as in tracks_stage_device: the call only enqueues."""
    fmt, ntracks, nch_src, src_total = _tracks_stage_source(packed, table)
    m = _mix_checked(matrix, nch_src=nch_src)
    out = _tracks_stage_out(out, (ntracks, int(row_frames), m.shape[0]), packed.device)
    packed = _tracks_stage_pointer(packed)
    _check(lib().RRX_tracks_stage_mix_device(*_where(packed.device, stream), int(in_rate), int(out_rate),
                                             table.data_ptr(), ntracks, fmt, nch_src, packed.data_ptr(), src_total,
                                             m.shape[0], m.ctypes.data, _ptr(out), int(row_frames)),
           "RRX_tracks_stage_mix_device")
    return out


def tracks_stage_mix_window_device(packed, table, matrix, in_rate, out_rate, row_frames, win_first, win_frames, out=None, stream=None):
    """tracks_stage_mix_device on a window of the rows (RRX_tracks_stage_mix_window_device): frames [win_first, win_first +
    win_frames) of every row, bit for bit, as tracks_stage_window_device gives those of tracks_stage_device; `out` as there."""
    fmt, ntracks, nch_src, src_total = _tracks_stage_source(packed, table)
    m = _mix_checked(matrix, nch_src=nch_src)
    nch = m.shape[0]
    row_frames, win_first, win_frames = _tracks_window(row_frames, win_first, win_frames)
    if out is not None and (out.dim() != 3 or out.shape[1] < win_frames):
        raise TypeError("out must be a contiguous float32 tensor [%d, at least %d, %d] on %s" % (ntracks, win_frames, nch, packed.device))
    out = _tracks_stage_out(out, (ntracks, win_frames if out is None else out.shape[1], nch), packed.device)
    packed = _tracks_stage_pointer(packed)
    if not win_frames:  # (an empty tensor has no pointer, and there is nothing to do)
        return out
    _check(lib().RRX_tracks_stage_mix_window_device(*_where(packed.device, stream), int(in_rate), int(out_rate),
                                                    table.data_ptr(), ntracks, fmt, nch_src, packed.data_ptr(),
                                                    src_total, nch, m.ctypes.data, row_frames, win_first, win_frames,
                                                    _ptr(out), out.shape[1]), "RRX_tracks_stage_mix_window_device")
    return out


def tracks_finish_device(rows, table, dst_format, dst_total, gain=None, dither=False, seed=0, out=None, peak=None, clipped=None, stream=None):
    """The output stage of a ragged batch on the device (RRX_tracks_finish_device): finish_device per track, in one call.

    `rows` is a contiguous float32 or float64 device tensor [ntracks, row_frames, nch] (a handle's output rows), `table` the
    device copy of a plan's table: track t's frames [out_first, out_first + out_frames) of row t go to frames [dst_first,
    dst_first + out_frames) of one packed destination of `dst_total` frames -- int16 / int32 [dst_total, nch], or uint8
    [dst_total, nch * 3] for RRX_FMT_S24_3; `dst_format` None measures only.  `gain`: None, a float, or a float64 device tensor
    [ntracks].  `peak` (float64 [ntracks, nch]) and `clipped` (int64 [ntracks, nch]) cover each track's own frames only; they
    are allocated (zeroed) when not passed and accumulated into otherwise.  Returns (out, peak, clipped).  The call only enqueues."""
    fmt, ntracks, row_frames, nch = _tracks_frames(rows, "rows", "row_frames")
    seed, dst_total, gain, out, peak, clipped = _tracks_finish_buffers(rows, table, dst_format, dst_total, gain, seed, out, peak, clipped)
    dev = rows.device
    write = out is not None and dst_total > 0  # (an empty tensor has no pointer: nothing to write is measure only)
    _check(lib().RRX_tracks_finish_device(*_where(dev, stream), table.data_ptr(), ntracks, nch, fmt, rows.data_ptr(), row_frames, dst_format or 0,
                                          out.data_ptr() if write else None, dst_total, _ptr(gain), 1 if dither else 0, seed, peak.data_ptr(),
                                          clipped.data_ptr()), "RRX_tracks_finish_device")
    return out, peak, clipped


def tracks_true_peak_device(rows, table, gain=None, filter="bs1770", true_peak=None, peak=None, stream=None):
    """true_peak_device per track of a ragged batch, in one call (RRX_tracks_true_peak_device): `rows` and `table` as in
    tracks_finish_device; track t's frames [out_first, out_first + out_frames) of row t are measured as one whole track -- from
    +0.0 at its first output frame (the row in front of it is not history: the written file does not hold it), flushed behind its
    last -- under `gain` (None, a float, or a float64 device tensor [ntracks]).  `filter` is true_peak_device's.  `true_peak` and
    `peak` (float64 [ntracks, nch]) are allocated (zeroed) when not passed and accumulated into otherwise.  Returns (true_peak,
    peak).  The call only enqueues."""
    fmt, ntracks, row_frames, nch = _tracks_frames(rows, "rows", "row_frames")
    dev = rows.device
    _tracks_table(table, ntracks, dev)
    phases, taps, coefs = _true_peak_filter(filter)
    gain = _gain(gain, ntracks, dev)
    true_peak, peak = _true_peak_stats(true_peak, peak, ntracks, nch, dev)
    if not row_frames:  # (an empty tensor has no pointer, and there is nothing to do)
        return true_peak, peak
    _ensure_init()
    _check(lib().RRX_tracks_true_peak_device(*_where(dev, stream), table.data_ptr(), ntracks, nch, fmt, rows.data_ptr(), row_frames, _ptr(gain),
                                             C.cast(coefs, C.c_void_p), phases, taps, true_peak.data_ptr(), peak.data_ptr()),
           "RRX_tracks_true_peak_device")
    return true_peak, peak


def _packed_table(table, max_frames, device):
    """the table of a packed meter call as (int64 device tensor [ntracks, 6], max_frames): a PackedPlan or TracksPlan is uploaded, a
    PackedTable brings its own max_frames, a bare device tensor needs `max_frames`"""
    if isinstance(table, (PackedPlan, TracksPlan)):
        import torch
        a = table.array()
        table = PackedTable(torch.from_numpy(a.view(np.int64)).to(device), table.src_total, int(a[:, 1].max()))
    if isinstance(table, PackedTable):
        table, own = table.tensor, table.max_frames
        max_frames = own if max_frames is None else max_frames
    elif max_frames is None:
        raise ValueError("a bare table tensor does not say how long its tracks are: give max_frames")
    max_frames = int(max_frames)
    if max_frames < 0:
        raise ValueError("max_frames is a frame count")
    return table, max_frames


def tracks_true_peak_packed_device(packed, table, gain=None, filter="bs1770", max_frames=None, true_peak=None, peak=None, stream=None):
    """True peak and sample peak per track of a library at rest (RRX_tracks_true_peak_packed_device): `packed` is the source of
    tracks_stage_device -- tracks laid end to end, float32 / int16 / int32 [src_total, nch] or uint8 [src_total, nch * 3] for packed
    24 bit -- measured as it is stored: no float copy, no rows, no handle.  `table`: a PackedPlan / TracksPlan (uploaded here), what
    their to_device returned, or a bare int64 device tensor [ntracks, 6] with `max_frames`, the most frames a track is measured
    for (taken from the plan otherwise).  Only src_first and frames of an entry are read, clamped to the source.  The sample value
    is exact -- s * 2^-15 / 2^-23 / 2^-31 in float64, so INT32_MAX peaks at 1 - 2^-31 -- and from there on every track is
    true_peak_device's one whole stream, flushed.  `gain`, `filter`, `true_peak`, `peak` and the return value are
    tracks_true_peak_device's.  The call only enqueues."""
    table, max_frames = _packed_table(table, max_frames, packed.device if hasattr(packed, "device") else None)
    fmt, ntracks, nch, src_total = _tracks_stage_source(packed, table)
    dev = packed.device
    phases, taps, coefs = _true_peak_filter(filter)
    gain = _gain(gain, ntracks, dev)
    true_peak, peak = _true_peak_stats(true_peak, peak, ntracks, nch, dev)
    if not max_frames or not src_total:  # (an empty tensor has no pointer, and there is nothing to do)
        return true_peak, peak
    _ensure_init()
    _check(lib().RRX_tracks_true_peak_packed_device(*_where(dev, stream), table.data_ptr(),
                                                    ntracks, nch, fmt, packed.data_ptr(), src_total, max_frames,
                                                    _ptr(gain), C.cast(coefs, C.c_void_p),
                                                    phases, taps, true_peak.data_ptr(), peak.data_ptr()),
           "RRX_tracks_true_peak_packed_device")
    return true_peak, peak


def limit_work_doubles(nstreams, frames, taps=12, lookahead=64):
    """Doubles of work memory that limit_device / tracks_limit_device need for `nstreams` rows of `frames` frames
    (RRX_limit_work_doubles: nstreams * 2 * (frames + taps + lookahead)); 0 for arguments the calls refuse.  Host only."""
    return int(lib().RRX_limit_work_doubles(int(nstreams), int(frames), int(taps), int(lookahead)))


def _limit_params(ceiling, lookahead, hold):
    """the limiter's scalar arguments, checked as the C call checks them"""
    ceiling, lookahead, hold = float(ceiling), int(lookahead), int(hold)
    if not (np.isfinite(ceiling) and ceiling > 0):
        raise ValueError("the ceiling is a finite linear level above 0")
    if not 1 <= lookahead <= RRX_LIMIT_MAX_LOOKAHEAD:
        raise ValueError("lookahead is 1..%d frames" % RRX_LIMIT_MAX_LOOKAHEAD)
    if not 0 <= hold <= RRX_LIMIT_MAX_HOLD:
        raise ValueError("hold is 0..%d frames" % RRX_LIMIT_MAX_HOLD)
    return ceiling, lookahead, hold


def _limit_buffers(x, out, n, frames, taps, lookahead, dev, block=None):
    """(out, reduction preset to 1.0, limited zeroed, work) of a limiter call on `n` rows of `frames` frames; with `block`, of a
    call with a release"""
    import torch
    if out is None:
        out = torch.empty_like(x)
    else:
        odt = str(out.dtype)
        if not (odt.endswith("float32") or odt.endswith("float64")) or tuple(out.shape) != tuple(x.shape) or out.device != dev or not out.is_contiguous():
            raise TypeError("out must be a contiguous float32 or float64 tensor of shape %r on %s" % (tuple(x.shape), dev))
        if out.data_ptr() == x.data_ptr() and out.dtype != x.dtype:
            raise TypeError("in place the destination has the source's dtype")
    reduction = torch.ones((n,), dtype=torch.float64, device=dev)
    limited = torch.zeros((n,), dtype=torch.int64, device=dev)
    need = limit_work_doubles(n, frames, taps, lookahead) if block is None else limit_release_work_doubles(n, frames, taps, lookahead, block)
    if not need:
        raise ValueError("the rows are too large for the limiter's work buffer")
    return out, reduction, limited, torch.empty((need,), dtype=torch.float64, device=dev)


def limit_device(x, ceiling, gain=None, lookahead=64, hold=0, filter="bs1770", out=None, stream=None):
    """The true-peak limiter on the device (RRX_limit_device): every frame of `x` under `gain` times a gain s[n] <= 1, one per
    frame and linked across a stream's channels, which holds |y| at `ceiling` (a linear level; exact for finite input up to one
    rounding) and the true peak -- true_peak_device's, with `filter` -- near it.  s is the minimum of the demanded reductions
    over a window that begins `hold` frames behind a frame and ends `lookahead` frames and the filter's length ahead of it,
    smoothed by a box of `lookahead` frames: it starts to fall lookahead + taps - 1 frames before a peak and returns over
    `lookahead` frames, `hold` frames behind it.  The true peak of y can exceed the ceiling by a residual that shrinks with
    `lookahead` (below one percent at 72); measure y with true_peak_device and trim where the bound has to hold.

    `x`, `gain` and `stream` are true_peak_device's.  `out`: None (a new tensor like x), x itself (in place), or a float32 /
    float64 tensor of x's shape that shares no memory with it.  Returns (y, reduction, limited): float64 [nstreams] the
    smallest s of each stream (1.0 where nothing was limited) and int64 [nstreams] the frames with s < 1.  The call only
    enqueues; its work buffer comes from torch's allocator."""
    return _limit_device(x, ceiling, gain, lookahead, hold, filter, out, stream, None)


def _limit_device(x, ceiling, gain, lookahead, hold, filter, out, stream, release):
    """limit_device (release = None) and limit_release_device (release = (pole, block), checked)"""
    _, fmt, nstreams, frames, nch = _float_frames(x, "the limiter")
    phases, taps, coefs = _true_peak_filter(filter)
    ceiling, lookahead, hold = _limit_params(ceiling, lookahead, hold)
    dev = _on_device(x, "the limiter")
    gain = _gain(gain, nstreams, dev)
    out, reduction, limited, work = _limit_buffers(x, out, nstreams, frames, taps, lookahead, dev, None if release is None else release[1])
    if not frames:  # (an empty tensor has no pointer, and there is nothing to do)
        return out, reduction, limited
    _ensure_init()
    head = (*_where(dev, stream), fmt, x.data_ptr(), frames, _float_fmt(out.dtype), _ptr(out), frames, nstreams, frames, nch, _ptr(gain), ceiling,
            C.cast(coefs, C.c_void_p), phases, taps, lookahead, hold)
    tail = (reduction.data_ptr(), limited.data_ptr(), work.data_ptr(), work.numel())
    if release is None:
        _check(lib().RRX_limit_device(*(head + tail)), "RRX_limit_device")
    else:
        _check(lib().RRX_limit_release_device(*(head + release + tail)), "RRX_limit_release_device")
    return out, reduction, limited


def tracks_limit_device(rows, table, ceiling, gain=None, lookahead=64, hold=0, filter="bs1770", out=None, stream=None):
    """limit_device per track of a ragged batch, in one call (RRX_tracks_limit_device): `rows`, `table` and `gain` as in
    tracks_true_peak_device; track t's frames [out_first, out_first + out_frames) of row t are limited as one whole track -- from
    +0.0 at its first output frame, the filter's tail behind its last -- and go to the same frames of `out`: None (in place,
    into `rows`), or a float32 / float64 tensor of rows' shape that shares no memory with it.  Frames outside the slices are
    not written.  Returns (out, reduction [ntracks], limited [ntracks]) as limit_device.  The call only enqueues."""
    return _tracks_limit_device(rows, table, ceiling, gain, lookahead, hold, filter, out, stream, None)


def _tracks_limit_device(rows, table, ceiling, gain, lookahead, hold, filter, out, stream, release):
    """tracks_limit_device (release = None) and tracks_limit_release_device (release = (pole, block), checked)"""
    fmt, ntracks, row_frames, nch = _tracks_frames(rows, "rows", "row_frames")
    dev = rows.device
    _tracks_table(table, ntracks, dev)
    phases, taps, coefs = _true_peak_filter(filter)
    ceiling, lookahead, hold = _limit_params(ceiling, lookahead, hold)
    gain = _gain(gain, ntracks, dev)
    out, reduction, limited, work = _limit_buffers(rows, rows if out is None else out, ntracks, row_frames, taps, lookahead, dev,
                                                   None if release is None else release[1])
    if not row_frames:  # (an empty tensor has no pointer, and there is nothing to do)
        return out, reduction, limited
    _ensure_init()
    head = (*_where(dev, stream), table.data_ptr(), ntracks, nch, fmt, rows.data_ptr(), _float_fmt(out.dtype), _ptr(out), row_frames, _ptr(gain),
            ceiling, C.cast(coefs, C.c_void_p), phases, taps, lookahead, hold)
    tail = (reduction.data_ptr(), limited.data_ptr(), work.data_ptr(), work.numel())
    if release is None:
        _check(lib().RRX_tracks_limit_device(*(head + tail)), "RRX_tracks_limit_device")
    else:
        _check(lib().RRX_tracks_limit_release_device(*(head + release + tail)), "RRX_tracks_limit_release_device")
    return out, reduction, limited


def limit_release_coef(release_ms, rate):
    """The per-frame pole of a release with the time constant `release_ms` at `rate` frames per second:
    exp(-1 / (release_ms * 1e-3 * rate)), the `release` of limit_release_device.  After release_ms the gain has covered 1 - 1/e of
    its way back.  ValueError for a time that is not positive.  Host only."""
    release_ms, rate = float(release_ms), float(rate)
    if not (release_ms > 0 and np.isfinite(release_ms) and rate > 0 and np.isfinite(rate)):
        raise ValueError("the release time and the rate are positive and finite")
    return float(math.exp(-1.0 / (release_ms * 1e-3 * rate)))


def limit_release_work_doubles(nstreams, frames, taps=12, lookahead=64, block=1024):
    """Doubles of work memory that limit_release_device / tracks_limit_release_device need (RRX_limit_release_work_doubles:
    nstreams * (2 * (frames + taps + lookahead) + 4 * (ceil((frames + lookahead - 1) / block) + 1))); 0 for arguments the calls
    refuse.  Host only."""
    return int(lib().RRX_limit_release_work_doubles(int(nstreams), int(frames), int(taps), int(lookahead), int(block)))


def _limit_release_params(release, block):
    """the release's two arguments, checked as the C call checks them"""
    release, block = float(release), int(block)
    if not 0.0 <= release < 1.0:  # (a NaN fails)
        raise ValueError("release is a per-frame pole in [0, 1): see limit_release_coef")
    if not RRX_LIMIT_RELEASE_MIN_BLOCK <= block <= RRX_LIMIT_RELEASE_MAX_BLOCK:
        raise ValueError("block is %d..%d entries" % (RRX_LIMIT_RELEASE_MIN_BLOCK, RRX_LIMIT_RELEASE_MAX_BLOCK))
    return release, block


def limit_release_device(x, ceiling, release, gain=None, lookahead=64, hold=0, block=1024, filter="bs1770", out=None, stream=None):
    """limit_device with an exponential release (RRX_limit_release_device): between the window minimum and the box the gain
    follows p = min(m, release * p + (1 - release) * m), so after a peak it recovers towards what the programme then demands along
    an exponential with the per-frame pole `release` in [0, 1) -- limit_release_coef(release_ms, rate) for a time constant; 0.0
    gives limit_device's bits -- and never rises above limit_device's gain.  The recursion runs as a scan over blocks of `block`
    entries (64..65536), which is part of the result's bits (include/ratelib_amd.h).  Everything else, the returns included, is
    limit_device's."""
    return _limit_device(x, ceiling, gain, lookahead, hold, filter, out, stream, _limit_release_params(release, block))


def tracks_limit_release_device(rows, table, ceiling, release, gain=None, lookahead=64, hold=0, block=1024, filter="bs1770", out=None,
                                stream=None):
    """limit_release_device per track of a ragged batch, in one call (RRX_tracks_limit_release_device): tracks_limit_device with
    the release of limit_release_device, every track's slice as a one-stream call of its own from the state 1.0."""
    return _tracks_limit_device(rows, table, ceiling, gain, lookahead, hold, filter, out, stream, _limit_release_params(release, block))


def limit_window_reach(lookahead, hold, filter="bs1770"):
    """(back, ahead) of the limiter (RRX_limit_window_reach): the gain of frame n depends on the samples of the frames
    [n - back, n + ahead] and on nothing else -- back = lookahead - 1 + hold + taps - 1, ahead = lookahead - 1 + taps - 1 with the
    taps of `filter` -- which is the halo tracks_limit_window_device needs around a window.  Host only."""
    _, taps, _ = _true_peak_filter(filter)
    _, lookahead, hold = _limit_params(1.0, lookahead, hold)
    back, ahead = C.c_size_t(0), C.c_size_t(0)
    _check(lib().RRX_limit_window_reach(taps, lookahead, hold, C.byref(back), C.byref(ahead)), "RRX_limit_window_reach")
    return int(back.value), int(ahead.value)


def tracks_limit_window_work_doubles(ntracks, win_frames, taps=12, lookahead=64, hold=0):
    """Doubles of work memory that tracks_limit_window_device needs for a window of `win_frames` frames of `ntracks` tracks
    (RRX_tracks_limit_window_work_doubles: ntracks * 2 * (win_frames + 2 * lookahead + hold + 2 * taps)); 0 for arguments the call
    refuses.  Host only."""
    return int(lib().RRX_tracks_limit_window_work_doubles(int(ntracks), int(win_frames), int(taps), int(lookahead), int(hold)))


def tracks_limit_window_device(buf, table, row_frames, buf_first, win_first, win_frames, ceiling, gain=None, lookahead=64, hold=0, filter="bs1770",
                               out=None, reduction=None, limited=None, stream=None, buf_frames=None):
    """tracks_limit_device on a window of the rows (RRX_tracks_limit_window_device).  The limiter has nothing recursive in it, so a
    window needs no state, only a halo of input: `buf`, a contiguous float32 or float64 device tensor [ntracks, buf_stride, nch],
    holds frames [buf_first, buf_first + buf_frames) of rows (`buf_frames`: None, all buf_stride of them, or fewer) of `row_frames` frames that need not exist anywhere, and must reach
    from max(0, win_first - back) to min(row_frames, win_first + win_frames + ahead) at least, (back, ahead) =
    limit_window_reach(lookahead, hold, filter); ValueError otherwise.  Of every track's slice the frames inside [win_first,
    win_first + win_frames) are limited as in the whole-row call -- from +0.0 in front of the slice and behind it, whatever the
    buffer holds there -- and go to `out[t][frame - win_first]`: None (a new float32 or float64 tensor [ntracks, win_frames, nch]
    of buf's dtype) or a contiguous one [ntracks, dst_stride >= win_frames, nch] that shares no memory with `buf` (in place is not
    offered: the next window's halo must be unlimited input).  Nothing else of `out` is written.  `reduction` (float64 [ntracks],
    preset to 1.0) and `limited` (int64 [ntracks], zeroed) are allocated when not passed and ACCUMULATED into: disjoint windows
    that cover [0, row_frames), in any order, each given the `reduction` and `limited` the first one returned, leave
    tracks_limit_device's bits in the emitted frames and its two statistics.  `ceiling`, `gain`, `lookahead`, `hold` and `filter`
    are tracks_limit_device's.  Returns (out, reduction, limited); the call only enqueues, its work buffer comes from torch's
    allocator."""
    return _tracks_limit_window_device(buf, table, row_frames, buf_first, win_first, win_frames, ceiling, gain, lookahead, hold, filter, out,
                                       reduction, limited, stream, buf_frames, None, None, None)[:3]


def _tracks_limit_window_device(buf, table, row_frames, buf_first, win_first, win_frames, ceiling, gain, lookahead, hold, filter, out, reduction,
                                limited, stream, buf_frames, release, state_in, state_out):
    """tracks_limit_window_device (release = None) and tracks_limit_release_window_device (release = (pole, block), checked):
    (out, reduction, limited, state_out)"""
    import torch
    fmt, ntracks, buf_stride, nch = _tracks_frames(buf, "buf", "buf_frames")
    row_frames, win_first, win_frames = _tracks_window(row_frames, win_first, win_frames)
    buf_first, buf_frames = int(buf_first), buf_stride if buf_frames is None else int(buf_frames)
    if not 0 <= buf_frames <= buf_stride:
        raise ValueError("%d buffered frames in a tensor of %d frames a row" % (buf_frames, buf_stride))
    dev = buf.device
    _tracks_table(table, ntracks, dev)
    phases, taps, coefs = _true_peak_filter(filter)
    ceiling, lookahead, hold = _limit_params(ceiling, lookahead, hold)
    back, ahead = limit_window_reach(lookahead, hold, filter)
    if buf_first < 0 or buf_first + buf_frames > row_frames:
        raise ValueError("the buffer [%d, %d) does not lie inside rows of %d frames" % (buf_first, buf_first + buf_frames, row_frames))
    if buf_first > max(0, win_first - back) or buf_first + buf_frames < min(row_frames, win_first + win_frames + ahead):
        raise ValueError("the buffer [%d, %d) does not cover the window [%d, %d) with its halo of %d frames behind and %d ahead"
                         % (buf_first, buf_first + buf_frames, win_first, win_first + win_frames, back, ahead))
    gain = _gain(gain, ntracks, dev)
    if out is None:
        out = torch.empty((ntracks, win_frames, nch), dtype=buf.dtype, device=dev)
    else:
        odt = str(out.dtype)
        if (out.dim() != 3 or not (odt.endswith("float32") or odt.endswith("float64")) or out.shape[0] != ntracks or out.shape[2] != nch
                or out.shape[1] < win_frames or out.device != dev or not out.is_contiguous()):
            raise TypeError("out must be a contiguous float32 or float64 tensor [%d, >= %d, %d] on %s" % (ntracks, win_frames, nch, dev))
        lo, hi = out.data_ptr(), out.data_ptr() + out.numel() * out.element_size()
        if lo < buf.data_ptr() + buf.numel() * buf.element_size() and buf.data_ptr() < hi:
            raise ValueError("out must share no memory with buf: the window form does not work in place")
    stats = []
    for t, sdt, name, preset in ((reduction, torch.float64, "reduction", 1.0), (limited, torch.int64, "limited", 0)):
        if t is None:
            t = torch.full((ntracks,), preset, dtype=sdt, device=dev)
        elif t.dtype != sdt or tuple(t.shape) != (ntracks,) or t.device != dev or not t.is_contiguous():
            raise TypeError("%s must be a contiguous %s tensor [%d] on %s" % (name, sdt, ntracks, dev))
        stats.append(t)
    reduction, limited = stats
    if release is not None:
        shape = (ntracks, RRX_LIMIT_RELEASE_WIN_STATE)
        for t, name in ((state_in, "state_in"), (state_out, "state_out")):
            if t is not None and (t.dtype != torch.float64 or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous()):
                raise TypeError("%s must be a contiguous float64 tensor [%d, %d] on %s" % ((name,) + shape + (dev,)))
        if state_in is None and win_first:
            raise ValueError("only a window at frame 0 starts without a state")
        if state_out is None:
            state_out = torch.zeros(shape, dtype=torch.float64, device=dev)
        if state_in is not None:
            lo, hi = state_out.data_ptr(), state_out.data_ptr() + state_out.numel() * 8
            if lo < state_in.data_ptr() + state_in.numel() * 8 and state_in.data_ptr() < hi:
                raise ValueError("state_out must share no memory with state_in")
    if not win_frames or not row_frames:  # (an empty tensor has no pointer, and there is nothing to do)
        return out, reduction, limited, state_out
    if release is None:
        need = tracks_limit_window_work_doubles(ntracks, win_frames, taps, lookahead, hold)
    else:
        need = tracks_limit_release_window_work_doubles(ntracks, win_frames, taps, lookahead, hold, release[1])
    if not need:
        raise ValueError("the window is too large for the limiter's work buffer")
    work = torch.empty((need,), dtype=torch.float64, device=dev)
    _ensure_init()
    head = (*_where(dev, stream), table.data_ptr(), ntracks, nch, fmt, buf.data_ptr(), buf_stride, buf_first, buf_frames, row_frames, win_first,
            win_frames, _float_fmt(out.dtype), _ptr(out), out.shape[1], _ptr(gain), ceiling, C.cast(coefs, C.c_void_p), phases, taps,
            lookahead, hold)
    tail = (reduction.data_ptr(), limited.data_ptr(), work.data_ptr(), work.numel())
    if release is None:
        _check(lib().RRX_tracks_limit_window_device(*(head + tail)), "RRX_tracks_limit_window_device")
    else:
        states = (_ptr(state_in), _ptr(state_out))
        _check(lib().RRX_tracks_limit_release_window_device(*(head + release + states + tail)), "RRX_tracks_limit_release_window_device")
    return out, reduction, limited, state_out


def tracks_limit_release_window_work_doubles(ntracks, win_frames, taps=12, lookahead=64, hold=0, block=1024):
    """Doubles of work memory that tracks_limit_release_window_device needs for a window of `win_frames` frames of `ntracks` tracks
    (RRX_tracks_limit_release_window_work_doubles: ntracks * (2 * (win_frames + 2 * lookahead + hold + 2 * taps) + 4 * ((win_frames +
    lookahead - 1) // block + 2))); 0 for arguments the call refuses.  Host only."""
    return int(lib().RRX_tracks_limit_release_window_work_doubles(int(ntracks), int(win_frames), int(taps), int(lookahead), int(hold),
                                                                  int(block)))


def tracks_limit_release_window_device(buf, table, row_frames, buf_first, win_first, win_frames, ceiling, release, state_in=None, gain=None,
                                       lookahead=64, hold=0, block=1024, filter="bs1770", out=None, reduction=None, limited=None,
                                       state_out=None, buf_frames=None, stream=None):
    """tracks_limit_window_device with the release of tracks_limit_release_device (RRX_tracks_limit_release_window_device).  The
    release is a recursion, so this call takes and returns a per-track state and depends on the order of the calls: windows that
    partition [0, row_frames), taken in ascending contiguous order, each given the `state_out` of the one before as its
    `state_in` (and the same `reduction` and `limited`), leave tracks_limit_release_device's bits and statistics for any cut
    positions -- the blocks of `block` entries stay on every track's own grid, and the scan's intermediate state crosses the cut
    (include/ratelib_amd.h).  `state_in`: a contiguous float64 device tensor [ntracks, 8], or None, which only a window at frame 0
    may pass; `state_out`: likewise, a new one when None, sharing no memory with `state_in`.  `release` and `block` are
    limit_release_device's and checked as there; release 0.0 gives tracks_limit_window_device's bits whatever the state holds.
    Everything else is tracks_limit_window_device's.  Returns (out, reduction, limited, state_out); the call only enqueues."""
    return _tracks_limit_window_device(buf, table, row_frames, buf_first, win_first, win_frames, ceiling, gain, lookahead, hold, filter, out,
                                       reduction, limited, stream, buf_frames, _limit_release_params(release, block), state_in, state_out)


K_WEIGHTING_48K =(1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
                   1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621)
"""The K-weighting of ITU-R BS.1770-4 at 48 kHz as published, in the order of RRX_loudness_device's `coefs`: b0, b1, b2, a1, a2 of
the shelving stage, then of the high-pass."""


def k_weighting(rate):
    """The ten coefficients of RRX_loudness_device for a sampling rate: the analog prototype behind the BS.1770 table -- a shelf
    (f0 1681.97 Hz, +4 dB, Q 0.7072) and a high-pass (f0 38.135 Hz, Q 0.5003, numerator 1, -2, 1 as published) -- through the
    bilinear transform.  At 48000 it reproduces K_WEIGHTING_48K to the digits the table has."""
    import math
    rate = float(rate)
    if not rate > 0:
        raise ValueError("a sampling rate is positive")
    k = math.tan(math.pi * 1681.974450955533 / rate)
    vh = 10.0 ** (3.999843853973347 / 20.0)
    vb = vh ** 0.4996667741545416
    q = 0.7071752369554196
    a0 = 1.0 + k / q + k * k
    shelf = ((vh + vb * k / q + k * k) / a0, 2.0 * (k * k - vh) / a0, (vh - vb * k / q + k * k) / a0, 2.0 * (k * k - 1.0) / a0,
             (1.0 - k / q + k * k) / a0)
    k = math.tan(math.pi * 38.13547087602444 / rate)
    q = 0.5003270373238773
    a0 = 1.0 + k / q + k * k
    return shelf + (1.0, -2.0, 1.0, 2.0 * (k * k - 1.0) / a0, (1.0 - k / q + k * k) / a0)


def _loudness_filter(rate, coefs, hop):
    """(ctypes array of the ten coefficients, hop): k_weighting(rate) and rate // 10 where not given"""
    if coefs is None:
        if rate is None:
            raise ValueError("give the sampling rate, or coefs and hop")
        coefs = k_weighting(rate)
    coefs = [float(v) for v in np.asarray(coefs, dtype=np.float64).reshape(-1)]
    if len(coefs) != 10 or not all(np.isfinite(coefs)):
        raise ValueError("the K-weighting is ten finite coefficients: b0, b1, b2, a1, a2 of two biquads")
    if hop is None:
        if rate is None:
            raise ValueError("give the sampling rate, or coefs and hop")
        hop = int(rate) // 10
    hop = int(hop)
    if hop < 1:
        raise ValueError("a hop has at least one frame")
    return (C.c_double * 10)(*coefs), hop


def _loudness_buffers(energy, work, n, nch, need_hops, need_work, dev):
    """the energy tensor (float64 [n, nch, >= need_hops], allocated zeroed when not passed) and the work buffer"""
    import torch
    if energy is None:
        energy = torch.zeros((n, nch, need_hops), dtype=torch.float64, device=dev)
    elif (energy.dtype != torch.float64 or energy.dim() != 3 or tuple(energy.shape[:2]) != (n, nch) or energy.shape[2] < need_hops
          or energy.device != dev or not energy.is_contiguous()):
        raise TypeError("energy must be a contiguous float64 tensor [%d, %d, >= %d] on %s" % (n, nch, need_hops, dev))
    if work is None:
        work = torch.empty((max(need_work, 1),), dtype=torch.float64, device=dev)
    elif work.dtype != torch.float64 or work.numel() < need_work or work.device != dev or not work.is_contiguous():
        raise TypeError("work must be a contiguous float64 tensor of at least %d elements on %s" % (need_work, dev))
    return energy, work


def loudness_device(x, rate=None, gain=None, first_frame=0, state=None, energy=None, coefs=None, hop=None, work=None, stream=None):
    """K-weighted hop energies on the device (RRX_loudness_device): for every (stream, channel) of `x` ([frames, nch] or
    [nstreams, frames, nch], float32 or float64, contiguous, on the device) the sum of squares of the K-weighted, gained frames
    over every whole hop of `hop` frames (default rate // 10, 100 ms), by the block decomposition the header defines.  `coefs`
    defaults to k_weighting(rate); `gain` and `stream` are finish_device's.

    `first_frame` must be a multiple of the hop; a call with first_frame > 0 needs `state`, the float64 [nstreams, nch, 4] tensor
    the call before returned.  Frames behind the last whole hop are not measured: a chunked caller feeds them again.  `energy`
    (float64 [nstreams, nch, >= first_frame // hop + frames // hop]) is allocated (zeroed) when not passed; the call WRITES hops
    first_frame // hop ... of it and touches nothing else.  `work` is scratch of RRX_loudness_work_doubles doubles, allocated when
    not passed.  Returns (energy, state_out): `state_out` is a NEW tensor.  Feed `energy` to loudness_gate_device.  The call only
    enqueues."""
    import torch
    _, fmt, nstreams, frames, nch = _float_frames(x, "the loudness pass")
    c, hop = _loudness_filter(rate, coefs, hop)
    first_frame = _first_frame(first_frame, frames)
    if first_frame % hop:
        raise ValueError("first_frame must be a multiple of the hop (%d)" % hop)
    if state is None and first_frame:
        raise ValueError("a call that does not begin the stream needs the state of the call before it")
    dev = _on_device(x, "the loudness pass")
    gain = _gain(gain, nstreams, dev)
    _stream_state(state, nstreams, nch, 4, dev)
    first_hop, n = first_frame // hop, frames // hop
    need = nstreams * nch * n * 4
    energy, work = _loudness_buffers(energy, work, nstreams, nch, first_hop + n, need, dev)
    # frames == 0 touches nothing, the state included: the state handed on is then the one that came in
    if frames or state is None or not first_frame:
        new_state = torch.zeros((nstreams, nch, 4), dtype=torch.float64, device=dev)
    else:
        new_state = state.clone()
    if not frames:  # (an empty tensor has no pointer, and there is nothing to do)
        return energy, new_state
    _ensure_init()
    _check(lib().RRX_loudness_device(*_where(dev, stream), fmt, x.data_ptr(), frames, nstreams, frames, nch, _ptr(gain), first_frame,
                                     C.cast(c, C.c_void_p), hop, _ptr(state), new_state.data_ptr(), energy.data_ptr(), energy.shape[2], work.data_ptr(),
                                     work.numel()), "RRX_loudness_device")
    return energy, new_state


def tracks_loudness_device(rows, table, rate=None, gain=None, coefs=None, hop=None, energy=None, work=None, stream=None):
    """loudness_device per track of a ragged batch, in one call (RRX_tracks_loudness_device): `rows` and `table` as in
    tracks_true_peak_device; track t's frames [out_first, out_first + out_frames) of row t are measured as one whole track from
    +0.0 under `gain` (None, a float, or a float64 device tensor [ntracks]).  Returns (energy, hops): `energy` float64 [ntracks,
    nch, row_frames // hop] (allocated zeroed when not passed; one that is passed may hold fewer hops, and the tracks' hops are
    clamped to it), of which track t's first hops[t] entries per channel are written, and `hops` int64 [ntracks], the whole hops of
    every track.  Feed both to loudness_gate_device.  The call only
    enqueues."""
    import torch
    fmt, ntracks, row_frames, nch = _tracks_frames(rows, "rows", "row_frames")
    dev = rows.device
    _tracks_table(table, ntracks, dev)
    c, hop = _loudness_filter(rate, coefs, hop)
    gain = _gain(gain, ntracks, dev)
    n = row_frames // hop
    energy, work = _loudness_buffers(energy, work, ntracks, nch, n if energy is None else 0, ntracks * nch * n * 4, dev)
    hops = torch.zeros((ntracks,), dtype=torch.int64, device=dev)
    if not n or not energy.shape[2]:  # (no row holds a whole hop: an empty tensor has no pointer, and there is nothing to do)
        return energy, hops
    _ensure_init()
    _check(lib().RRX_tracks_loudness_device(*_where(dev, stream), table.data_ptr(), ntracks, nch, fmt, rows.data_ptr(), row_frames, _ptr(gain),
                                            C.cast(c, C.c_void_p), hop, energy.data_ptr(), energy.shape[2], _ptr(hops), work.data_ptr(), work.numel()),
           "RRX_tracks_loudness_device")
    return energy, hops


def tracks_loudness_packed_device(packed, table, rate=None, gain=None, coefs=None, hop=None, max_frames=None, energy=None, work=None, stream=None):
    """K-weighted hop energies per track of a library at rest (RRX_tracks_loudness_packed_device): `packed`, `table` and
    `max_frames` as in tracks_true_peak_packed_device, everything else as in tracks_loudness_device with max_frames for
    row_frames.  Returns (energy, hops): `energy` float64 [ntracks, nch, max_frames // hop] (allocated zeroed when not passed; one
    that is passed may hold fewer hops, and the tracks' hops are clamped to it) and `hops` int64 [ntracks].  Feed both to
    loudness_gate_device or loudness_meter_device.  The call only enqueues."""
    import torch
    table, max_frames = _packed_table(table, max_frames, packed.device if hasattr(packed, "device") else None)
    fmt, ntracks, nch, src_total = _tracks_stage_source(packed, table)
    dev = packed.device
    c, hop = _loudness_filter(rate, coefs, hop)
    gain = _gain(gain, ntracks, dev)
    n = max_frames // hop
    energy, work = _loudness_buffers(energy, work, ntracks, nch, n if energy is None else 0, ntracks * nch * n * 4, dev)
    hops = torch.zeros((ntracks,), dtype=torch.int64, device=dev)
    if not n or not energy.shape[2] or not src_total:  # (no track holds a whole hop: an empty tensor has no pointer, and there is nothing to do)
        return energy, hops
    _ensure_init()
    _check(lib().RRX_tracks_loudness_packed_device(*_where(dev, stream), table.data_ptr(), ntracks, nch, fmt, packed.data_ptr(), src_total, max_frames,
                                                   _ptr(gain), C.cast(c, C.c_void_p), hop, energy.data_ptr(), energy.shape[2], _ptr(hops),
                                                   work.data_ptr(), work.numel()), "RRX_tracks_loudness_packed_device")
    return energy, hops


def loudness_gate(abs_lufs=-70.0, rel_lu=-10.0):
    """(abs_threshold, rel_factor) of RRX_loudness_gate_device for gates given in LUFS / LU: 10 ** ((abs_lufs + 0.691) / 10) and
    10 ** (rel_lu / 10)"""
    return 10.0 ** ((float(abs_lufs) + 0.691) / 10.0), 10.0 ** (float(rel_lu) / 10.0)


def loudness_gate_device(energy, hop, hops=None, abs_lufs=-70.0, rel_lu=-10.0, weights=None, stream=None):
    """The two-stage gate of BS.1770-4 on the device (RRX_loudness_gate_device) over `energy` (float64 [nstreams, nch, nhops], what
    loudness_device / tracks_loudness_device return) for hops of `hop` frames; `hops` (int64 device tensor [nstreams], or None:
    all of them) is the number of valid hops per stream.  `weights`: None (1.0), or per-channel weights as a sequence or a float64
    device tensor [nch] -- BS.1770 gives 1.41 to the surround channels and 0 to the LFE.  Returns float64 [nstreams, 4]:
    S2, N2, S1, N1 per stream; integrated_lufs turns it into LUFS.  The call only enqueues."""
    import torch
    if (energy.dtype != torch.float64 or energy.dim() != 3 or not getattr(energy, "is_cuda", False) or not energy.is_contiguous()):
        raise TypeError("energy must be a contiguous float64 device tensor [nstreams, nch, nhops]")
    nstreams, nch, nhops = energy.shape
    hop = int(hop)
    if hop < 1:
        raise ValueError("a hop has at least one frame")
    dev = energy.device
    if hops is not None and (hops.dtype != torch.int64 or tuple(hops.shape) != (nstreams,) or hops.device != dev or not hops.is_contiguous()):
        raise TypeError("hops must be a contiguous int64 tensor [%d] on %s" % (nstreams, dev))
    if weights is not None and not hasattr(weights, "data_ptr"):
        weights = torch.tensor([float(v) for v in weights], dtype=torch.float64, device=dev)
    if weights is not None and (weights.dtype != torch.float64 or tuple(weights.shape) != (nch,) or weights.device != dev or not weights.is_contiguous()):
        raise TypeError("weights must be %d floats, or a contiguous float64 tensor [%d] on %s" % (nch, nch, dev))
    result = torch.zeros((nstreams, 4), dtype=torch.float64, device=dev)
    if not nstreams or not nch or not nhops:
        return result
    abs_threshold, rel_factor = loudness_gate(abs_lufs, rel_lu)
    _ensure_init()
    _check(lib().RRX_loudness_gate_device(*_where(dev, stream), energy.data_ptr(), nhops,
                                          nstreams, nch, nhops, _ptr(hops),
                                          _ptr(weights), hop, abs_threshold, rel_factor,
                                          result.data_ptr()), "RRX_loudness_gate_device")
    return result


def integrated_lufs(result):
    """LUFS per stream from the gate's result [nstreams, 4] (a torch tensor, on the device or not; anything else is converted):
    -0.691 + 10 log10(S2 / N2), and -inf where no block passed the gates (N2 == 0).  Runs where the tensor lives, without a host
    synchronisation."""
    import torch
    r = result if hasattr(result, "data_ptr") else torch.as_tensor(np.asarray(result, dtype=np.float64))
    s2, n2 = r[..., 0], r[..., 1]
    some = n2 > 0
    mean = s2 / torch.where(some, n2, torch.ones_like(n2))
    return torch.where(some, -0.691 + 10.0 * torch.log10(mean), torch.full_like(mean, float("-inf")))


def loudness_normalizing_gain(lufs, n2, m, target_lufs=-18.0, max_dbtp=-1.0):
    """The gain of convert_tracks_to_pcm_loudness_normalized from its measurements (torch tensors [ntracks]: integrated_lufs, the
    gate's N2, and m = the largest of true peak and sample peak): min(10 ** ((target_lufs - lufs) / 20), 10 ** (max_dbtp / 20) / m),
    and 1.0 where N2 == 0 or m is 0 or not finite."""
    import torch
    ok = (n2 > 0) & torch.isfinite(m) & (m > 0)
    by_loudness = torch.pow(10.0, (float(target_lufs) - torch.where(ok, lufs, torch.zeros_like(lufs))) / 20.0)
    by_peak = torch.full_like(m, 10.0 ** (float(max_dbtp) / 20.0)) / torch.where(ok, m, torch.ones_like(m))
    return torch.where(ok, torch.minimum(by_loudness, by_peak), torch.ones_like(m)).contiguous()


def _loudness_blocks(energy, hop, block_hops, step_hops, hops, weights, stream, want_blocks=True):
    """loudness_blocks_device; want_blocks = False: the maximum alone (blocks and nblocks come back as None)"""
    import torch
    if (energy.dtype != torch.float64 or energy.dim() != 3 or not getattr(energy, "is_cuda", False) or not energy.is_contiguous()):
        raise TypeError("energy must be a contiguous float64 device tensor [nstreams, nch, nhops]")
    nstreams, nch, nhops = energy.shape
    hop, L, P = int(hop), int(block_hops), int(step_hops)
    if hop < 1:
        raise ValueError("a hop has at least one frame")
    if L < 1 or P < 1:
        raise ValueError("a block has at least one hop, and so has the step between blocks")
    dev = energy.device
    if hops is not None and (hops.dtype != torch.int64 or tuple(hops.shape) != (nstreams,) or hops.device != dev or not hops.is_contiguous()):
        raise TypeError("hops must be a contiguous int64 tensor [%d] on %s" % (nstreams, dev))
    if weights is not None and not hasattr(weights, "data_ptr"):
        weights = torch.tensor([float(v) for v in weights], dtype=torch.float64, device=dev)
    if weights is not None and (weights.dtype != torch.float64 or tuple(weights.shape) != (nch,) or weights.device != dev or not weights.is_contiguous()):
        raise TypeError("weights must be %d floats, or a contiguous float64 tensor [%d] on %s" % (nch, nch, dev))
    most = 0 if nhops < L else (nhops - L) // P + 1
    blocks = torch.zeros((nstreams, max(most, 1)), dtype=torch.float64, device=dev) if want_blocks else None
    nblocks = torch.zeros((nstreams,), dtype=torch.int64, device=dev) if want_blocks else None
    peak = torch.zeros((nstreams,), dtype=torch.float64, device=dev)
    if not nstreams or not nch or not most:  # (no block anywhere: an empty tensor has no pointer, and there is nothing to do)
        return blocks, nblocks, peak
    _ensure_init()
    _check(lib().RRX_loudness_blocks_device(*_where(dev, stream), energy.data_ptr(), nhops,
                                            nstreams, nch, nhops, _ptr(hops),
                                            _ptr(weights), hop, L, P,
                                            _ptr(blocks) if want_blocks else None, blocks.shape[1] if want_blocks else 0,
                                            _ptr(nblocks) if want_blocks else None, peak.data_ptr()),
           "RRX_loudness_blocks_device")
    return blocks, nblocks, peak


def loudness_blocks_device(energy, hop, block_hops, step_hops=1, hops=None, weights=None, stream=None):
    """Sliding block powers on the device (RRX_loudness_blocks_device) over `energy`, `hop`, `hops` and `weights` as in
    loudness_gate_device: blocks of `block_hops` hops every `step_hops` hops -- (4, 1) is momentary loudness, (30, 1) short-term,
    (30, 10) the 3 s blocks every second that loudness range is commonly computed on.  Returns (blocks float64 [nstreams, most],
    nblocks int64 [nstreams], max float64 [nstreams]): stream s's first nblocks[s] blocks are written (`most` is what nhops hops
    give, at least one column), and max[s] is the largest of them, +0.0 without one.  -0.691 + 10 log10 of a block is its loudness
    in LUFS.  The call only enqueues."""
    return _loudness_blocks(energy, hop, block_hops, step_hops, hops, weights, stream)


def _loudness_groups(blocks, nblocks, groups, ngroups):
    """the arguments of the two calls over groups, checked: (nstreams, stride, groups as an int32 device tensor, ngroups)"""
    import torch
    if blocks.dtype != torch.float64 or blocks.dim() != 2 or not getattr(blocks, "is_cuda", False) or not blocks.is_contiguous():
        raise TypeError("blocks must be a contiguous float64 device tensor [nstreams, stride]")
    nstreams, stride = blocks.shape
    dev = blocks.device
    if nblocks.dtype != torch.int64 or tuple(nblocks.shape) != (nstreams,) or nblocks.device != dev or not nblocks.is_contiguous():
        raise TypeError("nblocks must be a contiguous int64 tensor [%d] on %s" % (nstreams, dev))
    if groups is None:
        if ngroups is not None and int(ngroups) != nstreams:
            raise ValueError("without groups every stream is its own group: ngroups is %d" % nstreams)
        groups, ngroups = torch.arange(nstreams, dtype=torch.int32, device=dev), nstreams
    elif ngroups is None:
        raise ValueError("give ngroups with the groups")
    elif not hasattr(groups, "data_ptr"):
        groups = torch.tensor([int(v) for v in groups], dtype=torch.int32, device=dev)
    if groups.dtype != torch.int32 or tuple(groups.shape) != (nstreams,) or groups.device != dev or not groups.is_contiguous():
        raise TypeError("groups must be %d ints, or a contiguous int32 tensor [%d] on %s" % (nstreams, nstreams, dev))
    ngroups = int(ngroups)
    if nstreams and ngroups < 1:
        raise ValueError("there is at least one group")
    return nstreams, stride, groups, ngroups


def loudness_gate_groups_device(blocks, nblocks, groups, ngroups, abs_lufs=-70.0, rel_lu=-10.0, stream=None):
    """The two-stage gate of BS.1770-4 over the POOLED blocks of groups of streams (RRX_loudness_gate_groups_device): `blocks` and
    `nblocks` are what loudness_blocks_device returned -- (4, 1) blocks for the integrated loudness -- and may be concatenated from
    several batches; `groups` (a sequence of ints, or an int32 device tensor [nstreams]) gives every stream's group in
    [0, ngroups), any other value keeps the stream out of all groups.  Returns float64 [ngroups, 4]: S2, N2, S1, N1 per group,
    which integrated_lufs turns into LUFS: the album loudness of ReplayGain 2.0 when a group is an album's tracks.  The call only
    enqueues."""
    import torch
    nstreams, stride, groups, ngroups = _loudness_groups(blocks, nblocks, groups, ngroups)
    dev = blocks.device
    result = torch.zeros((ngroups, 4), dtype=torch.float64, device=dev)
    if not nstreams:
        return result
    abs_threshold, rel_factor = loudness_gate(abs_lufs, rel_lu)
    work = torch.empty((2 * nstreams + ngroups,), dtype=torch.float64, device=dev)
    _ensure_init()
    _check(lib().RRX_loudness_gate_groups_device(*_where(dev, stream), _ptr(blocks),
                                                 stride, nstreams, _ptr(nblocks), groups.data_ptr(), ngroups,
                                                 abs_threshold, rel_factor, result.data_ptr(), work.data_ptr(),
                                                 work.numel()), "RRX_loudness_gate_groups_device")
    return result


def loudness_range_device(blocks, nblocks, groups=None, ngroups=None, abs_lufs=-70.0, rel_lu=-20.0, low=10, high=95, stream=None):
    """Gated percentiles per group by exact selection (RRX_loudness_range_groups_device), the two ends of the loudness range of
    EBU Tech 3342: arguments as in loudness_gate_groups_device -- (30, 10) or (30, 1) blocks -- with `groups` = None for every
    stream as its own group.  Returns float64 [ngroups, 4]: P_low, P_high (the `low`-th and `high`-th percentile of the blocks that
    pass both gates, as block powers), N2 (their number) and T (the relative threshold); loudness_range_lu turns it into LU.  The
    call only enqueues."""
    import torch
    low, high = int(low), int(high)
    if not (0 <= low <= 100 and 0 <= high <= 100):
        raise ValueError("a percentile lies in 0..100")
    nstreams, stride, groups, ngroups = _loudness_groups(blocks, nblocks, groups, ngroups)
    dev = blocks.device
    result = torch.zeros((ngroups, 4), dtype=torch.float64, device=dev)
    if not nstreams:
        return result
    abs_threshold, rel_factor = loudness_gate(abs_lufs, rel_lu)
    work = torch.empty((2 * nstreams + ngroups,), dtype=torch.float64, device=dev)
    _ensure_init()
    _check(lib().RRX_loudness_range_groups_device(*_where(dev, stream), _ptr(blocks),
                                                  stride, nstreams, _ptr(nblocks), groups.data_ptr(), ngroups,
                                                  abs_threshold, rel_factor, low, high, result.data_ptr(),
                                                  work.data_ptr(), work.numel()), "RRX_loudness_range_groups_device")
    return result


def loudness_range_lu(result):
    """Loudness range in LU from loudness_range_device's result [ngroups, 4] (a torch tensor, on the device or not; anything else
    is converted): 10 log10(P_high / P_low), and 0.0 where no block passed the gates (N2 == 0).  Runs where the tensor lives."""
    import torch
    r = result if hasattr(result, "data_ptr") else torch.as_tensor(np.asarray(result, dtype=np.float64))
    some = r[..., 2] > 0
    one = torch.ones_like(r[..., 0])
    return torch.where(some, 10.0 * torch.log10(torch.where(some, r[..., 1], one) / torch.where(some, r[..., 0], one)), torch.zeros_like(one))


def loudness_meter_device(energy, hop, hops=None, weights=None, groups=None, ngroups=None):
    """The numbers of EBU R 128 from hop energies that stay in HBM (`energy`, `hop`, `hops`, `weights` as in loudness_gate_device),
    on the current stream and without a host synchronisation: a dict of float64 device tensors [nstreams] -- "integrated" (LUFS,
    -inf where no block passed), "momentary_max" and "short_term_max" (LUFS, the largest 400 ms and 3 s block, -inf without one)
    and "range" (LU, on 3 s blocks every second, gates at -70 LUFS and -20 LU, percentiles 10 and 95) -- and, when `groups` and
    `ngroups` are given as in loudness_gate_groups_device, "group_integrated" and "group_range" [ngroups] over the pooled blocks of
    each group.  Built from loudness_blocks_device, loudness_gate_groups_device and loudness_range_device."""
    import torch
    if not getattr(energy, "is_cuda", False):
        raise TypeError("energy must be a contiguous float64 device tensor [nstreams, nch, nhops]")
    cur = torch.cuda.current_stream(energy.device)
    b4, n4, m4 = _loudness_blocks(energy, hop, 4, 1, hops, weights, cur)
    _, _, m30 = _loudness_blocks(energy, hop, 30, 1, hops, weights, cur, want_blocks=False)
    b30, n30, _ = _loudness_blocks(energy, hop, 30, 10, hops, weights, cur)
    own = torch.arange(energy.shape[0], dtype=torch.int32, device=energy.device)
    out = {"integrated": integrated_lufs(loudness_gate_groups_device(b4, n4, own, energy.shape[0], stream=cur)),
           "momentary_max": -0.691 + 10.0 * torch.log10(m4), "short_term_max": -0.691 + 10.0 * torch.log10(m30),
           "range": loudness_range_lu(loudness_range_device(b30, n30, own, energy.shape[0], stream=cur))}
    if groups is not None:
        out["group_integrated"] = integrated_lufs(loudness_gate_groups_device(b4, n4, groups, ngroups, stream=cur))
        out["group_range"] = loudness_range_lu(loudness_range_device(b30, n30, groups, ngroups, stream=cur))
    return out


def scan_tracks_pcm(tracks, rate, album=None, weights=None, filter="bs1770"):
    """A ReplayGain 2.0 / EBU R 128 scan of tracks as they are stored: `tracks` is a list of device tensors of one dtype and
    channel count -- float32 / int16 / int32 [frames, nch], or uint8 [frames, nch * 3] for packed 24 bit -- at `rate` Hz.  One
    torch.cat, tracks_true_peak_packed_device, tracks_loudness_packed_device and loudness_meter_device, on the current stream and
    without a host synchronisation; no float copy, no padding to the longest track, no handle.  Returns a dict of device tensors:
    "true_peak" and "peak" (float64 [ntracks, nch], linear), every key of loudness_meter_device ("integrated", "momentary_max",
    "short_term_max", "range", [ntracks]) and "track_gain_db" = -18 - integrated.  `album`: one group index per track (a sequence
    of ints; any index below 0 keeps the track out of all groups) adds "group_integrated", "group_range", "group_true_peak" /
    "group_peak" (the maximum over each group's tracks and channels, +0.0 for a group without a track) and "album_gain_db" =
    -18 - group_integrated, all [ngroups] with ngroups = the largest index + 1.  `weights` is loudness_gate_device's, `filter`
    true_peak_device's."""
    import torch
    tracks = list(tracks)
    if not tracks:
        raise ValueError("a scan needs at least one track")
    first = tracks[0]
    for t in tracks:
        if not hasattr(t, "data_ptr") or t.dim() != 2 or t.dtype != first.dtype or t.shape[1] != first.shape[1] or t.device != first.device:
            raise TypeError("the tracks must be [frames, nch] tensors of one dtype, channel count and device")
    ngroups = None
    if album is not None:
        album = [int(v) for v in album]
        if len(album) != len(tracks):
            raise ValueError("album has %d entries for %d tracks" % (len(album), len(tracks)))
        ngroups = max(max(album) + 1, 1)
    dev = first.device
    table = packed_plan([t.shape[0] for t in tracks]).to_device(dev)
    packed = torch.cat(tracks).contiguous()
    cur = torch.cuda.current_stream(dev) if getattr(first, "is_cuda", False) else None
    true_peak, peak = tracks_true_peak_packed_device(packed, table, filter=filter, stream=cur)
    hop = int(rate) // 10
    energy, hops = tracks_loudness_packed_device(packed, table, rate=rate, stream=cur)
    out = {"true_peak": true_peak, "peak": peak}
    out.update(loudness_meter_device(energy, hop, hops, weights, album, ngroups))
    out["track_gain_db"] = -18.0 - out["integrated"]
    if album is not None:
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        for key, stat in (("group_true_peak", true_peak), ("group_peak", peak)):
            members = [[i for i, a in enumerate(album) if a == g] for g in range(ngroups)]
            out[key] = torch.stack([stat[m].amax() if m else zero for m in members])
        out["album_gain_db"] = -18.0 - out["group_integrated"]
    return out


def tracks_finish_shaped_device(rows, table, dst_format, dst_total, shaping, segment=65536, gain=None, dither=True, seed=0, out=None, peak=None,
                                clipped=None, stream=None):
    """tracks_finish_device with noise-shaped dither (RRX_tracks_finish_shaped_device): finish_shaped_device per track, in one
    call, with the frames and the segments counted from each track's own first output frame and no state -- whole rows only
    (by windows, with a state per track: tracks_finish_shaped_window_device).
    `shaping` and `segment` are finish_shaped_device's, everything else tracks_finish_device's, except that `dst_format` is never
    None (`out=False` measures only).  Returns (out, peak, clipped).  The call only enqueues."""
    fmt, ntracks, row_frames, nch = _tracks_frames(rows, "rows", "row_frames")
    _shaped_dst_format(dst_format)
    coefs, segment = _shaping(shaping, segment)
    measure = out is False
    seed, dst_total, gain, out, peak, clipped = _tracks_finish_buffers(rows, table, None if measure else dst_format, dst_total, gain, seed,
                                                                       None if measure else out, peak, clipped)
    write = out is not None and dst_total > 0  # (an empty tensor has no pointer: nothing to write is measure only)
    _check(lib().RRX_tracks_finish_shaped_device(*_where(rows.device, stream), table.data_ptr(), ntracks, nch, fmt, rows.data_ptr(), row_frames, dst_format,
                                                 out.data_ptr() if write else None, dst_total, _ptr(gain), 1 if dither else 0, seed,
                                                 C.cast(coefs, C.c_void_p), len(coefs), segment, peak.data_ptr(), clipped.data_ptr()),
           "RRX_tracks_finish_shaped_device")
    return out, peak, clipped


def _tracks_finish_buffers(rows, table, dst_format, dst_total, gain, seed, out, peak, clipped):
    """what tracks_finish_device and its window form share: the arguments checked, `gain` as a tensor or None, and `out`, `peak`
    and `clipped` allocated where they were not passed; (seed, dst_total, gain, out, peak, clipped)"""
    if dst_format not in (None, RRX_FMT_S16, RRX_FMT_S24_3, RRX_FMT_S32):
        raise ValueError("unknown dst_format %r (RRX_FMT_S16, RRX_FMT_S24_3, RRX_FMT_S32 or None)" % (dst_format,))
    ntracks, _, nch = rows.shape
    dev = rows.device
    _tracks_table(table, ntracks, dev)
    seed, dst_total = int(seed), int(dst_total)
    if not 0 <= seed < 1 << 64 or dst_total < 0:
        raise ValueError("seed must fit 64 unsigned bits, dst_total is a frame count")
    gain = _gain(gain, ntracks, dev)
    out = _pcm_out(out, dst_format, (dst_total,), nch, dev)
    peak, clipped = _finish_stats(peak, clipped, ntracks, nch, dev)
    _ensure_init()
    return seed, dst_total, gain, out, peak, clipped


def _state_handed_on(state, state_out, sshape, dev, touched):
    """the state a per-track window call returns.  A call that touches nothing hands on the state that came in (or zeros), as a new
    tensor; any other writes every entry of `state_out`, or of a new tensor"""
    import torch
    if not touched:
        return torch.zeros(sshape, dtype=torch.float64, device=dev) if state is None else state.clone()
    return torch.empty(sshape, dtype=torch.float64, device=dev) if state_out is None else state_out


def tracks_finish_window_device(win, table, row_frames, win_first, win_frames, dst_format, dst_total, gain=None, dither=False, seed=0, out=None,
                                peak=None, clipped=None, stream=None):
    """tracks_finish_device on a window of the output rows (RRX_tracks_finish_window_device): `win`, a contiguous float32 or float64
    device tensor [ntracks, win_stride, nch], holds frames [win_first, win_first + win_frames) of output rows of `row_frames` frames
    that need not exist anywhere.  Of every track's slice the frames inside the window are processed, with the dither index and the
    destination position they have in the whole-row call, so disjoint windows that cover the rows -- in any order, each call given
    the `out`, `peak` and `clipped` the first one returned, which are accumulated into, not reallocated -- leave tracks_finish_device's
    bytes and statistics.  Everything else as in tracks_finish_device.  Returns (out, peak, clipped); the call only enqueues."""
    fmt, ntracks, win_stride, nch = _tracks_frames(win, "win", "win_stride")
    row_frames, win_first, win_frames = _tracks_window(row_frames, win_first, win_frames, win_stride)
    seed, dst_total, gain, out, peak, clipped = _tracks_finish_buffers(win, table, dst_format, dst_total, gain, seed, out, peak, clipped)
    if not win_frames:  # (an empty tensor has no pointer, and there is nothing to do)
        return out, peak, clipped
    write = out is not None and dst_total > 0  # (an empty tensor has no pointer: nothing to write is measure only)
    _check(lib().RRX_tracks_finish_window_device(*_where(win.device, stream), table.data_ptr(), ntracks, nch, fmt, win.data_ptr(), win_stride, row_frames,
                                                 win_first, win_frames, dst_format or 0, out.data_ptr() if write else None, dst_total, _ptr(gain),
                                                 1 if dither else 0, seed, peak.data_ptr(), clipped.data_ptr()), "RRX_tracks_finish_window_device")
    return out, peak, clipped


def tracks_finish_shaped_window_device(win, table, row_frames, win_first, win_frames, dst_format, dst_total, shaping, segment=65536, gain=None,
                                       dither=True, seed=0, state=None, out=None, peak=None, clipped=None, stream=None):
    """tracks_finish_shaped_device on a window of the output rows (RRX_tracks_finish_shaped_window_device): tracks_finish_window_device
    with noise-shaped dither, the error history of every (track, channel) carried from window to window in `state`.

    `win`, `table`, `row_frames`, `win_first`, `win_frames`, `dst_total`, `gain`, `seed`, `out`, `peak`, `clipped` and `stream` are
    tracks_finish_window_device's, `shaping` and `segment` finish_shaped_device's; `dst_format` is never None (`out=False` measures
    only).  `state`: None, or the float64 [ntracks, nch, 16] tensor the call before returned; None is allowed only for the window
    at frame 0 (ValueError otherwise).  UNLIKE the unshaped window call this one depends on the order of the calls: windows that
    partition [0, row_frames), taken in ascending contiguous order, each given the `out`, `peak`, `clipped` and `state` of the one
    before, leave tracks_finish_shaped_device's bytes and statistics; anything else gives other samples.  Returns (out, peak,
    clipped, state): `state` is a NEW tensor on every call, holding every track's history -- handed on unchanged for the tracks the
    window did not touch, and the state that came in (or zeros) when `win_frames` is 0.  The call only enqueues."""
    return _tracks_finish_shaped_window(win, table, row_frames, win_first, win_frames, dst_format, dst_total, shaping, segment, gain, dither, seed,
                                        state, None, out, peak, clipped, stream)


def _tracks_finish_shaped_window(win, table, row_frames, win_first, win_frames, dst_format, dst_total, shaping, segment, gain, dither, seed, state,
                                 state_out, out, peak, clipped, stream):
    """tracks_finish_shaped_window_device with the tensor that receives the state given (`state_out`, checked as `state` is; None:
    a new one), for a caller that hands two tensors to and fro (Resampler._convert_tracks_streamed)"""
    fmt, ntracks, win_stride, nch = _tracks_frames(win, "win", "win_stride")
    _shaped_dst_format(dst_format)
    coefs, segment = _shaping(shaping, segment)
    row_frames, win_first, win_frames = _tracks_window(row_frames, win_first, win_frames, win_stride)
    if state is None and win_first:
        raise ValueError("only the window at frame 0 needs no state: pass the state the call before returned")
    dev = win.device
    sshape = (ntracks, nch, RRX_SHAPE_MAX_ORDER)
    _state_pair(state, state_out, sshape, dev)
    measure = out is False
    seed, dst_total, gain, out, peak, clipped = _tracks_finish_buffers(win, table, None if measure else dst_format, dst_total, gain, seed,
                                                                       None if measure else out, peak, clipped)
    new_state = _state_handed_on(state, state_out, sshape, dev, win_frames and row_frames)
    if not win_frames or not row_frames:  # touches nothing, the state included
        return out, peak, clipped, new_state
    write = out is not None and dst_total > 0  # (an empty tensor has no pointer: nothing to write is measure only)
    _check(lib().RRX_tracks_finish_shaped_window_device(*_where(dev, stream), table.data_ptr(), ntracks, nch, fmt, win.data_ptr(), win_stride, row_frames,
                                                        win_first, win_frames, dst_format, out.data_ptr() if write else None, dst_total, _ptr(gain),
                                                        1 if dither else 0, seed, C.cast(coefs, C.c_void_p), len(coefs), segment, _ptr(state),
                                                        new_state.data_ptr(), peak.data_ptr(), clipped.data_ptr()), "RRX_tracks_finish_shaped_window_device")
    return out, peak, clipped, new_state


def _tracks_measure_window(win, table, row_frames, win_first, win_frames, gain, state, state_out, width):
    """what the two measuring window calls share: `win`, the window, the table, the gain and the two state tensors checked;
    (RRX_FMT_*, ntracks, win_stride, nch, row_frames, win_first, win_frames, gain, state shape)"""
    fmt, ntracks, win_stride, nch = _tracks_frames(win, "win", "win_stride")
    row_frames, win_first, win_frames = _tracks_window(row_frames, win_first, win_frames, win_stride)
    if state is None and win_first:
        raise ValueError("only the window at frame 0 needs no state: pass the state the call before returned")
    dev = win.device
    _tracks_table(table, ntracks, dev)
    gain = _gain(gain, ntracks, dev)
    sshape = (ntracks, nch, width)
    _state_pair(state, state_out, sshape, dev)
    return fmt, ntracks, win_stride, nch, row_frames, win_first, win_frames, gain, sshape


def tracks_true_peak_window_device(win, table, row_frames, win_first, win_frames, gain=None, filter="bs1770", state=None, true_peak=None,
                                   peak=None, stream=None):
    """tracks_true_peak_device on a window of the output rows (RRX_tracks_true_peak_window_device): `win`, `table`, `row_frames`,
    `win_first` and `win_frames` are tracks_finish_window_device's, `gain` and `filter` tracks_true_peak_device's.  The filter's
    history of every (track, channel) is carried from window to window in `state`: None, or the float64 [ntracks, nch, 16] tensor
    the call before returned; None is allowed only for the window at frame 0 (ValueError otherwise).  Windows that partition
    [0, row_frames), taken in ascending contiguous order, each given the `true_peak`, `peak` and `state` of the one before, leave
    tracks_true_peak_device's bits; anything else gives other numbers.  Returns (true_peak, peak, state): `state` is a NEW tensor
    on every call -- handed on unchanged for the tracks the window did not touch, and the state that came in (or zeros) when
    `win_frames` is 0.  The call only enqueues."""
    return _tracks_true_peak_window(win, table, row_frames, win_first, win_frames, gain, filter, state, None, true_peak, peak, stream)


def _tracks_true_peak_window(win, table, row_frames, win_first, win_frames, gain, filter, state, state_out, true_peak, peak, stream):
    """tracks_true_peak_window_device with the tensor that receives the state given (`state_out`; None: a new one)"""
    fmt, ntracks, win_stride, nch, row_frames, win_first, win_frames, gain, sshape = _tracks_measure_window(
        win, table, row_frames, win_first, win_frames, gain, state, state_out, RRX_TP_MAX_TAPS)
    phases, taps, coefs = _true_peak_filter(filter)
    dev = win.device
    true_peak, peak = _true_peak_stats(true_peak, peak, ntracks, nch, dev)
    new_state = _state_handed_on(state, state_out, sshape, dev, win_frames and row_frames)
    if not win_frames or not row_frames:  # touches nothing, the state included
        return true_peak, peak, new_state
    _ensure_init()
    _check(lib().RRX_tracks_true_peak_window_device(*_where(dev, stream), table.data_ptr(), ntracks, nch, fmt, win.data_ptr(), win_stride, row_frames,
                                                    win_first, win_frames, _ptr(gain), C.cast(coefs, C.c_void_p), phases, taps, _ptr(state),
                                                    new_state.data_ptr(), true_peak.data_ptr(), peak.data_ptr()), "RRX_tracks_true_peak_window_device")
    return true_peak, peak, new_state


def tracks_loudness_window_device(win, table, row_frames, win_first, win_frames, rate=None, gain=None, coefs=None, hop=None, state=None,
                                  energy=None, hops=None, work=None, stream=None):
    """tracks_loudness_device on a window of the output rows (RRX_tracks_loudness_window_device): `win`, `table`, `row_frames`,
    `win_first` and `win_frames` are tracks_finish_window_device's, `rate`, `gain`, `coefs` and `hop` tracks_loudness_device's.
    Hops are counted from every track's own first output frame, so a window cuts them anywhere -- it may be shorter than a hop --
    and `state` carries the hop in progress of every (track, channel): None, or the float64 [ntracks, nch, 16] tensor the call
    before returned; None is allowed only for the window at frame 0 (ValueError otherwise).  `energy` (float64 [ntracks, nch,
    nhops]) is allocated zeroed, with row_frames // hop hops, when not passed; one that is passed may hold fewer, and the tracks'
    hops are clamped to it.  The call WRITES the energies of the hops that complete in this window and leaves the others alone.
    `hops` (int64 [ntracks]) receives every track's hop count; `work` is scratch of RRX_tracks_loudness_window_work_doubles
    doubles; both are allocated when not passed.  Windows that partition [0, row_frames), taken in ascending contiguous order, each
    given the `energy` and `state` of the one before, leave tracks_loudness_device's energies and hops, bit for bit.  Returns
    (energy, hops, state): `state` is a NEW tensor on every call, as in tracks_true_peak_window_device.  The call only enqueues."""
    return _tracks_loudness_window(win, table, row_frames, win_first, win_frames, rate, gain, coefs, hop, state, None, energy, hops, work, stream)


def _tracks_loudness_window(win, table, row_frames, win_first, win_frames, rate, gain, coefs, hop, state, state_out, energy, hops, work, stream):
    """tracks_loudness_window_device with the tensor that receives the state given (`state_out`; None: a new one)"""
    import torch
    fmt, ntracks, win_stride, nch, row_frames, win_first, win_frames, gain, sshape = _tracks_measure_window(
        win, table, row_frames, win_first, win_frames, gain, state, state_out, RRX_LOUDNESS_WIN_STATE)
    c, hop = _loudness_filter(rate, coefs, hop)
    dev = win.device
    need = ntracks * nch * (win_frames // hop + 2) * 4
    energy, work = _loudness_buffers(energy, work, ntracks, nch, row_frames // hop if energy is None else 0, need, dev)
    if hops is None:
        hops = torch.zeros((ntracks,), dtype=torch.int64, device=dev)
    elif hops.dtype != torch.int64 or tuple(hops.shape) != (ntracks,) or hops.device != dev or not hops.is_contiguous():
        raise TypeError("hops must be a contiguous int64 tensor [%d] on %s" % (ntracks, dev))
    new_state = _state_handed_on(state, state_out, sshape, dev, win_frames and row_frames)
    if not win_frames or not row_frames:  # touches nothing, the state included
        return energy, hops, new_state
    _ensure_init()
    if not energy.shape[2]:  # (an empty tensor has no pointer; no hop is written through this one)
        energy_ptr = torch.zeros((1,), dtype=torch.float64, device=dev)
    else:
        energy_ptr = energy
    _check(lib().RRX_tracks_loudness_window_device(*_where(dev, stream), table.data_ptr(), ntracks, nch, fmt, win.data_ptr(), win_stride, row_frames,
                                                   win_first, win_frames, _ptr(gain), C.cast(c, C.c_void_p), hop, _ptr(state), new_state.data_ptr(),
                                                   energy_ptr.data_ptr(), energy.shape[2], _ptr(hops), work.data_ptr(), work.numel()),
           "RRX_tracks_loudness_window_device")
    return energy, hops, new_state


class _WindowMeter:
    """The measuring pass of the streamed normalising conversions (Resampler._convert_tracks_streamed, `measure=`): true peak and,
    with `rate`, hop energies of every pulled window at the running output position, each through two state tensors handed to and
    fro.  Allocates the states, the statistics, one window's work buffer and ceil(longest output row / hop) hop energies per
    (stream, channel); `result()` is (true_peak, sample_peak, energy or None, hops or None)."""

    def __init__(self, rate, nch, plan, table, cap, win_out, dev, stream):
        import torch
        self.table, self.cap, self.stream, self.rate = table, cap, stream, rate
        n = table.shape[0]
        f64 = dict(dtype=torch.float64, device=dev)
        self.true_peak, self.peak = torch.zeros((n, nch), **f64), torch.zeros((n, nch), **f64)
        self.tp_states = [torch.zeros((n, nch, RRX_TP_MAX_TAPS), **f64) for _ in range(2)]
        self.energy = self.hops = None
        if rate is not None:
            hop = rate // 10
            need = max(int(e.out_first + e.out_frames) for e in plan.table)
            self.energy = torch.zeros((n, nch, max(1, -(-need // hop))), **f64)
            self.hops = torch.zeros((n,), dtype=torch.int64, device=dev)
            self.work = torch.empty((n * nch * (win_out // hop + 2) * 4,), **f64)
            self.ld_states = [torch.zeros((n, nch, RRX_LOUDNESS_WIN_STATE), **f64) for _ in range(2)]

    def __call__(self, wout, first, frames):
        _tracks_true_peak_window(wout, self.table, self.cap, first, frames, None, "bs1770", self.tp_states[0], self.tp_states[1],
                                 self.true_peak, self.peak, self.stream)
        self.tp_states.reverse()
        if self.rate is not None:
            _tracks_loudness_window(wout, self.table, self.cap, first, frames, self.rate, None, None, None, self.ld_states[0],
                                    self.ld_states[1], self.energy, self.hops, self.work, self.stream)
            self.ld_states.reverse()

    def result(self):
        return self.true_peak, self.peak, self.energy, self.hops


class _WindowLimiter:
    """The limiter between the pull and the next stage of the streamed conversions (Resampler._convert_tracks_streamed, `limit=`).
    A carry buffer per row holds the pulled frames [emitted - back, pulled), (back, ahead) = limit_window_reach(lookahead, hold):
    after every pull the frames [emitted, pulled - ahead) are limited under `gain` into a window buffer of the pulled window's shape
    (tracks_limit_window_device; nothing while that range is empty -- a pulled window may be shorter than `ahead`), and the frames
    still within reach are moved to the front of the second carry buffer, which then takes the first one's place.  `flush(got)`
    emits the rest, in pieces no longer than a pulled window, with the rows as long as what was delivered.  The emitted windows are
    ascending and contiguous from frame 0.  Memory: 2 * (back + ahead + window) + window frames per row; `reduction` and `limited`
    are accumulated into.  With `release` = (pole, block) the windows go through tracks_limit_release_window_device instead --
    their order is the one it needs -- and two [rows, 8] state buffers take turns as its state_in and state_out, the first window
    starting without one."""

    def __init__(self, ceiling, gain, lookahead, hold, reduction, limited, table, cap, wout, stream, release=None):
        import torch
        self.kw = dict(ceiling=ceiling, gain=gain, lookahead=lookahead, hold=hold, reduction=reduction, limited=limited, stream=stream)
        self.release = release
        if release is not None:
            self.states = [torch.zeros((wout.shape[0], RRX_LIMIT_RELEASE_WIN_STATE), dtype=torch.float64, device=wout.device) for _ in range(2)]
        self.table, self.cap = table, cap
        self.back, self.ahead = limit_window_reach(lookahead, hold)
        n, width, nch = wout.shape
        self.bufs = [torch.empty((n, self.back + self.ahead + width, nch), dtype=wout.dtype, device=wout.device) for _ in range(2)]
        self.out = torch.empty_like(wout)
        self.first = self.frames = self.emitted = 0  # the carry buffer holds the frames [first, first + frames) of the rows

    def _emit(self, frames, row_frames):
        if self.release is None:
            tracks_limit_window_device(self.bufs[0], self.table, row_frames, self.first, self.emitted, frames, out=self.out,
                                       buf_frames=self.frames, **self.kw)
        else:
            tracks_limit_release_window_device(self.bufs[0], self.table, row_frames, self.first, self.emitted, frames, release=self.release[0],
                                               block=self.release[1], state_in=self.states[0] if self.emitted else None,
                                               state_out=self.states[1], out=self.out, buf_frames=self.frames, **self.kw)
            self.states.reverse()
        at, self.emitted = self.emitted, self.emitted + frames
        return self.out, at, frames

    def feed(self, wout, k):
        """takes the k frames just pulled into `wout`; (window buffer, first frame, frames) of what can be emitted now, or None"""
        self.bufs[0][:, self.frames:self.frames + k].copy_(wout[:, :k])
        self.frames += k
        frames = self.first + self.frames - self.ahead - self.emitted  # at most k: what could be emitted before has been
        if frames <= 0:
            return None
        window = self._emit(frames, self.cap)
        shift = max(0, self.emitted - self.back) - self.first
        if shift:
            self.bufs[1][:, :self.frames - shift].copy_(self.bufs[0][:, shift:self.frames])
            self.bufs.reverse()
            self.first, self.frames = self.first + shift, self.frames - shift
        return window

    def flush(self, got):
        """after the final pull: the windows that cover the rest, [emitted, got), the rows being `got` frames long"""
        while self.emitted < got:
            yield self._emit(min(self.out.shape[1], got - self.emitted), got)


def _ensure_init():
    global _inited
    if not _inited:
        if lib().init_ratelib(_alloc_cb) != 0:
            raise RuntimeError("init_ratelib failed: no usable HIP device (the engine has no CPU path)")
        _inited = True


def _check(rc, what):
    if rc:
        raise RRError(rc, what)


# -- the shared gain expressions of the Resampler.convert_tracks_to_pcm_* family: the streamed forms equal the whole-row forms bit for bit
# -- in gain, trim and lufs because both call these
def _album_checked(album, ntracks):
    """the `album=` of a conversion: None, or one non-negative int per track, as a list"""
    if album is not None:
        album = [int(v) for v in album]
        if len(album) != ntracks or any(v < 0 for v in album):
            raise ValueError("album is one non-negative int per track")
    return album


def _limiter_frames(rate, max_dbtp, lookahead_ms, hold_ms):
    """(ceiling, lookahead, hold) of the limited conversions: max_dbtp as a linear level, the two times rounded to frames of `rate`
    and clamped to what the limiter takes"""
    ceiling = 10.0 ** (float(max_dbtp) / 20.0)
    lookahead = min(max(int(round(float(lookahead_ms) * rate / 1000.0)), 1), RRX_LIMIT_MAX_LOOKAHEAD)
    hold = min(max(int(round(float(hold_ms) * rate / 1000.0)), 0), RRX_LIMIT_MAX_HOLD)
    return ceiling, lookahead, hold


def _largest_peak(true_peak, sample_peak):
    """m [rows]: per row, the largest of true peak and sample peak over its channels"""
    import torch
    return torch.maximum(true_peak, sample_peak).amax(1)


def _peak_normalizing_gain(true_peak, sample_peak, target):
    """the gain that brings every row's largest peak to the linear level `target`; 1.0 where that peak is 0 or not finite"""
    import torch
    m = _largest_peak(true_peak, sample_peak)
    return torch.where(torch.isfinite(m) & (m > 0), torch.full_like(m, target) / m, torch.ones_like(m)).contiguous()  # (one division, one rounding)


def _trim(true_peak, sample_peak, ceiling):
    """min(1, ceiling / m) per row; 1.0 where m, the row's largest peak, is 0 or not finite"""
    import torch
    m = _largest_peak(true_peak, sample_peak)
    ok = torch.isfinite(m) & (m > 0)
    return torch.where(ok, torch.clamp(torch.full_like(m, ceiling) / torch.where(ok, m, torch.ones_like(m)), max=1.0), torch.ones_like(m)).contiguous()


def _loudness_measured(energy, hops, n, album, weights, rate, cur):
    """The gated loudness of the rows' hop energies: (lufs, n2, of).  Without `album`, per row, `of` None.  With it, per album --
    the gate over the pooled 400 ms blocks of an album's tracks -- and `of` the album of each of the `n` tracks as an index tensor;
    the rows without a track are in no album."""
    import torch
    if album is None:
        result = loudness_gate_device(energy, rate // 10, hops=hops, weights=weights, stream=cur)
        return integrated_lufs(result), result[:, 1], None
    dev = energy.device
    of = torch.tensor(album, dtype=torch.int64, device=dev)
    groups = torch.full((energy.shape[0],), -1, dtype=torch.int32, device=dev)
    groups[:n] = of.to(torch.int32)
    blocks, nblocks, _ = loudness_blocks_device(energy, rate // 10, 4, 1, hops=hops, weights=weights, stream=cur)
    result = loudness_gate_groups_device(blocks, nblocks, groups, max(album) + 1, stream=cur)
    return integrated_lufs(result), result[:, 1], of


def _loudness_normalized_gain(lufs, n2, of, m, n, target_lufs, max_dbtp):
    """(gain [rows], lufs per track) of the loudness-normalised conversions from _loudness_measured's answer and m =
    _largest_peak: loudness_normalizing_gain per row, or per album -- with the largest m over the album's tracks -- gathered per
    track"""
    import torch
    if of is None:
        return loudness_normalizing_gain(lufs, n2, m, target_lufs, max_dbtp), lufs
    most = torch.zeros((lufs.shape[0],), dtype=m.dtype, device=m.device).scatter_reduce(0, of, m[:n], "amax", include_self=True)
    gain = torch.ones_like(m)
    gain[:n] = loudness_normalizing_gain(lufs, n2, most, target_lufs, max_dbtp)[of]
    return gain, lufs[of]


def _tracks_views(pcm, plan, n):
    """the first `n` tracks' slices of the packed destination, or None for a call that measured only"""
    return None if pcm is None else [pcm[int(e.dst_first):int(e.dst_first + e.out_frames)] for _, e in zip(range(n), plan.table)]


def _finish_rows(rows, table, plan, n, dst_format, shaping, segment, finish_kw):
    """the tail of the whole-row conversions: the rows finished, shaped or not, and cut per track; (views, peak, clipped)"""
    if shaping is not None:
        pcm, peak, clipped = tracks_finish_shaped_device(rows, table, dst_format, plan.dst_total, shaping, segment, **finish_kw)
    else:
        pcm, peak, clipped = tracks_finish_device(rows, table, dst_format, plan.dst_total, **finish_kw)
    return _tracks_views(pcm, plan, n), peak[:n], clipped[:n]


class Resampler:
    """One RR_handle (optionally a batch of lock-stepped streams).

    Host arrays are numpy float32 shaped [frames, nch] (one stream) or [streams, frames, nch].
    Device buffers are anything with `data_ptr()` (torch CUDA tensors) of the same shapes.
    dtype=np.float64 opens a double-format handle (RRX_open_batch_fmt, RRX_FMT_DOUBLE): host arrays and device tensors are
    then float64 and go through the RRX_*_double calls.  A buffer of the other precision is refused before any C call.
    sample_format=RRX_FMT_S16 / RRX_FMT_S32 opens an integer PCM handle: host arrays are int16 / int32, device tensors
    torch.int16 / torch.int32, and every data call goes through the format-tagged RRX_*_samples calls (conversions:
    ratelib_amd.h).  `dtype` keeps meaning float32 or float64 only; `self.dtype` is the handle's sample dtype.
    What a handle accepts: an integer handle takes arrays and tensors of exactly its own dtype.  A float or double handle
    refuses the other float precision and the two PCM dtypes (int16, int32: data meant for an integer handle); anything else
    (lists, float16, int8, uint8, int64 ...) is converted to the handle's dtype by value, as numpy does, with no PCM scaling.
    A wrong type is a TypeError, an unknown `sample_format` value a ValueError, both before any C call.
    """

    def __init__(self, in_rate, out_rate, nch=2, nstreams=1, device=None, dtype=None, sample_format=None, **kw):
        if dtype is not None:
            dtype = np.dtype(dtype)
            if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
                raise TypeError("Resampler dtype must be float32 or float64, not %s (integer PCM: sample_format=RRX_FMT_S16 / "
                                "RRX_FMT_S32)" % dtype)
        if sample_format is not None:
            if sample_format not in _FMT_DTYPE:
                raise ValueError("unknown sample_format %r" % (sample_format,))
            if dtype is not None and dtype != _FMT_DTYPE[sample_format]:
                raise TypeError("dtype %s does not go with sample_format %r: give one of the two" % (dtype, sample_format))
            dtype = _FMT_DTYPE[sample_format]
        elif dtype is None:
            dtype = np.dtype(np.float32)
        _ensure_init()
        self.L = lib()
        self.nch, self.nstreams = nch, nstreams
        self.dtype = dtype
        self.cfg = _config(in_rate, out_rate, **kw)
        self.h = C.c_void_p()
        self._stream = None  # the caller's hipStream_t (an integer) after set_stream, None while the handle uses its own
        self._used = False   # a data call has moved the handle away from its just-opened state (reset() brings it back)
        if dtype != np.float32:
            _check(self.L.RRX_open_batch_fmt(C.byref(self.cfg), nch, nstreams, -1 if device is None else int(device), _DTYPE_FMT[dtype],
                                             C.byref(self.h)), "RRX_open_batch_fmt")
        elif device is not None:  # explicit HIP device index (RRX_open_batch_on)
            _check(self.L.RRX_open_batch_on(C.byref(self.cfg), nch, nstreams, int(device), C.byref(self.h)), "RRX_open_batch_on")
        elif nstreams == 1:
            _check(self.L.RR_open(C.byref(self.cfg), nch, C.byref(self.h)), "RR_open")
        else:
            _check(self.L.RRX_open_batch(C.byref(self.cfg), nch, nstreams, C.byref(self.h)), "RRX_open_batch")

    # -- lifecycle
    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.L.RR_close(C.byref(self.h))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def double(self):
        return self.dtype == np.float64

    @property
    def integer(self):
        """The handle takes and gives integer PCM frames (RRX_FMT_S16 / RRX_FMT_S32)."""
        return self.dtype.kind == "i"

    @property
    def sample_format(self):
        """The RRX_FMT_* that goes with the handle's sample dtype (what the *_samples calls are tagged with)."""
        return _DTYPE_FMT[self.dtype]

    @property
    def format(self):
        """RRX_format of the handle (RRX_FMT_*)."""
        return self.L.RRX_format(self.h)

    @property
    def device(self):
        return self.L.RRX_device(self.h)

    @property
    def isamp_max(self):
        return self.L.RRX_isamp_max(self.h)

    @property
    def available(self):
        return self.L.RRX_available(self.h)

    def set_stream(self, hip_stream_ptr):
        """hipStream_t as an integer (torch: stream.cuda_stream); 0 / None = the default stream."""
        _check(self.L.RRX_set_stream(self.h, C.c_void_p(hip_stream_ptr or 0)), "RRX_set_stream")
        self._stream = int(hip_stream_ptr or 0)

    def use_own_stream(self):
        """Back to the stream the handle created for itself (RRX_STREAM_OWN)."""
        _check(self.L.RRX_set_stream(self.h, C.c_void_p(C.c_size_t(-1).value)), "RRX_set_stream")
        self._stream = None

    def sync(self):
        _check(self.L.RRX_sync(self.h), "RRX_sync")

    def reset(self):
        """Back to the just-opened state (RRX_reset): whatever the handle holds is dropped, and every sample it produces from now
        on is bit for bit what a fresh Resampler of the same arguments produces.  The stream, the profiling switch and every
        allocation stay; the call only enqueues.  This is how one handle takes track after track."""
        _check(self.L.RRX_reset(self.h), "RRX_reset")
        self._used = False

    def profile(self, enable=True):
        _check(self.L.RRX_profile(self.h, 1 if enable else 0), "RRX_profile")

    def profile_read(self):
        hm, om = C.c_double(0), C.c_double(0)
        hn, on = C.c_longlong(0), C.c_longlong(0)
        _check(self.L.RRX_profile_read(self.h, C.byref(hm), C.byref(hn), C.byref(om), C.byref(on)), "RRX_profile_read")
        return {"hot_ms": hm.value, "hot_launches": hn.value, "other_ms": om.value, "other_launches": on.value}

    def profile_report(self):
        """Per-kernel records since the last read: [{"kernel", "hot", "launches", "ms"}, ...]."""
        buf = C.create_string_buffer(1 << 14)
        n = self.L.RRX_profile_report(self.h, buf, len(buf))
        if n < 0:
            raise RRError(-n, "RRX_profile_report")
        return json.loads(buf.value.decode())

    # -- host API (RR_push / RR_pull / RR_flow / RR_drain)
    def _host_in(self, x):
        xd = getattr(x, "dtype", None)
        if self.integer:
            if xd != self.dtype:
                raise TypeError("%s samples on an %s handle: integer PCM handles take arrays of their own dtype only" % (xd, self.dtype))
        elif xd is not None and np.dtype(xd) in (np.dtype(np.int16), np.dtype(np.int32)):
            raise TypeError("%s samples on a %s handle: open the Resampler with sample_format=RRX_FMT_S16 / RRX_FMT_S32" % (xd, self.dtype))
        if getattr(x, "dtype", None) == np.float64 and not self.double:
            raise TypeError("float64 samples on a float32 handle: open the Resampler with dtype=np.float64")
        if getattr(x, "dtype", None) == np.float32 and self.double:
            raise TypeError("float32 samples on a float64 handle: pass float64 arrays (or open it with dtype=np.float32)")
        x = np.ascontiguousarray(x, dtype=self.dtype)
        if self.nstreams == 1:
            x = x.reshape(-1, self.nch)
            return x, x.shape[0]
        x = x.reshape(self.nstreams, -1, self.nch)
        return x, x.shape[1]

    def push(self, x):
        x, n = self._host_in(x)
        if n == 0:
            return
        self._used = True
        if self.integer:
            _check(self.L.RRX_push_samples(self.h, self.sample_format, x.ctypes.data, n, n), "RRX_push_samples")
        elif self.double:
            _check(self.L.RRX_push_double(self.h, x.ctypes.data, n, n), "RRX_push_double")
        elif self.nstreams == 1:
            _check(self.L.RR_push(self.h, x.ctypes.data, n), "RR_push")
        else:
            _check(self.L.RRX_push_strided(self.h, x.ctypes.data, n, n), "RRX_push_strided")

    def pull(self, max_frames):
        shape = (max_frames, self.nch) if self.nstreams == 1 else (self.nstreams, max_frames, self.nch)
        out = np.empty(shape, dtype=self.dtype)
        n = C.c_size_t(0)
        if self.integer:
            _check(self.L.RRX_pull_samples(self.h, self.sample_format, out.ctypes.data, max_frames, max_frames, C.byref(n)), "RRX_pull_samples")
            return out[: n.value] if self.nstreams == 1 else out[:, : n.value]
        if self.double:
            _check(self.L.RRX_pull_double(self.h, out.ctypes.data, max_frames, max_frames, C.byref(n)), "RRX_pull_double")
            return out[: n.value] if self.nstreams == 1 else out[:, : n.value]
        if self.nstreams == 1:
            _check(self.L.RR_pull(self.h, out.ctypes.data, max_frames, C.byref(n)), "RR_pull")
            return out[: n.value]
        _check(self.L.RRX_pull_strided(self.h, out.ctypes.data, max_frames, max_frames, C.byref(n)), "RRX_pull_strided")
        return out[:, : n.value]

    def pull_all(self, chunk=1 << 16):
        parts = []
        ax = 0 if self.nstreams == 1 else 1
        while True:
            p = self.pull(chunk)
            if p.shape[ax] == 0:
                break
            parts.append(p.copy())
        if parts:
            return np.concatenate(parts, axis=ax)
        return np.empty((0, self.nch) if self.nstreams == 1 else (self.nstreams, 0, self.nch), self.dtype)

    def flow(self, x, max_out):
        assert self.nstreams == 1
        x, n = self._host_in(x)
        out = np.empty((max_out, self.nch), dtype=self.dtype)
        iu, og = C.c_size_t(0), C.c_size_t(0)
        self._used = True
        if self.integer:
            _check(self.L.RRX_flow_samples(self.h, self.sample_format, x.ctypes.data if n else None, n, out.ctypes.data, max_out, n,
                                           max_out, C.byref(iu), C.byref(og)), "RRX_flow_samples")
            return iu.value, out[: og.value]
        if self.double:
            _check(self.L.RRX_flow_double(self.h, x.ctypes.data if n else None, n, out.ctypes.data, max_out, n, max_out,
                                          C.byref(iu), C.byref(og)), "RRX_flow_double")
            return iu.value, out[: og.value]
        _check(self.L.RR_flow(self.h, x.ctypes.data if n else None, out.ctypes.data, n, max_out, C.byref(iu), C.byref(og)),
               "RR_flow")
        return iu.value, out[: og.value]

    def drain(self):
        self._used = True
        _check(self.L.RR_drain(self.h), "RR_drain")

    def process(self, x, chunk=None):
        """push everything in `chunk`-frame pushes (default isamp_max), drain, return all output."""
        x, n = self._host_in(x)
        chunk = chunk or self.isamp_max
        ax = 0 if self.nstreams == 1 else 1
        parts = []
        for s in range(0, n, chunk):
            self.push(x[s:s + chunk] if self.nstreams == 1 else x[:, s:s + chunk])
            parts.append(self.pull_all())
        self.drain()
        parts.append(self.pull_all())
        return np.concatenate(parts, axis=ax)

    # -- device API (buffers expose data_ptr(); strides in frames)
    def _dev_check(self, t):
        """A tensor whose dtype names the other precision is refused (torch.float32 / torch.float64 vs the handle)."""
        dt = str(getattr(t, "dtype", ""))
        if self.integer:
            if not dt.endswith("." + self.dtype.name) and dt != self.dtype.name:
                raise TypeError("%s buffer on an %s handle: integer PCM handles take tensors of their own dtype only" % (dt or "untyped", self.dtype))
            return C.c_void_p(t.data_ptr())
        if dt.endswith("int16") or dt.endswith("int32"):
            raise TypeError("%s buffer on a %s handle: open the Resampler with sample_format=RRX_FMT_S16 / RRX_FMT_S32" % (dt, self.dtype))
        if dt.endswith("float64") and not self.double:
            raise TypeError("torch.float64 buffer on a float32 handle: open the Resampler with dtype=np.float64")
        if dt.endswith("float32") and self.double:
            raise TypeError("torch.float32 buffer on a float64 handle: pass torch.float64 tensors")
        return C.c_void_p(t.data_ptr())

    def push_device(self, t, frames, stride=None):
        p = self._dev_check(t)
        self._used = True
        if self.integer:
            _check(self.L.RRX_push_device_samples(self.h, self.sample_format, p, stride or frames, frames), "RRX_push_device_samples")
            return
        if self.double:
            _check(self.L.RRX_push_device_double(self.h, p, stride or frames, frames), "RRX_push_device_double")
            return
        _check(self.L.RRX_push_device(self.h, p, stride or frames, frames), "RRX_push_device")

    def pull_device(self, t, max_frames, stride=None):
        n = C.c_size_t(0)
        p = self._dev_check(t)
        if self.integer:
            _check(self.L.RRX_pull_device_samples(self.h, self.sample_format, p, stride or max_frames, max_frames, C.byref(n)),
                   "RRX_pull_device_samples")
            return n.value
        if self.double:
            _check(self.L.RRX_pull_device_double(self.h, p, stride or max_frames, max_frames, C.byref(n)), "RRX_pull_device_double")
            return n.value
        _check(self.L.RRX_pull_device(self.h, p, stride or max_frames, max_frames, C.byref(n)),
               "RRX_pull_device")
        return n.value

    def flow_device(self, tin, in_frames, tout, out_cap, in_stride=None, out_stride=None):
        iu, og = C.c_size_t(0), C.c_size_t(0)
        if tin is not None:
            self._dev_check(tin)
        self._dev_check(tout)
        self._used = True
        if self.integer:
            _check(self.L.RRX_flow_device_samples(self.h, self.sample_format, C.c_void_p(tin.data_ptr()) if tin is not None else None,
                                                  in_stride or in_frames, C.c_void_p(tout.data_ptr()), out_stride or out_cap,
                                                  in_frames, out_cap, C.byref(iu), C.byref(og)), "RRX_flow_device_samples")
            return iu.value, og.value
        if self.double:
            _check(self.L.RRX_flow_device_double(self.h, C.c_void_p(tin.data_ptr()) if tin is not None else None,
                                                 in_stride or in_frames, C.c_void_p(tout.data_ptr()), out_stride or out_cap,
                                                 in_frames, out_cap, C.byref(iu), C.byref(og)), "RRX_flow_device_double")
            return iu.value, og.value
        _check(self.L.RRX_flow_device(self.h, C.c_void_p(tin.data_ptr()) if tin is not None else None,
                                      in_stride or in_frames, C.c_void_p(tout.data_ptr()), out_stride or out_cap,
                                      in_frames, out_cap, C.byref(iu), C.byref(og)), "RRX_flow_device")
        return iu.value, og.value

    def convert_track_device(self, x):
        """One whole track per stream, device to device, with the plugin's edge treatment (dsp_rate::on_chunk / flushwrite,
        foo_dsp_rate.cpp:154-168, 218-313) for all streams of the handle at once: `x` is a float32 device tensor
        [nstreams, frames, nch]; the resampled tracks are returned as a new tensor [nstreams, frames_out, nch].

        Up to 2 * LPC_ORDER = 64 frames a track is pushed, drained and pulled as it is (:222-239).  A longer one is extended at
        both ends by n_add frames of LPC extrapolation from its first and its last prime = min(frames, prime_len) frames
        (edge_geometry), pushed in isamp_max-sized pieces and drained, and n_drop frames are cut from each end of what comes out.
        Everything runs on torch's current stream of x's device (the handle is switched to it for the call and back afterwards);
        no sample is copied to the host.  The handle is left drained, as after RR_drain: the plugin gives the next track a handle of
        its own (foo_dsp_rate.cpp:282); this one takes it after reset()."""
        import torch
        if self.dtype != np.float32:
            raise TypeError("convert_track_device needs a float32 handle (the LPC arithmetic is float32), not %s" % self.dtype)
        if tuple(x.shape[::2]) != (self.nstreams, self.nch) or x.dim() != 3:
            raise ValueError("expected a [%d, frames, %d] tensor, got shape %r" % (self.nstreams, self.nch, tuple(x.shape)))
        if x.dtype != torch.float32 or not x.is_cuda or x.device.index != self.device:
            raise TypeError("expected a torch.float32 tensor on the handle's device (cuda:%d)" % self.device)
        x = x.contiguous()
        frames = x.shape[1]
        in_rate, out_rate = self.cfg.in_rate, self.cfg.out_rate
        n_add, n_drop, prime_len, _ = edge_geometry(in_rate, out_rate)
        cur = torch.cuda.current_stream(x.device)
        prev = self._stream
        self.set_stream(cur.cuda_stream)
        try:
            if frames > 64:
                prime = min(frames, prime_len)
                src = x.new_empty((self.nstreams, n_add + frames + n_add, self.nch))
                src[:, n_add:n_add + frames] = x
                lpc_extrapolate_device(src, n_add, prime, n_add, 0, stream=cur)
                lpc_extrapolate_device(src, n_add + frames - prime, prime, 0, n_add, stream=cur)
            else:
                src, n_drop = x, 0
            total = src.shape[1]
            cap = total * out_rate // in_rate + 2  # drain leaves round(total * out_rate / in_rate) frames in all
            out = x.new_empty((self.nstreams, cap, self.nch))
            got = 0

            def pull():
                nonlocal got
                while self.available:
                    if got >= cap:
                        raise RuntimeError("convert_track_device: more output than %d frames in gives" % total)
                    got += self.pull_device(out[:, got:], cap - got, stride=cap)

            step = self.isamp_max
            for pos in range(0, total, step):
                self.push_device(src[:, pos:], min(step, total - pos), stride=total)
                pull()
            self.drain()
            pull()
            return out[:, n_drop:max(got - n_drop, n_drop)].contiguous()
        finally:
            if prev is None:
                self.use_own_stream()
            else:
                self.set_stream(prev)

    def convert_track_to_pcm_device(self, x, dst_format, shaping=None, segment=65536, **finish_kw):
        """convert_track_device followed by the output stage, finish_device(..., dst_format, **finish_kw), on torch's current
        stream of x's device: whole tracks in, integer PCM (and peak / clip count per stream and channel) out.  Returns
        finish_device's (out, peak, clipped).  With `shaping` (a name of NOISE_SHAPES or coefficients) the output stage is
        finish_shaped_device(..., dst_format, shaping, segment, **finish_kw) instead -- noise-shaped dither, on by default there
        -- and the same three values are returned."""
        import torch
        y = self.convert_track_device(x)
        finish_kw.setdefault("stream", torch.cuda.current_stream(y.device))
        if shaping is not None:
            return finish_shaped_device(y, dst_format, shaping, segment, **finish_kw)[:3]
        return finish_device(y, dst_format, **finish_kw)

    def _tracks_mix(self, mix):
        """the `mix=` of a convert_tracks_* call: None, or the matrix [nch, nch_src] checked against the handle's channels"""
        return None if mix is None else _mix_checked(mix, nch_dst=self.nch)

    def _tracks_checked(self, tracks, mix=None, gapless=None):
        """the tracks of a convert_tracks_* call, checked: (list of tracks, plan with the idle streams as zero-length tracks).
        `mix` (a checked matrix): the tracks have its column count of channels, not the handle's.  `gapless`: one group id per
        track, and the plan is album.tracks_plan_album's -- or, from convert_library_to_pcm, a batch's plan as it stands."""
        import torch
        if gapless is not None and mix is not None:
            raise ValueError("gapless= together with mix= is not built")
        if self.dtype != np.float32:
            raise TypeError("convert_tracks_device needs a float32 handle (the LPC arithmetic is float32), not %s" % self.dtype)
        tracks = list(tracks)
        if not 1 <= len(tracks) <= self.nstreams:
            raise ValueError("expected 1 to %d tracks (the handle's streams), got %d" % (self.nstreams, len(tracks)))
        dt = tracks[0].dtype
        if _tracks_src_format(dt) is None:
            raise TypeError("expected float32, int16, int32 or uint8 (packed 24-bit) tensors, not %s" % dt)
        nch_src = self.nch if mix is None else mix.shape[1]
        last = nch_src * 3 if dt == torch.uint8 else nch_src
        for x in tracks:
            if x.dtype != dt:
                raise TypeError("the tracks of one call share a dtype: %s and %s" % (dt, x.dtype))
            if x.dim() != 2 or x.shape[1] != last:
                raise ValueError("expected [frames, %d] %s tensors, got shape %r" % (last, dt, tuple(x.shape)))
            if not x.is_cuda or x.device.index != self.device:
                raise TypeError("expected tensors on the handle's device (cuda:%d)" % self.device)
        # the streams without a track are zero-length tracks: they own no output
        idle = self.nstreams - len(tracks)
        if gapless is None:
            return tracks, _tracks_plan(self.cfg, [x.shape[0] for x in tracks] + [0] * idle)
        if isinstance(gapless, TracksPlan):
            return tracks, gapless
        from . import album
        return tracks, album._tracks_plan_album(self.cfg, [x.shape[0] for x in tracks] + [0] * idle,
                                                album._gapless_checked(gapless, len(tracks)) + [-1] * idle)

    @staticmethod
    def _tracks_staged(tracks, plan, dev):
        """(packed source, device links or None) of a planned batch"""
        import torch
        packed = plan.packed if plan.packed is not None else torch.cat(tracks).contiguous()
        return packed, None if plan.links is None else plan.links_to_device(dev)

    def _convert_tracks_rows(self, tracks, scratch=None, mix=None, gapless=None):
        """convert_tracks_device up to the handle's output rows: (plan, device table, output rows [nstreams, out_row_cap, nch]).
        `scratch` (a _Scratch): the staged rows and the output rows are views of its buffers instead of new tensors.  `mix`: the
        stage call is tracks_stage_mix_device.  `gapless`: it is album.tracks_stage_album_device, on the album plan."""
        import torch
        mix = self._tracks_mix(mix)
        tracks, plan = self._tracks_checked(tracks, mix, gapless)
        dev = tracks[0].device
        table = plan.to_device(dev)
        total, cap = plan.row_frames, plan.out_row_cap
        if scratch is not None:
            out = scratch.take("out_rows", (self.nstreams, cap, self.nch), dev)
        else:
            out = torch.empty((self.nstreams, cap, self.nch), dtype=torch.float32, device=dev)  # (the handle's rows are float32 whatever the tracks are)
        if not total:  # nothing but zero-length tracks
            return plan, table, out
        cur = torch.cuda.current_stream(dev)
        prev = self._stream
        self.set_stream(cur.cuda_stream)
        try:
            rows = None if scratch is None else scratch.take("rows", (self.nstreams, total, self.nch), dev)
            if gapless is not None:
                from . import album
                packed, links = self._tracks_staged(tracks, plan, dev)
                src = album.tracks_stage_album_device(packed, table, links, self.cfg.in_rate, self.cfg.out_rate, total, out=rows, stream=cur)
            elif mix is None:
                src = tracks_stage_device(torch.cat(tracks).contiguous(), table, self.cfg.in_rate, self.cfg.out_rate, total, out=rows, stream=cur)
            else:
                src = tracks_stage_mix_device(torch.cat(tracks).contiguous(), table, mix, self.cfg.in_rate, self.cfg.out_rate, total, out=rows,
                                              stream=cur)
            got = 0

            def pull():
                nonlocal got
                while self.available:
                    if got >= cap:
                        raise RuntimeError("convert_tracks_device: more output than %d frames in gives" % total)
                    got += self.pull_device(out[:, got:], cap - got, stride=cap)

            step = self.isamp_max
            for pos in range(0, total, step):
                self.push_device(src[:, pos:], min(step, total - pos), stride=total)
                pull()
            self.drain()
            pull()
        finally:
            if prev is None:
                self.use_own_stream()
            else:
                self.set_stream(prev)
        need = max(int(e.out_first + e.out_frames) for e in plan.table)
        if got < need:
            raise RuntimeError("convert_tracks_device: %d output frames where the plan expects %d" % (got, need))
        return plan, table, out

    def convert_tracks_device(self, tracks, mix=None, gapless=None):
        """Whole tracks of UNEQUAL length, one per stream, device to device: convert_track_device for a ragged batch.  `tracks`
        is a list of float32 device tensors [frames_i, nch], at most `nstreams` of them (the streams left over run empty) -- or of
        integer PCM as it is stored: all int16, all int32, or all uint8 [frames_i, nch * 3] (packed 24 bit), which the stage pass
        converts on load (tracks_stage_device); mixed dtypes raise TypeError.  The handle is a float32 handle and the result is
        float32 either way.

        The tracks are planned (tracks_plan), packed end to end, staged into rows of the longest extended length -- each with the
        LPC extension at its own two ends and zeros behind it (tracks_stage_device) -- and the rows are pushed in isamp_max
        pieces, drained and pulled, which is convert_track_device's loop.  The zeros behind a shorter track are its drain, so
        every track gets, shape and bits, what convert_track_device gives it on a one-stream handle of its own.  Returns a list
        of tensors [out_frames_i, nch]: views of the handle's output rows.  Runs on torch's current stream of the tracks'
        device, copies no sample to the host and leaves the handle drained, as convert_track_device does (reset() makes it take the
        next batch).  The padding is resampled too: batch tracks of similar length (tracks_batches, convert_library_to_pcm).

        `mix` (a name of MIX_MATRICES or an array [nch, nch_src]): the tracks hold nch_src channels and are mixed down (or up) to
        the handle's nch on load, by tracks_stage_mix_device -- "these 5.1 tracks to 48 kHz stereo" reads the source once and
        resamples two channels.  A matrix whose shape does not fit the handle or the tracks raises ValueError.

        `gapless` (one group id per track; negative: a single): consecutive tracks with one non-negative id are cut from one
        master, in play order.  They are planned by album.tracks_plan_album and staged from their neighbours
        (album.tracks_stage_album_device): an inner edge holds the neighbour's frames where a single's is extrapolated, and the
        row starts on the album's output grid, so the album's results laid end to end are the album converted as ONE track --
        its length exactly, its samples to the chain's rounding -- with no click at a join ("Gapless albums").
        None is the path without it, untouched; with `mix` it raises ValueError."""
        plan, _, out = self._convert_tracks_rows(tracks, mix=mix, gapless=gapless)
        return [out[t, int(e.out_first):int(e.out_first + e.out_frames)] for t, e in zip(range(len(tracks)), plan.table)]

    def _tracks_finish_kw(self, ntracks, finish_kw, who):
        import torch
        if "gain" in finish_kw and hasattr(finish_kw["gain"], "data_ptr") and self.nstreams > ntracks:  # per-track gains: the idle streams get unity
            g = finish_kw["gain"]
            finish_kw["gain"] = torch.cat([g, g.new_ones(self.nstreams - ntracks)])
        for k in ("peak", "clipped"):
            if finish_kw.get(k) is not None:
                raise ValueError("%s is allocated by %s" % (k, who))

    def convert_tracks_to_pcm_streamed(self, tracks, dst_format, window=None, _scratch=None, shaping=None, segment=65536, **finish_kw):
        """convert_tracks_to_pcm_device in bounded memory: the same inputs, the same (views, peak, clipped), equal bit for bit, and
        no rows.  The tracks are planned, packed and the table uploaded as there; then ONE input window [nstreams, window, nch] and
        ONE output window are allocated besides the packed destination and the statistics, and on torch's current stream the rows
        are staged a window at a time (tracks_stage_window_device), pushed, and whatever the handle has available is pulled into
        the output window and finished at the running output position (tracks_finish_window_device), then drained the same way.
        Everything is on one stream, which orders the reuse of the two windows.  `window` (frames, at most isamp_max, the
        default) sets the footprint: nstreams * window frames instead of nstreams * the longest track ("Windows").

        The virtual rows are ceil(2 * in_rate / out_rate) + 1 frames longer than the plan's: how many frames a drained handle yields
        in all depends on the push pattern by a frame or two (rate_base.h:436-468), and the extra zeros -- more of every track's
        drain -- put every track's last output frame inside what comes out whatever the pattern is.

        `shaping` is accepted for symmetry with convert_tracks_to_pcm_device and refused: noise shaping needs a per-track state
        across windows, and the windowed form of it is not built.  (It is built under a name of its own,
        convert_tracks_to_pcm_streamed_shaped, which carries that state.)

        `mix=` (a keyword beside those of the output stage; default None) as in convert_tracks_device: the windows are staged by
        tracks_stage_mix_window_device.  `gapless=` (a keyword like `mix=`; default None) as in convert_tracks_device: the windows
        are staged by album.tracks_stage_album_window_device."""
        mix = finish_kw.pop("mix", None)
        gapless = finish_kw.pop("gapless", None)
        if shaping is not None:
            raise ValueError("noise shaping in the windowed form is not built: use convert_tracks_to_pcm_device")
        return self._convert_tracks_streamed(tracks, dst_format, window, _scratch, None, finish_kw, "convert_tracks_to_pcm_streamed", mix=mix,
                                             gapless=gapless)

    def convert_tracks_to_pcm_streamed_shaped(self, tracks, dst_format, shaping, segment=65536, window=None, **finish_kw):
        """convert_tracks_to_pcm_device(..., shaping=, segment=) in bounded memory: convert_tracks_to_pcm_streamed with noise-shaped
        dither.  The loop is that method's; every pulled window is finished by tracks_finish_shaped_window_device at the running
        output position -- the pulls are ascending and contiguous from frame 0, the order that call needs -- and the error history of
        every (track, channel) is handed from window to window through two state tensors [nstreams, nch, 16] (float64), allocated
        besides the two windows.  `shaping` (a name of NOISE_SHAPES or coefficients) and `segment` are finish_shaped_device's; dither
        is on by default, `dst_format` is never None and `out=False` measures only.  Returns (views, peak, clipped), equal bit for bit
        to convert_tracks_to_pcm_device(tracks, dst_format, shaping=shaping, segment=segment, ...) whatever `window` is.

        A track's segments that fall into different windows no longer run side by side, so this form costs about (number of output
        windows) * min(segment, output window) frames of the serial chain where the whole-row form costs `segment` (DESIGN.md 11,
        "Windows with noise shaping").  The name is new because convert_tracks_to_pcm_streamed(..., shaping=) is pinned as a refusal."""
        _shaping(shaping, segment)  # (refused before anything is planned)
        scratch = finish_kw.pop("_scratch", None)
        return self._convert_tracks_streamed(tracks, dst_format, window, scratch, (shaping, segment), finish_kw, "convert_tracks_to_pcm_streamed_shaped")

    def _convert_tracks_streamed(self, tracks, dst_format, window, _scratch, shaped, finish_kw, who, measure=None, limit=None, mix=None,
                                 gapless=None):
        """the loop of convert_tracks_to_pcm_streamed (shaped None) and convert_tracks_to_pcm_streamed_shaped (shaped = (shaping,
        segment)): stage a window, push it, pull whatever is available into the output window and finish it at the running output
        position, then drain the same way.  The shaped form finishes with tracks_finish_shaped_window_device and ping-pongs two
        state tensors.  `measure` (the measuring pass of the normalising forms): called once as measure(plan, table, cap, longest
        output window, device, stream), it gives a callable (_WindowMeter) that is called as (wout, first, frames) for every pulled
        window instead of the output stage; nothing is written then, and the return is what that callable's `result()` gives.
        `limit` (the limited form): called once as limit(table, cap, output window, stream), it gives a _WindowLimiter, which sits
        between the pull and the stage behind it -- that stage then sees the limited windows the limiter emits, ascending and
        contiguous from frame 0 like the pulled ones, and the rest of them after the final pull.  `mix`: the windows are staged by
        tracks_stage_mix_window_device; `gapless`: by album.tracks_stage_album_window_device, on the album plan."""
        import torch
        mix = self._tracks_mix(mix)
        tracks, plan = self._tracks_checked(tracks, mix, gapless)
        n, dev = len(tracks), tracks[0].device
        step = self.isamp_max
        window = step if window is None else int(window)
        if not 1 <= window <= step:
            raise ValueError("window must be 1 to isamp_max = %d frames, not %d" % (step, window))
        self._tracks_finish_kw(n, finish_kw, who)
        if finish_kw.get("stream") is not None:
            raise ValueError("%s runs on torch's current stream" % who)
        in_rate, out_rate = self.cfg.in_rate, self.cfg.out_rate
        cur = torch.cuda.current_stream(dev)
        finish_kw["stream"] = cur
        table = plan.to_device(dev)
        total = plan.row_frames + -(-2 * in_rate // out_rate) + 1 if plan.row_frames else 0
        cap = total * out_rate // in_rate + 2                 # (as out_row_cap: drain leaves round(total * out_rate / in_rate) frames in all)
        win_out = -(-window * out_rate // in_rate)            # about what one push makes available; the loop takes any size
        if _scratch is not None:  # (convert_library_to_pcm: the two windows of the first batch serve every batch)
            win = _scratch.take("win", (self.nstreams, min(window, max(total, 1)), self.nch), dev)
            wout = _scratch.take("wout", (self.nstreams, min(win_out, cap), self.nch), dev)
        else:
            win = torch.empty((self.nstreams, min(window, max(total, 1)), self.nch), dtype=torch.float32, device=dev)
            wout = torch.empty((self.nstreams, min(win_out, cap), self.nch), dtype=torch.float32, device=dev)
        # nothing to finish yet: allocates (and checks) the destination and the statistics
        if measure is not None:
            measure = measure(plan, table, cap, wout.shape[1], dev, cur)
        elif shaped is None:
            pcm, peak, clipped = tracks_finish_window_device(wout, table, cap, 0, 0, dst_format, plan.dst_total, **finish_kw)
            finish_kw.update(out=pcm, peak=peak, clipped=clipped)
        else:
            pcm, peak, clipped = tracks_finish_shaped_window_device(wout, table, cap, 0, 0, dst_format, plan.dst_total, *shaped, **finish_kw)[:3]
            finish_kw.update(out=False if pcm is None else pcm, peak=peak, clipped=clipped)
            # the history of every (track, channel): read from one tensor and written to the other, window after window
            states = [torch.zeros((self.nstreams, self.nch, RRX_SHAPE_MAX_ORDER), dtype=torch.float64, device=dev) for _ in range(2)]

            def shaped_window(buf, first, frames):
                kw = dict({"gain": None, "dither": True, "seed": 0}, **finish_kw)
                _tracks_finish_shaped_window(buf, table, cap, first, frames, dst_format, plan.dst_total, shaped[0], shaped[1], kw["gain"],
                                             kw["dither"], kw["seed"], states[0], states[1], kw["out"], kw["peak"], kw["clipped"], kw["stream"])
        if finish_kw.get("gain") is not None and not hasattr(finish_kw["gain"], "data_ptr"):
            finish_kw["gain"] = torch.full((self.nstreams,), float(finish_kw["gain"]), dtype=torch.float64, device=dev)  # (once, not per window)
        if limit is not None:
            limit = limit(table, cap, wout, cur)

        def stage(buf, first, k):  # what follows the pull: frames [first, first + k) of the rows, in `buf`
            if measure is not None:
                if k:
                    measure(buf, first, k)
            elif shaped is None:
                tracks_finish_window_device(buf, table, cap, first, k, dst_format, plan.dst_total, **finish_kw)
            elif k:  # (an empty window touches nothing, the state included: the two tensors keep their roles)
                shaped_window(buf, first, k)
                states.reverse()

        got = 0
        if total:
            packed, links = self._tracks_staged(tracks, plan, dev)
            if gapless is not None:
                from . import album
            prev = self._stream
            self.set_stream(cur.cuda_stream)
            try:
                def pull():
                    nonlocal got
                    while self.available:
                        if got >= cap:
                            raise RuntimeError("%s: more output than %d frames in gives" % (who, total))
                        k = self.pull_device(wout, min(wout.shape[1], cap - got), stride=wout.shape[1])
                        if limit is None:
                            stage(wout, got, k)
                        elif k:
                            emitted = limit.feed(wout, k)
                            if emitted is not None:
                                stage(*emitted)
                        got += k

                for pos in range(0, total, window):
                    k = min(window, total - pos)
                    if gapless is not None:
                        album.tracks_stage_album_window_device(packed, table, links, in_rate, out_rate, total, pos, k, out=win, stream=cur)
                    elif mix is None:
                        tracks_stage_window_device(packed, table, in_rate, out_rate, total, pos, k, out=win, stream=cur)
                    else:
                        tracks_stage_mix_window_device(packed, table, mix, in_rate, out_rate, total, pos, k, out=win, stream=cur)
                    self.push_device(win, k, stride=win.shape[1])
                    pull()
                self.drain()
                pull()
            finally:
                if prev is None:
                    self.use_own_stream()
                else:
                    self.set_stream(prev)
        need = max(int(e.out_first + e.out_frames) for e in plan.table)
        if got < need:
            raise RuntimeError("%s: %d output frames where the plan expects %d" % (who, got, need))
        if limit is not None:  # (every slice ends inside the `got` frames: rows of that length hold the same slices)
            for emitted in limit.flush(got):
                stage(*emitted)
        if measure is not None:
            return measure.result()
        return _tracks_views(pcm, plan, n), peak[:n], clipped[:n]

    def convert_tracks_to_pcm_device(self, tracks, dst_format, _scratch=None, shaping=None, segment=65536, mix=None, gapless=None, **finish_kw):
        """convert_tracks_device followed by the ragged output stage, tracks_finish_device(..., dst_format, **finish_kw), into ONE
        packed buffer, on torch's current stream: whole tracks of unequal length in, integer PCM out.  The tracks may be integer PCM
        themselves (int16, int32, or uint8 packed 24 bit, as in convert_tracks_device): PCM in, PCM out, with float32 only in the
        rows the handle is pushed from.  Returns (list of per-track
        views of that buffer, peak [ntracks, nch], clipped [ntracks, nch]); the buffer itself is the `_base` of the views.
        With `shaping` (a name of NOISE_SHAPES or coefficients) the output stage is tracks_finish_shaped_device(..., shaping,
        segment, **finish_kw): noise-shaped dither, on by default there, in segments counted from each track's first frame.
        `mix` and `gapless` as in convert_tracks_device."""
        import torch
        tracks = list(tracks)
        plan, table, out = self._convert_tracks_rows(tracks, _scratch, mix=mix, gapless=gapless)
        n = len(tracks)
        self._tracks_finish_kw(n, finish_kw, "convert_tracks_to_pcm_device")
        finish_kw.setdefault("stream", torch.cuda.current_stream(out.device))
        return _finish_rows(out, table, plan, n, dst_format, shaping, segment, finish_kw)

    def convert_tracks_to_pcm_normalized(self, tracks, dst_format, target_dbtp=-1.0, shaping=None, segment=65536, dither=False, seed=0):
        """convert_tracks_to_pcm_device with every track normalised to a TRUE peak of `target_dbtp` dBTP: the rows are converted
        once (as in convert_tracks_device), measured with tracks_true_peak_device (the "bs1770" filter), and per track
        m = max over its channels of max(true peak, sample peak) gives the gain 10 ** (target_dbtp / 20) / m -- or 1.0 where m is 0
        or not finite (a silent track stays silent) -- computed on the device, without a host synchronisation; then the rows are
        finished under that gain with tracks_finish_device, or tracks_finish_shaped_device when `shaping` is given (`segment` as
        there).  Returns (list of per-track views of the packed PCM, peak [ntracks, nch], clipped [ntracks, nch], gain [ntracks],
        true_peak [ntracks, nch]); `peak` is the sample peak AFTER the gain, as the output stage reports it, `true_peak` the
        measured one BEFORE it.  Dither and shaping add their noise after the gain, so near 0 dBTP `clipped` can be nonzero with
        them; without them, at the default target, it is zero."""
        import torch
        tracks = list(tracks)
        plan, table, out = self._convert_tracks_rows(tracks)
        n = len(tracks)
        cur = torch.cuda.current_stream(out.device)
        true_peak, sample_peak = tracks_true_peak_device(out, table, stream=cur)
        gain = _peak_normalizing_gain(true_peak, sample_peak, 10.0 ** (float(target_dbtp) / 20.0))
        views, peak, clipped = _finish_rows(out, table, plan, n, dst_format, shaping, segment, dict(gain=gain, dither=dither, seed=seed, stream=cur))
        return views, peak, clipped, gain[:n], true_peak[:n]

    def convert_tracks_to_pcm_loudness_normalized(self, tracks, dst_format, target_lufs=-18.0, max_dbtp=-1.0, weights=None, shaping=None,
                                                  segment=65536, dither=False, seed=0, album=None):
        """convert_tracks_to_pcm_device with every track normalised to an integrated LOUDNESS of `target_lufs` LUFS, held under a
        true peak of `max_dbtp` dBTP (ReplayGain 2.0, EBU R 128): the rows are converted once, measured with
        tracks_loudness_device + loudness_gate_device (K-weighting of the output rate, hops of out_rate // 10 frames, the gates of
        BS.1770, channel `weights` as there) and with tracks_true_peak_device, and per track, with L its loudness and m as in
        convert_tracks_to_pcm_normalized, the gain is min(10 ** ((target_lufs - L) / 20), 10 ** (max_dbtp / 20) / m) -- or 1.0 where
        no block passed the gates (a silent or very short track) or m is 0 or not finite -- computed on the device, without a host
        synchronisation; then the rows are finished under that gain as in convert_tracks_to_pcm_normalized.  Returns what that
        call returns, plus the loudness: (views, peak, clipped, gain [ntracks], true_peak [ntracks, nch], lufs [ntracks]); `lufs`
        is the measured loudness BEFORE the gain, -inf where no block passed.

        `album` (None, or one non-negative int per track): the tracks of one album get ONE gain, which keeps the level differences
        the album was mastered with (the album gain of ReplayGain 2.0).  L is then the album's loudness -- the gate over the pooled
        400 ms blocks of its tracks, loudness_blocks_device + loudness_gate_groups_device -- and m the largest peak over its
        tracks; the formula above is applied per album and gathered per track on the device.  The tuple keeps its six entries,
        and `lufs[t]` is the loudness of t's album."""
        import torch
        tracks = list(tracks)
        album = _album_checked(album, len(tracks))
        plan, table, out = self._convert_tracks_rows(tracks)
        n = len(tracks)
        cur = torch.cuda.current_stream(out.device)
        rate = int(self.cfg.out_rate)
        energy, hops = tracks_loudness_device(out, table, rate, stream=cur)
        lufs, n2, of = _loudness_measured(energy, hops, n, album, weights, rate, cur)
        true_peak, sample_peak = tracks_true_peak_device(out, table, stream=cur)
        gain, lufs = _loudness_normalized_gain(lufs, n2, of, _largest_peak(true_peak, sample_peak), n, target_lufs, max_dbtp)
        views, peak, clipped = _finish_rows(out, table, plan, n, dst_format, shaping, segment, dict(gain=gain, dither=dither, seed=seed, stream=cur))
        return views, peak, clipped, gain[:n], true_peak[:n], lufs[:n]

    def _gain_by_loudness(self, energy, hops, n, album, weights, target_lufs, cur):
        """(gain, lufs), both [rows], of the limited conversions from the hop energies of the rows: 10 ** ((target_lufs - L) / 20), 1.0
        where no block passed the gates; with `album` L is the loudness of the track's album"""
        import torch
        lufs, n2, of = _loudness_measured(energy, hops, n, album, weights, int(self.cfg.out_rate), cur)
        passed = n2 > 0
        if of is not None:  # per album so far: gathered per track, the rows without a track at -inf and not passed
            rows, dev = energy.shape[0], energy.device
            album_lufs, album_passed = lufs, passed
            lufs = torch.full((rows,), float("-inf"), dtype=album_lufs.dtype, device=dev)
            lufs[:n] = album_lufs[of]
            passed = torch.zeros((rows,), dtype=torch.bool, device=dev)
            passed[:n] = album_passed[of]
        by_loudness = torch.pow(10.0, (float(target_lufs) - torch.where(passed, lufs, torch.zeros_like(lufs))) / 20.0)
        gain = torch.where(passed, by_loudness, torch.ones_like(by_loudness)).contiguous()
        return gain, lufs

    def convert_tracks_to_pcm_loudness_limited(self, tracks, dst_format, target_lufs=-14.0, max_dbtp=-1.0, lookahead_ms=1.5, hold_ms=10.0,
                                               weights=None, shaping=None, segment=65536, dither=False, seed=0, album=None, release_ms=None,
                                               release_block=1024):
        """convert_tracks_to_pcm_loudness_normalized with a true-peak LIMITER in place of the peak-bound gain: a track with a few
        loud transients over a quiet bed reaches `target_lufs` where the static gain min(by loudness, by peak) would leave it far
        below.  The rows are converted once and their loudness measured as there (`weights`, `album` as there); the gain is
        10 ** ((target_lufs - L) / 20) ALONE, 1.0 where no block passed the gates.  Then tracks_limit_device limits the rows in
        place under that gain at the ceiling 10 ** (max_dbtp / 20), with `lookahead_ms` and `hold_ms` rounded to frames of the
        output rate and clamped to 1..RRX_LIMIT_MAX_LOOKAHEAD and 0..RRX_LIMIT_MAX_HOLD; tracks_true_peak_device measures the
        limited rows, and trim = min(1, ceiling / max(true peak, sample peak)) -- 1.0 where that maximum is 0 or not finite --
        removes what the limiter leaves over the ceiling between the samples; the rows are finished under `trim` as in
        convert_tracks_to_pcm_normalized.  Everything is computed on the device, without a host synchronisation.  Returns (views,
        peak, clipped, gain [ntracks], trim [ntracks], reduction [ntracks], limited [ntracks], lufs [ntracks]): `reduction` the
        limiter's smallest gain, `limited` the frames it lowered, `lufs` the loudness BEFORE the gain (of t's album with `album`).
        With `release_ms` the limiter is tracks_limit_release_device under limit_release_coef(release_ms, out_rate) in blocks of
        `release_block` entries: the gain recovers exponentially behind a transient; None is the limiter without a release."""
        import torch
        tracks = list(tracks)
        album = _album_checked(album, len(tracks))
        rate = int(self.cfg.out_rate)
        ceiling, lookahead, hold = _limiter_frames(rate, max_dbtp, lookahead_ms, hold_ms)
        plan, table, out = self._convert_tracks_rows(tracks)
        n = len(tracks)
        cur = torch.cuda.current_stream(out.device)
        energy, hops = tracks_loudness_device(out, table, rate, stream=cur)
        gain, lufs = self._gain_by_loudness(energy, hops, n, album, weights, target_lufs, cur)
        if release_ms is None:
            _, reduction, limited = tracks_limit_device(out, table, ceiling, gain=gain, lookahead=lookahead, hold=hold, stream=cur)
        else:
            _, reduction, limited = tracks_limit_release_device(out, table, ceiling, limit_release_coef(release_ms, rate), gain=gain,
                                                                lookahead=lookahead, hold=hold, block=release_block, stream=cur)
        true_peak, sample_peak = tracks_true_peak_device(out, table, stream=cur)
        trim = _trim(true_peak, sample_peak, ceiling)
        views, peak, clipped = _finish_rows(out, table, plan, n, dst_format, shaping, segment, dict(gain=trim, dither=dither, seed=seed, stream=cur))
        return views, peak, clipped, gain[:n], trim[:n], reduction[:n], limited[:n], lufs[:n]

    def _streamed_under_gain(self, tracks, dst_format, window, shaping, segment, gain, dither, seed, who):
        """pass B of the streamed normalising forms: reset(), then the streamed loop, shaped or not, under the per-track gain"""
        if shaping is not None:
            _shaping(shaping, segment)
        self.reset()
        kw = dict(gain=gain[:len(tracks)].contiguous(), dither=dither, seed=seed)
        return self._convert_tracks_streamed(tracks, dst_format, window, None, None if shaping is None else (shaping, segment), kw, who)

    def convert_tracks_to_pcm_streamed_normalized(self, tracks, dst_format, target_dbtp=-1.0, window=None, shaping=None, segment=65536,
                                                  dither=False, seed=0):
        """convert_tracks_to_pcm_normalized in bounded memory: the same inputs, the same (views, peak, clipped, gain, true_peak), equal
        bit for bit whatever `window` is, and no rows.  Two passes over the same windows.  Pass A is convert_tracks_to_pcm_streamed's
        loop with tracks_true_peak_window_device on every pulled window in place of the output stage -- the pulls are ascending and
        contiguous from frame 0, the order that call needs; nothing is written.  The gain is derived on the device by
        convert_tracks_to_pcm_normalized's own expressions, without a host synchronisation; the handle is reset(); pass B is the
        streamed conversion, shaped (convert_tracks_to_pcm_streamed_shaped) or not, under that gain.  The tracks are resampled twice:
        that is the price of never holding the rows ("Windows with true peak and loudness").  Memory: that of the
        streamed form plus the two filter states [nstreams, nch, 16] and the statistics."""
        import functools
        tracks = list(tracks)
        if shaping is not None:
            _shaping(shaping, segment)  # (refused before anything is converted)
        who = "convert_tracks_to_pcm_streamed_normalized"
        true_peak, sample_peak, _, _ = self._convert_tracks_streamed(tracks, dst_format, window, None, None, {}, who,
                                                                     measure=functools.partial(_WindowMeter, None, self.nch))
        n = len(tracks)
        gain = _peak_normalizing_gain(true_peak, sample_peak, 10.0 ** (float(target_dbtp) / 20.0))
        views, peak, clipped = self._streamed_under_gain(tracks, dst_format, window, shaping, segment, gain, dither, seed, who)
        return views, peak, clipped, gain[:n], true_peak[:n]

    def convert_tracks_to_pcm_streamed_loudness_normalized(self, tracks, dst_format, target_lufs=-18.0, max_dbtp=-1.0, weights=None,
                                                           window=None, shaping=None, segment=65536, dither=False, seed=0, album=None):
        """convert_tracks_to_pcm_loudness_normalized in bounded memory: the same inputs, `album` included, the same (views, peak,
        clipped, gain, true_peak, lufs), equal bit for bit whatever `window` is, and no rows.  Two passes as in
        convert_tracks_to_pcm_streamed_normalized: pass A measures every pulled window with tracks_true_peak_window_device and
        tracks_loudness_window_device (K-weighting of the output rate, hops of out_rate // 10 frames counted from every track's own
        first output frame, so a window cuts them anywhere); the gain comes from convert_tracks_to_pcm_loudness_normalized's own
        expressions over the hop energies, on the device; pass B converts again under it.  Memory: that of the streamed form plus
        the states (two of [nstreams, nch, 16] per measurement), one window's work buffer and nstreams * nch *
        ceil(longest output row / hop) doubles of hop energies -- a ten-thousandth of the audio."""
        import functools
        import torch
        tracks = list(tracks)
        album = _album_checked(album, len(tracks))
        if shaping is not None:
            _shaping(shaping, segment)  # (refused before anything is converted)
        who = "convert_tracks_to_pcm_streamed_loudness_normalized"
        rate = int(self.cfg.out_rate)
        true_peak, sample_peak, energy, hops = self._convert_tracks_streamed(tracks, dst_format, window, None, None, {}, who,
                                                                             measure=functools.partial(_WindowMeter, rate, self.nch))
        n = len(tracks)
        lufs, n2, of = _loudness_measured(energy, hops, n, album, weights, rate, torch.cuda.current_stream(energy.device))
        gain, lufs = _loudness_normalized_gain(lufs, n2, of, _largest_peak(true_peak, sample_peak), n, target_lufs, max_dbtp)
        del energy, hops, n2, sample_peak  # (pass B runs in the streamed form's memory, beside what is returned)
        views, peak, clipped = self._streamed_under_gain(tracks, dst_format, window, shaping, segment, gain.contiguous(), dither, seed, who)
        return views, peak, clipped, gain[:n], true_peak[:n], lufs[:n]

    def convert_tracks_to_pcm_streamed_loudness_limited(self, tracks, dst_format, target_lufs=-14.0, max_dbtp=-1.0, lookahead_ms=1.5,
                                                        hold_ms=10.0, weights=None, window=None, shaping=None, segment=65536, dither=False,
                                                        seed=0, album=None, release_ms=None, release_block=1024):
        """convert_tracks_to_pcm_loudness_limited in bounded memory: the same inputs, the same (views, peak, clipped, gain, trim,
        reduction, limited, lufs), equal bit for bit whatever `window` is, and no rows.  Three passes over the same windows, with
        reset() between them.  Pass A measures the hop energies of every pulled window (tracks_loudness_window_device); the gain
        comes from convert_tracks_to_pcm_loudness_limited's own expressions, on the device.  Pass B converts again and limits under
        that gain by windows: the limiter has nothing recursive in it, so it needs no state, only a halo -- a carry buffer per row
        keeps the frames within reach of what is not emitted yet, and tracks_limit_window_device emits every frame once its
        look-ahead has been pulled; the limited windows are measured with tracks_true_peak_window_device, which gives `trim`,
        and the limiter's own statistics `reduction` and `limited`.  Pass C converts and limits once more, statistics into scratch,
        and finishes the limited windows, shaped or not, under `trim`.  The tracks are resampled three times and limited twice:
        that is the price of never holding the rows ("Windows with the limiter").  Memory: that of the streamed
        form, plus per row two carry buffers of back + ahead + one output window frames and one limited window, the hop
        energies and the states of the measuring passes.
        With `release_ms` the limiter has convert_tracks_to_pcm_loudness_limited's release, limit_release_coef(release_ms, out_rate)
        in blocks of `release_block` entries, by windows: tracks_limit_release_window_device carries the scan's state per track from
        one emitted window into the next, passes B and C each from a fresh state (two [nstreams, 8] buffers); the returns stay
        equal to the whole-row method's bit for bit.  None is the limiter without a release."""
        import functools
        import torch
        tracks = list(tracks)
        album = _album_checked(album, len(tracks))
        if shaping is not None:
            _shaping(shaping, segment)  # (refused before anything is converted)
        who = "convert_tracks_to_pcm_streamed_loudness_limited"
        rate = int(self.cfg.out_rate)
        ceiling, lookahead, hold = _limiter_frames(rate, max_dbtp, lookahead_ms, hold_ms)
        release = None if release_ms is None else _limit_release_params(limit_release_coef(release_ms, rate), release_block)
        n = len(tracks)
        # pass A: the loudness
        _, _, energy, hops = self._convert_tracks_streamed(tracks, dst_format, window, None, None, {}, who,
                                                           measure=functools.partial(_WindowMeter, rate, self.nch))
        dev = energy.device
        cur = torch.cuda.current_stream(dev)
        gain, lufs = self._gain_by_loudness(energy, hops, n, album, weights, target_lufs, cur)
        del energy, hops
        # pass B: what the limiter leaves over the ceiling, and its statistics
        rows = gain.shape[0]
        reduction = torch.ones((rows,), dtype=torch.float64, device=dev)
        limited = torch.zeros((rows,), dtype=torch.int64, device=dev)
        self.reset()
        true_peak, sample_peak, _, _ = self._convert_tracks_streamed(
            tracks, dst_format, window, None, None, {}, who, measure=functools.partial(_WindowMeter, None, self.nch),
            limit=functools.partial(_WindowLimiter, ceiling, gain, lookahead, hold, reduction, limited, release=release))
        trim = _trim(true_peak, sample_peak, ceiling)
        del true_peak, sample_peak
        # pass C: the same limited windows, finished under the trim
        self.reset()
        kw = dict(gain=trim[:n].contiguous(), dither=dither, seed=seed)
        views, peak, clipped = self._convert_tracks_streamed(
            tracks, dst_format, window, None, None if shaping is None else (shaping, segment), kw, who,
            limit=functools.partial(_WindowLimiter, ceiling, gain, lookahead, hold, torch.ones_like(reduction), torch.zeros_like(limited),
                                    release=release))
        return views, peak, clipped, gain[:n], trim[:n], reduction[:n], limited[:n], lufs[:n]

    def convert_library_to_pcm(self, tracks, dst_format, window=None, gain=None, dither=False, seed=0, shaping=None, segment=65536, mix=None,
                               gapless=None):
        """A whole library on this ONE handle: any number of tracks of unequal length (tensors as in convert_tracks_device), cut
        into the length-sorted batches of tracks_batches for the handle's own `nstreams` -- no other split resamples less padding
        -- and converted batch after batch, with reset() before every batch whenever the handle has been used.  Each batch runs
        through convert_tracks_to_pcm_device, or with `window` (frames) through convert_tracks_to_pcm_streamed in bounded memory.
        No handle is opened, and the row and window buffers are taken once, at the first and longest batch's size, and reused as
        views by the later batches.

        `gain`: None, a float, or one value per track in the caller's order (a sequence, or a float64 device tensor [ntracks]).
        Dither: the track of sorted rank r is stream r of the library as ONE ragged batch -- batch b is finished with
        seed + b * nstreams * nch * 0xBF58476D1CE4E5B9 (mod 2^64), which puts that track on dither channel r * nch + ch -- so its
        bytes and statistics are those of a one-stream finish_device on its slice with seed + r * nch * 0xBF58476D1CE4E5B9,
        whatever `nstreams` is.  Returns (per-track PCM tensors in the caller's order, peak [ntracks, nch], clipped [ntracks, nch]).
        Runs on torch's current stream and copies no sample to the host.

        `shaping` (a name of NOISE_SHAPES or coefficients) and `segment`: every batch is finished by tracks_finish_shaped_device
        with the same per-batch seed, so the rule above holds with finish_shaped_device for finish_device; `dither` keeps its
        default here.  With `window` it raises ValueError: the windowed form of noise shaping is not built (under this name:
        convert_library_to_pcm_streamed_shaped is that form).

        `mix` as in convert_tracks_device: every batch is staged with it.

        `gapless` (one group id per track of the library, as in convert_tracks_device; `tracks` is then in play order): the
        library is packed and planned ONCE, in the order given (album.tracks_plan_album), and every length-sorted batch takes its
        tracks' entries of that one plan.  An entry points into the library's packed source and destination, so the tracks of an
        album may land in different batches and are still staged from their neighbours, and all batches write ONE packed
        destination, in which an album lies contiguous and in order: the views of its tracks are adjacent slices of that buffer.
        With `mix` it raises ValueError."""
        if shaping is not None and window is not None:
            raise ValueError("noise shaping in the windowed form is not built: leave `window` out")
        if gapless is not None and mix is not None:
            raise ValueError("gapless= together with mix= is not built")
        kw = {} if shaping is None else {"shaping": shaping, "segment": segment}
        if mix is not None:
            kw["mix"] = self._tracks_mix(mix)
        if window is None:
            return self._convert_library(tracks, dst_format, gain, dither, seed,
                                         lambda batch, bkw: self.convert_tracks_to_pcm_device(batch, dst_format, **kw, **bkw), gapless=gapless)
        return self._convert_library(tracks, dst_format, gain, dither, seed,
                                     lambda batch, bkw: self.convert_tracks_to_pcm_streamed(batch, dst_format, window=window, **kw, **bkw),
                                     gapless=gapless)

    def convert_library_to_pcm_streamed_shaped(self, tracks, dst_format, window, shaping, segment=65536, gain=None, dither=True, seed=0):
        """convert_library_to_pcm(..., shaping=, segment=) in bounded memory: the library rule of that method -- length-sorted
        batches, reset() between them, the per-batch seed shift, the window buffers taken once -- with every batch run through
        convert_tracks_to_pcm_streamed_shaped(batch, dst_format, shaping, segment, window=window).  A track's bytes and statistics
        are those convert_library_to_pcm(..., shaping=, segment=) gives it without a window: they depend neither on `nstreams` nor
        on `window` (None: isamp_max).  `dst_format` is never None.  The name is new for the reason given there."""
        _shaping(shaping, segment)
        return self._convert_library(tracks, dst_format, gain, dither, seed,
                                     lambda batch, bkw: self.convert_tracks_to_pcm_streamed_shaped(batch, dst_format, shaping, segment, window=window, **bkw))

    def _convert_library(self, tracks, dst_format, gain, dither, seed, convert, gapless=None):
        """the library rule of convert_library_to_pcm: `convert(batch, kw)` is one batch's conversion, kw its dither, seed, scratch
        and gains -- and with `gapless` its plan, a subset of the library's one album plan, and the one packed destination"""
        import torch
        tracks = list(tracks)
        n, S = len(tracks), self.nstreams
        if n < 1:
            raise ValueError("a library needs at least one track")
        for x in tracks:
            if not hasattr(x, "data_ptr") or x.dim() != 2:
                raise ValueError("expected [frames, nch] device tensors")
        seed = int(seed)
        if not 0 <= seed < 1 << 64:
            raise ValueError("seed must fit 64 unsigned bits")
        dev = tracks[0].device
        if gain is not None:
            if hasattr(gain, "data_ptr"):
                if gain.dtype != torch.float64 or tuple(gain.shape) != (n,) or gain.device != dev:
                    raise TypeError("gain must be a float, %d floats, or a float64 tensor [%d] on %s" % (n, n, dev))
            else:
                vals = [float(gain)] * n if not hasattr(gain, "__len__") else [float(g) for g in gain]
                if len(vals) != n:
                    raise ValueError("%d gains for %d tracks" % (len(vals), n))
                gain = torch.tensor(vals, dtype=torch.float64, device=dev)
        lib_batches = _tracks_batches(self.cfg, [x.shape[0] for x in tracks], S)
        if gapless is not None:
            from . import album
            if dst_format not in (None, RRX_FMT_S16, RRX_FMT_S24_3, RRX_FMT_S32):
                raise ValueError("unknown dst_format %r (RRX_FMT_S16, RRX_FMT_S24_3, RRX_FMT_S32 or None)" % (dst_format,))
            whole = album._tracks_plan_album(self.cfg, [x.shape[0] for x in tracks], gapless)
            packed = torch.cat(tracks).contiguous()
            pcm = None if dst_format is None else _pcm_out(None, dst_format, (whole.dst_total,), self.nch, dev)
        peak = torch.zeros((n, self.nch), dtype=torch.float64, device=dev)
        clipped = torch.zeros((n, self.nch), dtype=torch.int64, device=dev)
        views = [None] * n
        scratch = _Scratch()
        for b, idx in enumerate(lib_batches.batches):
            if self._used:
                self.reset()
            kw = {"dither": dither, "seed": (seed + b * S * self.nch * 0xBF58476D1CE4E5B9) % (1 << 64), "_scratch": scratch}
            where = torch.tensor(idx, dtype=torch.int64, device=dev)
            if gain is not None:
                kw["gain"] = gain[where].contiguous()
            batch = [tracks[i] for i in idx]
            if gapless is not None:
                kw["gapless"] = whole.subset(idx, pad=S - len(idx))
                kw["gapless"].packed = packed
                if pcm is not None:
                    kw["out"] = pcm
            v, p, c = convert(batch, kw)
            peak[where] = p
            clipped[where] = c
            if v is not None:
                for i, vi in zip(idx, v):
                    views[i] = vi
        return (None if dst_format is None else views), peak, clipped
