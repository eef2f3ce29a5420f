"""foo_dsp_resampler_amd -- Python binding of the MI355X SoX-rate engine.

The product is the C-ABI shared library `libratelib_amd.so` (include/ratelib.h, include/ratelib_amd.h, include/ratelib_amd_album.h)
whose entry points are what the reference plugin binds (rate/ratelib.h:72-81).  This package is a thin
ctypes mirror of that interface used by the tests and bench.py; it contains no signal processing and
no CPU fallback: if the library (or a GPU) is missing, calls fail.
"""
from .ratelib import (RRConfig, RRError, Resampler, available_symbols, describe_dispatch, describe_plan, edge_geometry, lib, lib_path,  # noqa: F401
                      lpc_extrapolate_device, finish_device, plan_table, RRXTrack, TracksPlan, track_geometry, tracks_plan,
                      tracks_stage_device, tracks_finish_device, tracks_stage_window_device, tracks_finish_window_device,
                      TracksBatches, tracks_batches, plan_cache_clear, plan_cache_stats, RR_BEST, RR_NORM, RRX_FMT_FLOAT, RRX_FMT_DOUBLE, RRX_FMT_S16, RRX_FMT_S32, RRX_FMT_S24_3, EXPECTED_SYMBOLS,
                      finish_shaped_device, tracks_finish_shaped_device, tracks_finish_shaped_window_device, NOISE_SHAPES, RRX_SHAPE_MAX_ORDER,
                      true_peak_device, tracks_true_peak_device, TRUE_PEAK_FILTERS, RRX_TP_MAX_PHASES, RRX_TP_MAX_TAPS,
                      k_weighting, K_WEIGHTING_48K, loudness_device, tracks_loudness_device, loudness_gate, loudness_gate_device, integrated_lufs,
                      loudness_normalizing_gain, loudness_blocks_device, loudness_gate_groups_device, loudness_range_device, loudness_range_lu,
                      loudness_meter_device, tracks_true_peak_window_device, tracks_loudness_window_device, RRX_LOUDNESS_WIN_STATE,
                      limit_device, tracks_limit_device, limit_work_doubles, RRX_LIMIT_MAX_LOOKAHEAD, RRX_LIMIT_MAX_HOLD,
                      limit_release_coef, limit_release_work_doubles, limit_release_device, tracks_limit_release_device,
                      RRX_LIMIT_RELEASE_MIN_BLOCK, RRX_LIMIT_RELEASE_MAX_BLOCK,
                      limit_window_reach, tracks_limit_window_work_doubles, tracks_limit_window_device,
                      tracks_limit_release_window_work_doubles, tracks_limit_release_window_device, RRX_LIMIT_RELEASE_WIN_STATE,
                      PackedPlan, PackedTable, packed_plan, tracks_true_peak_packed_device, tracks_loudness_packed_device, scan_tracks_pcm,
                      MIX_MATRICES, RRX_MIX_MAX_CH, mix_matrix, mix_device, tracks_stage_mix_device, tracks_stage_mix_window_device)
from .album import (ALBUM_SYMBOLS, RRX_LINK_NONE, RRXTrackLink, TracksAlbumPlan, tracks_plan_album, tracks_stage_album_device,  # noqa: F401
                    tracks_stage_album_window_device)

__all__ = ["RRConfig", "RRError", "Resampler", "describe_plan", "describe_dispatch", "plan_table", "edge_geometry", "lpc_extrapolate_device", "finish_device", "lib",
           "RRXTrack", "TracksPlan", "track_geometry", "tracks_plan", "tracks_stage_device", "tracks_finish_device", "tracks_stage_window_device", "tracks_finish_window_device",
           "TracksBatches", "tracks_batches", "plan_cache_clear", "plan_cache_stats",
           "lib_path",
           "available_symbols", "RR_BEST", "RR_NORM", "RRX_FMT_FLOAT", "RRX_FMT_DOUBLE", "RRX_FMT_S16", "RRX_FMT_S32", "RRX_FMT_S24_3",
           "EXPECTED_SYMBOLS", "finish_shaped_device", "tracks_finish_shaped_device", "tracks_finish_shaped_window_device", "NOISE_SHAPES", "RRX_SHAPE_MAX_ORDER",
           "true_peak_device", "tracks_true_peak_device", "TRUE_PEAK_FILTERS", "RRX_TP_MAX_PHASES", "RRX_TP_MAX_TAPS",
           "k_weighting", "K_WEIGHTING_48K", "loudness_device", "tracks_loudness_device", "loudness_gate", "loudness_gate_device", "integrated_lufs",
           "loudness_normalizing_gain", "loudness_blocks_device", "loudness_gate_groups_device", "loudness_range_device", "loudness_range_lu",
           "loudness_meter_device", "tracks_true_peak_window_device", "tracks_loudness_window_device", "RRX_LOUDNESS_WIN_STATE",
           "limit_device", "tracks_limit_device", "limit_work_doubles", "RRX_LIMIT_MAX_LOOKAHEAD", "RRX_LIMIT_MAX_HOLD",
           "limit_release_coef", "limit_release_work_doubles", "limit_release_device", "tracks_limit_release_device",
           "RRX_LIMIT_RELEASE_MIN_BLOCK", "RRX_LIMIT_RELEASE_MAX_BLOCK",
           "limit_window_reach", "tracks_limit_window_work_doubles", "tracks_limit_window_device",
           "tracks_limit_release_window_work_doubles", "tracks_limit_release_window_device", "RRX_LIMIT_RELEASE_WIN_STATE",
           "PackedPlan", "PackedTable", "packed_plan", "tracks_true_peak_packed_device", "tracks_loudness_packed_device", "scan_tracks_pcm",
           "MIX_MATRICES", "RRX_MIX_MAX_CH", "mix_matrix", "mix_device", "tracks_stage_mix_device", "tracks_stage_mix_window_device",
           "ALBUM_SYMBOLS", "RRX_LINK_NONE", "RRXTrackLink", "TracksAlbumPlan", "tracks_plan_album", "tracks_stage_album_device",
           "tracks_stage_album_window_device"]
