// Channel mixing ("Channel mixing"): a matrix [nch_dst][nch_src] applied per frame, on load in the stage pass of a
// ragged batch (RRX_tracks_stage_mix_device and its window form) and on plain rows (RRX_mix_device).  Implemented in
// tracks_mix.hip; everything that includes this header is compiled with -ffp-contract=off.
//
// The rule is part of the ABI (include/ratelib_amd.h).  For one frame and output channel o
//   v_c = the source sample of channel c as an exact double (tracks_load_value, tracks.hpp; a double row sample as it is)
//   y_o = sum over c ascending of mix[o][c] * v_c, every product and every sum rounded on its own in fp64, never fused,
//         WITHOUT the terms whose coefficient is zero (either sign); the sum starts from its first product; no term: +0.0
//   x_o = (float)y_o for float32 rows, y_o for float64 rows
// A zero coefficient means "not connected": what an unconnected channel holds, a NaN included, does not reach the output, and
// -0.0 passes through a permutation.  tracks_mix_sum below is that rule, once: the kernels, the LPC base-frame loads
// (tracks_mix.hip) and the host loops behind RRX_debug_mix_host / RRX_debug_tracks_mix_host (capi_stage.cpp) all call it.
#pragma once
#include "tracks.hpp"

namespace rsmp {

constexpr int kMixMaxCh = 16; // RRX_MIX_MAX_CH

// What a mixed source holds: TracksSrc (tracks.hpp), and float64 rows for RRX_mix_device
constexpr int kMixSrcF64 = 4;

constexpr int mix_src_bytes(int kind) { return kind == kMixSrcF64 ? 8 : tracks_src_bytes(kind); }

// The copy kernels bring the source bytes of a tile of consecutive frames into LDS: at most kMixTileBytes of them, so a tile is
//   mix_tile_frames(kind, nch_src) = kMixTileBytes / (nch_src * bytes of a sample)   frames
// (at least 128: 16 channels of float64).  Tiles count from frame 0 of a row, of a window or of a stream.
constexpr int kMixTileBytes = 16384;

constexpr int mix_tile_frames(int kind, int nch_src) { return kMixTileBytes / (nch_src * mix_src_bytes(kind)); }

// The matrix as the kernels take it, in their launch arguments: the connected terms of every output channel, in the order of
// the sum.  Output channel o owns terms [start[o], start[o + 1]); coef holds the caller's coefficients bit for bit.
struct TracksMix {
  double coef[kMixMaxCh * kMixMaxCh];
  unsigned char col[kMixMaxCh * kMixMaxCh]; // the source channel of a term
  unsigned short start[kMixMaxCh + 1];
  int nch_src, nch_dst;
};

// mix: [nch_dst][nch_src], row-major.  False for a coefficient that is not finite.
inline bool tracks_mix_build(const double *mix, int nch_src, int nch_dst, TracksMix &m)
{
  int n = 0;
  for (int o = 0; o < nch_dst; ++o) {
    m.start[o] = (unsigned short)n;
    for (int c = 0; c < nch_src; ++c) {
      const double k = mix[o * nch_src + c];
      if (!(k - k == 0.0)) return false; // NaN or infinity
      if (k == 0.0) continue;
      m.coef[n] = k;
      m.col[n] = (unsigned char)c;
      ++n;
    }
  }
  for (int o = nch_dst; o <= kMixMaxCh; ++o) m.start[o] = (unsigned short)n;
  for (; n < kMixMaxCh * kMixMaxCh; ++n) m.coef[n] = 0.0, m.col[n] = 0; // (never read)
  m.nch_src = nch_src;
  m.nch_dst = nch_dst;
  return true;
}

// Channel c of the frame at `frame` (nch_src samples of `kind`, at the alignment of one sample) as the exact double
__host__ __device__ __forceinline__ double tracks_mix_value(int kind, const void *frame, unsigned c)
{
  return kind == kMixSrcF64 ? static_cast<const double *>(frame)[c] : tracks_load_value(kind, frame, c);
}

// y_o of the frame at `frame`: the rule above.  Reads exactly the bytes of the connected channels' samples.
__host__ __device__ __forceinline__ double tracks_mix_sum(const TracksMix &m, int kind, const void *frame, int o)
{
  int k = m.start[o];
  const int end = m.start[o + 1];
  if (k == end) return 0.0;
  double y = m.coef[k] * tracks_mix_value(kind, frame, m.col[k]);
  for (++k; k < end; ++k) {
    const double p = m.coef[k] * tracks_mix_value(kind, frame, m.col[k]);
    y = y + p;
  }
  return y;
}

// x_o for float32 rows: one rounding, to nearest even, from the fp64 sum -- for an S32 source from the exact sum, which is NOT
// the result of converting to float32 first (tracks_load_sample) and mixing afterwards
__host__ __device__ __forceinline__ float tracks_mix_sample(const TracksMix &m, int kind, const void *frame, int o)
{
  return (float)tracks_mix_sum(m, kind, frame, o);
}

// what RRX_mix_device was given, after validation
struct MixRowsArgs {
  const void *src;                           // [nstreams][src_stride / nch_src][nch_src]: float (is_double = 0) or double
  void *dst;                                 // [nstreams][dst_stride / nch_dst][nch_dst], the same type
  unsigned long long src_stride, dst_stride; // samples
  unsigned long long frames;
  int nstreams;
  int is_double;
};

// All three only enqueue on `stream`.  The stage forms take TracksStageArgs (tracks.hpp) with a.nch the channels of the ROWS
// (m.nch_dst) and the packed source [src_total][m.nch_src]; clamps, regions and the window are launch_tracks_stage's.  The copy
// kernel loads aligned 16-byte pieces and, at a tile's ends, single dwords: only dwords that hold a byte of the frames it mixes.
hipError_t launch_tracks_stage_mix(hipStream_t stream, const TracksStageArgs &a, const TracksMix &m);
hipError_t launch_tracks_stage_mix_window(hipStream_t stream, const TracksStageArgs &a, const TracksMix &m, const TracksWindow &w);
hipError_t launch_mix_rows(hipStream_t stream, const MixRowsArgs &a, const TracksMix &m);

// the host twins: serial loops over tracks_mix_sum
void mix_rows_host(const MixRowsArgs &a, const TracksMix &m);

} // namespace rsmp
