// The two measuring passes of a ragged batch by windows ("Windows with true peak and loudness"):
// RRX_tracks_true_peak_window_device and RRX_tracks_loudness_window_device.  The arithmetic is true_peak_frame (true_peak.hpp) and
// loudness_step / loudness_carry (loudness.hpp), unchanged; what is new is the geometry -- a window cuts every track's slice, and
// every track's hops, at a different place -- and a per-track state that crosses windows.  The cut functions below are called by
// the kernels (measure_window.hip) and by the host twins alike, so they cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

#include "loudness.hpp"
#include "tracks.hpp"
#include "true_peak.hpp"

namespace rsmp {

// ------------------------------------------------------------------------------------------------------------------ true peak
// What RRX_tracks_true_peak_window_device was given, after validation (pointers of the device, or of the host for the twin).
struct TruePeakWindowArgs {
  const void *src;                 // the window buffer [ntracks][w.stride][nch]: float (src_double = 0) or double
  const double *gain;              // [ntracks], null = unity
  const double *state_in;          // [ntracks * nch][kTpMaxTaps], null only with w.first == 0
  double *state_out;               // the same layout, null = not wanted
  double *true_peak, *peak;        // [ntracks * nch] each, null = not taken
  const Track *tracks;             // [ntracks]
  unsigned long long row_frames;   // length of the virtual rows
  TracksWindow w;
  int ntracks, nch;
  int src_double;
  TruePeakFilter f;
};

// Track t's part of a true-peak window call: window frames [w0, w0 + frames) are frames index, index + 1, ... of its slice;
// flush: the window holds the slice's last frame.  frames == 0: the window does not touch the track.
struct TruePeakWindowCut {
  unsigned long long w0, frames, index;
  bool flush;
};

__host__ __device__ __forceinline__ TruePeakWindowCut true_peak_window_cut(const Track &tr, unsigned long long row_frames, const TracksWindow &w)
{
  const TracksFinishCut c = tracks_finish_cut(tr, row_frames, 0, false, w);
  const TracksSlice s = tracks_slice(tr, row_frames, 0, false);
  TruePeakWindowCut r;
  r.w0 = c.w0;
  r.frames = c.w1 - c.w0;
  r.index = c.index;
  r.flush = r.frames && c.index + r.frames == s.frames;
  return r;
}

hipError_t launch_true_peak_window(hipStream_t stream, const TruePeakWindowArgs &a);
void true_peak_window_host(const TruePeakWindowArgs &a);

// ------------------------------------------------------------------------------------------------------------------- loudness
constexpr int kLoudnessWinState = 16; // S[4], Z[4], C[4], E, three zeros

// What RRX_tracks_loudness_window_device was given, after validation.
struct LoudnessWindowArgs {
  const void *src;                 // the window buffer [ntracks][w.stride][nch]
  const double *gain;              // [ntracks], null = unity
  const double *state_in;          // [ntracks * nch][kLoudnessWinState], null only with w.first == 0
  double *state_out;               // the same layout, null = not wanted
  double *energy;                  // channel c's hops at energy + c * energy_stride
  double *work;                    // [ntracks][pieces][nch][4]: a piece's z after launch 1, its hop's start state after launch 2
  const Track *tracks;             // [ntracks]
  unsigned long long *hops_out;    // [ntracks]
  unsigned long long row_frames;
  unsigned long long hop, pieces;  // pieces = w.frames / hop + 2: what a track's range meets at most
  unsigned long long energy_stride;
  TracksWindow w;
  int ntracks, nch;
  int src_double;
  double c[10], m[16];
};

inline unsigned long long loudness_window_work_doubles(unsigned long long ntracks, unsigned long long nch, unsigned long long win_frames,
                                                       unsigned long long hop)
{
  return hop ? ntracks * nch * (win_frames / hop + 2ull) * 4ull : 0ull;
}

// Track t's part of a loudness window call.  n: the whole-row call's hop count; the processed range is the finish cut of the
// window intersected with slice frames [0, n * hop): window frames [w0, w0 + frames), which begin r0 frames into hop k0 of the
// track.  The range meets `pieces` hops; frames == 0: nothing of the track is processed.
struct LoudnessWindowCut {
  unsigned long long n, w0, frames, index, k0, r0, pieces;
};

__host__ __device__ __forceinline__ LoudnessWindowCut loudness_window_cut(const Track &tr, unsigned long long row_frames, unsigned long long hop,
                                                                          unsigned long long energy_stride, const TracksWindow &w)
{
  const TracksFinishCut c = tracks_finish_cut(tr, row_frames, 0, false, w);
  const TracksSlice s = tracks_slice(tr, row_frames, 0, false);
  LoudnessWindowCut r;
  r.n = s.frames / hop;
  if (r.n > energy_stride) r.n = energy_stride;
  const unsigned long long last = r.n * hop, end = c.index + (c.w1 - c.w0) < last ? c.index + (c.w1 - c.w0) : last; // (n * hop <= slice frames)
  r.w0 = c.w0;
  r.index = c.index;
  r.frames = end > c.index ? end - c.index : 0;
  r.k0 = c.index / hop;
  r.r0 = c.index - r.k0 * hop;
  r.pieces = r.frames ? (r.r0 + r.frames + hop - 1) / hop : 0; // <= frames / hop + 2: r0 < hop
  return r;
}

// Piece j of a cut, j < pieces: hop k0 + j, of which frames [a, b) lie in the range; they begin `off` frames behind window frame w0.
struct LoudnessPiece {
  unsigned long long a, b, off;
};

__host__ __device__ __forceinline__ LoudnessPiece loudness_piece(const LoudnessWindowCut &c, unsigned long long hop, unsigned long long j)
{
  LoudnessPiece p;
  p.a = j ? 0 : c.r0;
  const unsigned long long left = c.r0 + c.frames - j * hop; // frames of the range from the start of hop k0 + j on
  p.b = left < hop ? left : hop;
  p.off = j * hop + p.a - c.r0;
  return p;
}

hipError_t launch_loudness_window(hipStream_t stream, const LoudnessWindowArgs &a);
void loudness_window_host(const LoudnessWindowArgs &a);

} // namespace rsmp
