// True-peak limiter for device-resident frames ("Limiter"): a gain per frame, linked across a stream's channels,
// that holds the gained frames' sample peak at a ceiling and their true peak near it.  The detector is true_peak_frame
// (true_peak.hpp); the gain is a window minimum of the demanded reductions smoothed by a box of `lookahead` frames, so nothing in
// it is recursive.  The per-frame arithmetic below is the ABI of RRX_limit_device (include/ratelib_amd.h); the kernels
// (limit.hip) and the host twin behind RRX_debug_limit_host are both loops around these functions, so they cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

#include "tracks.hpp"
#include "true_peak.hpp"

namespace rsmp {

constexpr int kLimitMaxLookahead = 1024, kLimitMaxHold = 4096;

// The reduction a detector frame demands: `lev` is the bit pattern of the frame's level, the largest true peak or |sample| over
// the stream's channels.  A NaN level fails the comparison and demands nothing; +inf demands +0.0.  The division is correctly
// rounded.  Never a NaN, never below +0.0, never above 1.0.
__host__ __device__ __forceinline__ double limit_reduction(unsigned long long lev, double ceiling)
{
  double v;
  __builtin_memcpy(&v, &lev, sizeof(v));
  return v > ceiling ? ceiling / v : 1.0;
}

// The gains of kN consecutive frames n, n + 1, ... from the window minima: m(t) is m[n - (lookahead - 1) + t], and frame n + j
// sums m(j) .. m(j + lookahead - 1) serially from the oldest to the newest, every sum rounded on its own; the fmin keeps the sum's
// rounding from lifting the gain above the frame's own m.  Every m(t) is loaded once and goes to the frames it belongs to: kN
// independent sums, each in the order of the single frame's (kN = 1: limit_smooth).  m(t) is read for t < lookahead + kN - 1.
template <int kN, typename Load>
__host__ __device__ __forceinline__ void limit_smooth_frames(Load &&m, unsigned lookahead, double inv_l, double (&s)[kN])
{
  double acc[kN];
#pragma unroll
  for (int j = 0; j < kN; ++j) acc[j] = 0.0;
  const unsigned head = (unsigned)(kN - 1), tail = lookahead > head ? lookahead : head; // [head, tail): inside every frame's window
  for (unsigned t = 0; t < head; ++t) {
    const double v = m(t);
#pragma unroll
    for (int j = 0; j < kN; ++j)
      if (t >= (unsigned)j && t - (unsigned)j < lookahead) acc[j] = acc[j] + v;
  }
#pragma unroll 4
  for (unsigned t = head; t < lookahead; ++t) {
    const double v = m(t);
#pragma unroll
    for (int j = 0; j < kN; ++j) acc[j] = acc[j] + v;
  }
  for (unsigned t = tail; t < lookahead + head; ++t) {
    const double v = m(t);
#pragma unroll
    for (int j = 0; j < kN; ++j)
      if (t >= (unsigned)j && t - (unsigned)j < lookahead) acc[j] = acc[j] + v;
  }
#pragma unroll
  for (int j = 0; j < kN; ++j) s[j] = fmin(acc[j] * inv_l, m((unsigned)j + lookahead - 1));
}

// y of a gained sample under its frame's gain: one product, stored as a double or rounded once to float32
template <typename T> __host__ __device__ __forceinline__ T limit_output(double g, double s) { return (T)(g * s); }

// one frame: m[0 .. lookahead) are m[n - (lookahead - 1)] .. m[n]
__host__ __device__ __forceinline__ double limit_smooth(const double *m, unsigned lookahead, double inv_l)
{
  double s[1];
  limit_smooth_frames<1>([m](unsigned t) { return m[t]; }, lookahead, inv_l, s);
  return s[0];
}

// What RRX_limit_device (tracks == null) or RRX_tracks_limit_device (tracks != null) was given, after validation (pointers of the
// device, or of the host for limit_host).
struct LimitArgs {
  const void *src;                 // frame 0 of stream 0, or the rows [ntracks][row_frames][nch]: float (src_double = 0) or double
  void *dst;                       // the same geometry with dst_stride; may be src
  const double *gain;              // [nstreams], null = unity
  double *reduction;               // [nstreams], the smallest gain (an atomic minimum on the bit pattern), null = not taken
  unsigned long long *limited;     // [nstreams], frames with a gain below 1.0, added, null = not taken
  double *work;                    // [nstreams][2][work_stride]: r, then m
  const Track *tracks;             // [nstreams] on the device: stream t is track t's slice of row t
  unsigned long long src_stride, dst_stride; // SAMPLES between streams (tracks: unused)
  unsigned long long frames;       // per stream (tracks: the rows' length, row_frames)
  unsigned long long work_stride;  // frames + taps + lookahead: room for frames + taps - 1 of r and frames + lookahead - 1 of m
                                   // (with a release: more, the blocks' summaries lie behind each: limit_release.hpp)
  unsigned lookahead, hold;
  double ceiling, inv_l;           // inv_l = 1.0 / (double)lookahead
  int nstreams, nch;
  int src_double, dst_double;
  TruePeakFilter f;
};

// The window form (RRX_tracks_limit_window_device; a.tracks != null) takes this beside its LimitArgs, in which `frames` is then
// the length of the virtual rows, src the buffer [nstreams][src_stride / nch][nch] that holds their frames [buf_first, buf_first
// + buf_frames), dst [nstreams][dst_stride / nch][nch], whose frame j receives row frame win_first + j, and work_stride
// win_frames + 2 * lookahead + hold + 2 * taps.  Of every slice the frames inside [win_first, win_first + win_frames) are emitted.
// (A struct of its own: the whole-row kernels' arguments stay what they were.)
struct LimitWindow {
  unsigned long long win_first, win_frames, buf_first, buf_frames;
};

// How far the gain of a frame reaches (RRX_limit_window_reach): frame n depends on the samples of [n - back, n + ahead] only.
// m[n - i], i < lookahead, covers r[F], F in [n - (lookahead - 1) - hold, n + lookahead - 1 + taps - 1], and r[F] reads the
// frames [F - (taps - 1), F].
__host__ __device__ __forceinline__ unsigned long long limit_reach_back(int taps, unsigned lookahead, unsigned hold)
{
  return (unsigned long long)(lookahead - 1) + hold + (unsigned)(taps - 1);
}
__host__ __device__ __forceinline__ unsigned long long limit_reach_ahead(int taps, unsigned lookahead)
{
  return (unsigned long long)(lookahead - 1) + (unsigned)(taps - 1);
}

// Window minimum (launch 2): a workgroup holds kLimitMinTile entries of r in LDS, of which lookahead + hold + taps - 2 are halo.
// Smoothing (launch 3): a workgroup takes kLimitApplyFrames frames, kLimitLaneFrames consecutive ones to a lane, with
// lookahead - 1 further entries of m.
constexpr int kLimitMinTile = 8192, kLimitApplyFrames = 1024, kLimitLaneFrames = 4;

// Only enqueues on `stream`: three launches, each split into as many as the grid limits ask for; the arguments are the caller's
// to validate.  The table of the tracks form cannot be: the kernels clamp what they take from it (tracks_slice, tracks.hpp).
// With a window the same three launches run on the sub-range of every row that the window asks for: the detector on the frames
// within reach of it, the minimum on the entries of m under its frames, the product on its frames.
hipError_t launch_limit(hipStream_t stream, const LimitArgs &a, const LimitWindow *w = nullptr);
// The plain call's results on host pointers, as serial loops over the functions above (test hooks: RRX_debug_limit_host and,
// with a window and a host table, RRX_debug_tracks_limit_window_host).
void limit_host(const LimitArgs &a, const LimitWindow *w = nullptr);

// The whole-row form in parts, for a call that puts launches of its own between the window minimum and the product (the release,
// limit_release.hip): the launches [first, last) of detect (0), window minimum (1), product (2), which reads as m whatever the
// work buffer then holds in its place.  launch_limit(stream, a) is launch_limit_passes(stream, a, 0, 3).
hipError_t launch_limit_passes(hipStream_t stream, const LimitArgs &a, int first, int last);
// limit_host likewise: head = r and m, tail = the gains, the product and the statistics
void limit_host_passes(const LimitArgs &a, bool head, bool tail);
// The window form in parts, likewise (the release by windows, limit_release_window.hip): the same launches on the window's
// sub-range of every row.  launch_limit(stream, a, &w) is launch_limit_window_passes(stream, a, w, 0, 3).
hipError_t launch_limit_window_passes(hipStream_t stream, const LimitArgs &a, const LimitWindow &w, int first, int last);
void limit_host_window_passes(const LimitArgs &a, const LimitWindow &w, bool head, bool tail);

} // namespace rsmp
