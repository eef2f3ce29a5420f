// True-peak measurement for device-resident frames ("True peak"): the peak of the gained frames oversampled by a
// caller-supplied polyphase filter (ITU-R BS.1770-4 Annex 2 with the 4 x 12 table), beside the sample peak, per (stream, channel).
// The per-frame arithmetic below is the ABI of RRX_true_peak_device (include/ratelib_amd.h); the kernels (true_peak.hip) and the
// host twin behind RRX_debug_true_peak_host are both loops around true_peak_frame, so they cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

#include "tracks.hpp"

namespace rsmp {

constexpr int kTpMaxPhases = 8, kTpMaxTaps = 16;

// the filter as the caller gave it: phase-major, phases * taps coefficients, NOT padded (0 * inf is a NaN: a padded table would
// give other bits for non-finite samples)
struct TruePeakFilter {
  double c[kTpMaxPhases * kTpMaxTaps];
  int phases, taps;
};

// bits of a non-negative double order as unsigned integers (a NaN, sign cleared by fabs, lies above +inf and stays)
__host__ __device__ __forceinline__ unsigned long long true_peak_bits(double a)
{
  unsigned long long b;
  __builtin_memcpy(&b, &a, sizeof(b));
  return b;
}

// One frame of one channel: h[k] is the gained sample k frames back (h[0] the frame itself), k < taps.  Every phase is one serial
// sum from the oldest tap to the newest, each product and each sum rounded on its own (the files that include this are compiled
// with -ffp-contract=off); the result is the largest |y_p| as a bit pattern.  kP / kT: the filter's shape when it is known at
// compile time, 0 = take it from `phases` / `taps`; an instance with a fixed shape runs the same operations in the same order as
// the loop, only unrolled.
template <int kP, int kT>
__host__ __device__ __forceinline__ unsigned long long true_peak_frame(const double *coefs, int phases, int taps, const double (&h)[kTpMaxTaps])
{
  const int np = kP ? kP : phases, nt = kT ? kT : taps;
  unsigned long long best = 0;
#pragma unroll
  for (int p = 0; p < (kP ? kP : kTpMaxPhases); ++p) {
    if (p < np) {
      double acc = 0.0;
#pragma unroll
      for (int k = kTpMaxTaps - 1; k >= 0; --k)
        if (k < nt) acc = acc + coefs[p * nt + k] * h[k];
      const unsigned long long b = true_peak_bits(fabs(acc));
      best = b > best ? b : best;
    }
  }
  return best;
}

// What RRX_true_peak_device (tracks == null) or RRX_tracks_true_peak_device (tracks != null) was given, after validation
// (pointers of the device, or of the host for true_peak_host).
struct TruePeakArgs {
  const void *src;                 // frame 0 of stream 0, or the output rows [ntracks][row_frames][nch]: float (src_double = 0) or double
  const double *gain;              // [nstreams], null = unity
  const double *state_in;          // [nstreams * nch][kTpMaxTaps]; null: the history in front of the call is +0.0
  double *state_out;               // the same layout, null = not wanted
  double *true_peak, *peak;        // [nstreams * nch] each, null = not taken
  const Track *tracks;             // [nstreams] on the device: stream t is track t's slice of row t, flushed, without a state
  unsigned long long src_stride;   // SAMPLES between streams (tracks: unused; packed: FRAMES of the source, src_total)
  unsigned long long frames;       // per stream (tracks: the rows' length, row_frames; packed: max_frames)
  int nstreams, nch;
  int src_double;
  int flush;
  TruePeakFilter f;
};

// One-frame tile plus halo, nch * taps doubles, has to fit kTpLdsDoubles of LDS and nch the per-channel tables of the workgroup;
// any other channel count takes the direct form, which reads its taps from global memory.
constexpr int kTpLdsDoubles = 4096, kTpLdsChannels = 1024;
inline bool true_peak_lds_form(int nch, int taps)
{
  return nch <= kTpLdsChannels && (unsigned long long)nch * (unsigned)taps <= (unsigned long long)kTpLdsDoubles;
}

// Only enqueues on `stream`, split into as many launches as the grid limits ask for; the arguments are the caller's to validate.
// The table of the tracks form cannot be: the kernel clamps what it takes from it (tracks_slice, tracks.hpp).
hipError_t launch_true_peak(hipStream_t stream, const TruePeakArgs &a);
// The plain call's results on host pointers, as one serial loop over true_peak_frame (test hook: RRX_debug_true_peak_host).
void true_peak_host(const TruePeakArgs &a);
// RRX_tracks_true_peak_packed_device: a.src is a packed source of `kind` (TracksSrc) of a.src_stride frames, a.tracks the table,
// a.frames the most frames a track is measured for; track t is tracks_packed_cut's clamp of its entry, flushed, without a state.
// The kernel arguments keep their layout, so the kind travels beside them.  The second is its host twin, the same loop as above.
hipError_t launch_true_peak_packed(hipStream_t stream, const TruePeakArgs &a, int kind);
void true_peak_packed_host(const TruePeakArgs &a, int kind);

} // namespace rsmp
