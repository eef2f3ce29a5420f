// Programme loudness for device-resident frames ("Loudness"): K-weighted energies of 100 ms hops per (stream,
// channel) and the two-stage gate of ITU-R BS.1770-4 over them.  K-weighting is two biquads, an IIR recursion, so the hop energies
// are defined by an exact block decomposition (include/ratelib_amd.h, RRX_loudness_device): the functions below are that
// arithmetic, and both the kernels (loudness.hip) and the host twins behind RRX_debug_loudness_host / RRX_debug_loudness_gate_host
// are loops around them, so they cannot drift apart.  The files that include this are compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

#include "tracks.hpp"

namespace rsmp {

// One frame of one channel through both biquads (transposed direct form II): c[0..4] = b0, b1, b2, a1, a2 of stage A, c[5..9] of
// stage B; s[0..1] is stage A's state, s[2..3] stage B's.  Returns the K-weighted sample v.
__host__ __device__ __forceinline__ double loudness_step(const double *c, double g, double (&s)[4])
{
  const double y = c[0] * g + s[0];
  s[0] = (c[1] * g - c[3] * y) + s[1];
  s[1] = c[2] * g - c[4] * y;
  const double v = c[5] * y + s[2];
  s[2] = (c[6] * y - c[8] * v) + s[3];
  s[3] = c[7] * y - c[9] * v;
  return v;
}

// S' = M S + z, row i as (((M[i][0] S[0] + M[i][1] S[1]) + M[i][2] S[2]) + M[i][3] S[3]) + z[i]; m is row-major
__host__ __device__ __forceinline__ void loudness_carry(const double *m, const double *z, double (&s)[4])
{
  double r[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = (((m[4 * i] * s[0] + m[4 * i + 1] * s[1]) + m[4 * i + 2] * s[2]) + m[4 * i + 3] * s[3]) + z[i];
#pragma unroll
  for (int i = 0; i < 4; ++i) s[i] = r[i];
}

// out = x y (4 x 4, row-major): every entry an ascending-k sum from +0.0, products and sums rounded on their own
inline void loudness_matmul(const double *x, const double *y, double *out)
{
  double r[16];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      double acc = 0.0;
      for (int k = 0; k < 4; ++k) acc = acc + x[4 * i + k] * y[4 * k + j];
      r[4 * i + j] = acc;
    }
  for (int i = 0; i < 16; ++i) out[i] = r[i];
}

// M = A^hop, hop >= 1.  Column i of A is one loudness_step with g = 0 from the unit state e_i; the power is square-and-multiply
// over the bits of hop from the most significant one: R = A, then for every lower bit R = R R and, where the bit is set, R = R A.
inline void loudness_power(const double *c, unsigned long long hop, double *m)
{
  double a[16];
  for (int i = 0; i < 4; ++i) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    s[i] = 1.0;
    loudness_step(c, 0.0, s);
    for (int r = 0; r < 4; ++r) a[4 * r + i] = s[r];
  }
  int top = 63;
  while (!(hop >> top)) --top;
  for (int i = 0; i < 16; ++i) m[i] = a[i];
  for (int b = top - 1; b >= 0; --b) {
    loudness_matmul(m, m, m);
    if ((hop >> b) & 1) loudness_matmul(m, a, m);
  }
}

// What RRX_loudness_device (tracks == null) or RRX_tracks_loudness_device (tracks != null) was given, after validation (pointers
// of the device, or of the host for loudness_host).
struct LoudnessArgs {
  const void *src;                 // frame 0 of stream 0, or the output rows [ntracks][row_frames][nch]: float (src_double = 0) or double
  const double *gain;              // [nstreams], null = unity
  const double *state_in;          // [nstreams * nch][4]; null: S_0 = +0.0
  double *state_out;               // the same layout, or null (tracks)
  double *energy;                  // channel c's hops at energy + c * energy_stride
  double *work;                    // [nstreams][max_hops][nch][4]: z_k after pass 1, S_k after the carry
  const Track *tracks;             // [nstreams] on the device: stream t is track t's slice of row t, from +0.0
  unsigned long long *hops_out;    // [nstreams], tracks only: the hops measured per track
  unsigned long long src_stride;   // SAMPLES between streams (tracks: unused; packed: FRAMES of the source, src_total)
  unsigned long long frames;       // per stream (tracks: the rows' length, row_frames; packed: max_frames)
  unsigned long long hop, max_hops; // max_hops = frames / hop: what a stream has (tracks: at most)
  unsigned long long first_hop;    // first_frame / hop
  unsigned long long energy_stride;
  int nstreams, nch;
  int src_double;
  double c[10], m[16];
};

inline unsigned long long loudness_work_doubles(unsigned long long nstreams, unsigned long long nch, unsigned long long frames, unsigned long long hop)
{
  return hop ? nstreams * nch * (frames / hop) * 4ull : 0ull;
}

// What RRX_loudness_gate_device was given, after validation
struct LoudnessGateArgs {
  const double *energy;            // channel c's hops at energy + c * energy_stride
  const unsigned long long *hops;  // [nstreams] or null: nhops for all
  const double *weights;           // [nch] or null: 1.0
  double *result;                  // [nstreams][4]: S2, N2, S1, N1
  unsigned long long energy_stride, nhops;
  int nstreams, nch;
  double inv, abs_threshold, rel_factor; // inv = 1 / (4 hop)
};

// z_j of one stream: e = the stream's channel 0, hop j
__host__ __device__ __forceinline__ double loudness_block(const LoudnessGateArgs &a, const double *e, unsigned long long j)
{
  double acc = 0.0;
  for (int ch = 0; ch < a.nch; ++ch) {
    const double *p = e + (unsigned long long)ch * a.energy_stride + j;
    const double q = ((p[0] + p[1]) + p[2]) + p[3];
    acc = a.weights ? acc + a.weights[ch] * q : acc + q;
  }
  return acc * a.inv;
}

// All three only enqueue on `stream` (loudness: pass 1, the carry, pass 3, each split into as many launches as the grid limits ask
// for); the arguments are the caller's to validate.  The table of the tracks form cannot be: the kernels clamp what they take from
// it (tracks_slice, and the hop count to energy_stride and max_hops).
hipError_t launch_loudness(hipStream_t stream, const LoudnessArgs &a);
hipError_t launch_loudness_gate(hipStream_t stream, const LoudnessGateArgs &a);
// The plain call's results on host pointers, as serial loops over the functions above (test hooks).
void loudness_host(const LoudnessArgs &a);
// RRX_tracks_loudness_packed_device: a.src is a packed source of `kind` (TracksSrc) of a.src_stride frames, a.tracks the table,
// a.frames the most frames a track is measured for (max_hops = a.frames / hop); track t is tracks_packed_cut's clamp of its entry,
// from +0.0.  The kernel arguments keep their layout, so the kind travels beside them.  The second is its host twin: the loops of
// loudness_host over the same rows, which also leaves hops_out.
hipError_t launch_loudness_packed(hipStream_t stream, const LoudnessArgs &a, int kind);
void loudness_packed_host(const LoudnessArgs &a, int kind);
void loudness_gate_host(const LoudnessGateArgs &a);

} // namespace rsmp
