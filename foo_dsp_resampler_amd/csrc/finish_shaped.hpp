// Noise-shaped dither for the output stage ("Noise-shaped dither"): finish.hpp's gain, TPDF dither and PCM
// quantisation with the requantisation error of a channel's previous 1..16 frames fed back through an FIR filter, in segments
// whose error history starts from zero.  The per-sample arithmetic below is the ABI of RRX_finish_shaped_device
// (include/ratelib_amd.h); the kernels (finish_shaped.hip) and the host twin behind RRX_debug_finish_shaped_host are loops around
// shaped_front and shaped_step, so they cannot drift apart.  finish_dither, finish_store_bytes and FinishSample are finish.hpp's.
#pragma once
#include "finish.hpp"
#include "tracks.hpp"

namespace rsmp {

constexpr int kShapeMaxOrder = 16; // RRX_SHAPE_MAX_ORDER

// what RRX_finish_shaped_device was given, after validation (pointers of the device, or of the host for finish_shaped_host)
struct ShapedArgs {
  const void *src;                    // frame 0 of stream 0: float (src_double = 0) or double
  void *dst;                          // null: measure only (bits still those of the destination format)
  const double *gain;                 // [nstreams], null = unity
  double *peak;                       // [nstreams * nch], null = not taken
  unsigned long long *clipped;        // [nstreams * nch], null = not taken
  const double *state_in;             // [nstreams * nch][kShapeMaxOrder]; read only when the call begins inside a segment
  double *state_out;                  // the same layout, null = not wanted
  unsigned long long src_stride, dst_stride; // SAMPLES between streams
  unsigned long long frames;
  unsigned long long seed, first_frame;
  unsigned long long segment;         // frames between restarts of the history, 0 = never
  int nstreams, nch;
  int src_double;
  int bits;                           // 15 / 23 / 31: S16, packed S24, S32
  int dither;
  int order;                          // 1..kShapeMaxOrder
  double coefs[kShapeMaxOrder];       // zeros from `order` on
};

// what RRX_tracks_finish_shaped_device was given, after validation: TracksFinishArgs and the filter
struct TracksShapedArgs {
  TracksFinishArgs t;                 // t.bits is the destination format's, measure only included
  unsigned long long segment;
  int order;
  double coefs[kShapeMaxOrder];
};

// what RRX_tracks_finish_shaped_window_device was given, after validation: s.t.src is the window buffer [ntracks][w.stride][nch]
// with frames [w.first, w.first + w.frames) of the output rows, s.t.row_frames the length of the virtual rows
struct TracksShapedWindowArgs {
  TracksShapedArgs s;
  TracksWindow w;                     // w.frames > 0
  const double *state_in;             // [ntracks * nch][kShapeMaxOrder]; null only with w.first == 0
  double *state_out;                  // the same layout, every entry written; null = not wanted
};

// The part of a sample that does not depend on the channel's earlier errors: the gained sample's magnitude, the scaled sample
// and the dither.  g and t are finish_sample's.
struct ShapedFront {
  double a, t, d;
};

__host__ __device__ __forceinline__ ShapedFront shaped_front(double v, bool has_gain, double gain, double scale, bool dither,
                                                             unsigned long long seed, unsigned long long frame, unsigned long long c)
{
  ShapedFront f;
  const double g = has_gain ? v * gain : v;
  f.a = fabs(g);
  f.t = g * scale;
  f.d = dither ? finish_dither(seed, frame, c) : 0.0;
  return f;
}

// The recursion.  e[k - 1] is the error of the channel's k-th previous frame; kK >= order, with coef[order..kK) zero, gives the
// bits of kK = order: acc starts at +0.0, the errors are finite, and +0.0 + (+-0.0) = +0.0.  The sum runs from the oldest error
// to the newest, so everything but its last term is known before the previous sample's error is.
template <int kK>
__host__ __device__ __forceinline__ FinishSample shaped_step(const ShapedFront &f, bool dither, double lo, double hi, const double (&coef)[kK],
                                                             double (&e)[kK])
{
  FinishSample r;
  r.a = f.a;
  double acc = 0.0;
#pragma unroll
  for (int k = kK; k >= 1; --k) acc = acc + coef[k - 1] * e[k - 1];
  const double w = f.t - acc;
  const double u = dither ? w + f.d : w;
  const double q = rint(u);
  r.clip = !(q >= lo && q <= hi);
  r.q = (int)fmin(fmax(q, lo), hi);
  double err = q - w; // from the unsaturated q: a clipped passage does not wind the filter up
  if (!(fabs(err) <= 2.0)) err = 0.0; // +-inf or a NaN leaves no trace
#pragma unroll
  for (int k = kK - 1; k >= 1; --k) e[k] = e[k - 1];
  e[0] = err;
  return r;
}

// Whether a channel's history is all zeros in front of absolute frame F
__host__ __device__ __forceinline__ bool shaped_restarts(unsigned long long F, unsigned long long segment)
{
  return segment ? F % segment == 0 : F == 0;
}

// All three only enqueue on `stream`, split into as many launches as the grid limits ask for; the arguments are the caller's to
// validate.  The table of the tracks form cannot be: the kernel clamps what it takes from it (tracks_slice, tracks.hpp).
hipError_t launch_finish_shaped(hipStream_t stream, const ShapedArgs &a);
hipError_t launch_tracks_finish_shaped(hipStream_t stream, const TracksShapedArgs &a);
// The window form: of every track's slice the frames inside the window (tracks_finish_cut), as a one-stream shaped call on them
// with first_frame = their index in the track and the track's entries of the state.
hipError_t launch_tracks_finish_shaped_window(hipStream_t stream, const TracksShapedWindowArgs &a);
// RRX_finish_shaped_device's results on host pointers, as one serial loop per channel over shaped_front and shaped_step
// (test hook: RRX_debug_finish_shaped_host).
void finish_shaped_host(const ShapedArgs &a);
// RRX_tracks_finish_shaped_window_device's results on host pointers and a HOST table, as one serial loop per (track, channel) over
// tracks_finish_cut, shaped_front and shaped_step (test hook: RRX_debug_tracks_finish_shaped_window_host).
void tracks_finish_shaped_window_host(const TracksShapedWindowArgs &a);

} // namespace rsmp
