// Output stage for device-resident frames: gain, TPDF dither, PCM quantisation, peak and clipped-sample count.
// The per-sample arithmetic below is the ABI of RRX_finish_device (include/ratelib_amd.h); the kernel (finish.hip) and the host
// twin behind RRX_debug_finish_host (capi_stage.cpp) are both loops around finish_sample, so they cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "kernels.hpp"

namespace rsmp {

// what RRX_finish_device was given, after validation (pointers of the device, or of the host for finish_host)
struct FinishArgs {
  const void *src;                    // frame 0 of stream 0: float (src_double = 0) or double
  void *dst;                          // null: measure only
  const double *gain;                 // [nstreams], null = unity
  double *peak;                       // [nstreams * nch], null = not taken
  unsigned long long *clipped;        // [nstreams * nch], null = not taken
  unsigned long long src_stride, dst_stride; // SAMPLES between streams
  unsigned long long n;               // samples per stream: frames * nch
  unsigned long long seed, first_frame;
  int nstreams, nch;
  int src_double;
  int bits;                           // 15 / 23 / 31: S16, packed S24, S32 (measure only: 31)
  int dither;
};

// TPDF noise of (seed, stream * nch + channel, absolute frame): a splitmix64 finaliser over a linear counter; the difference of
// the two halves of the word is triangular on (-1, 1) LSB, every step exact in fp64.
__host__ __device__ __forceinline__ double finish_dither(unsigned long long seed, unsigned long long frame, unsigned long long c)
{
  unsigned long long z = seed + frame * 0x9E3779B97F4A7C15ull + c * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return ((double)(unsigned)(z >> 32) - (double)(unsigned)z) * 0x1p-32;
}

struct FinishSample {
  double a; // |gained sample|: what the peak takes
  int q;    // the quantised sample, saturated
  bool clip;
};

// One sample.  v * gain is rounded once, on its own; g * 2^bits is exact, so whether the compiler fuses it with the addition of
// the dither or not gives the same bits, and nothing else here can be contracted (the files that include this are compiled with
// -ffp-contract=off besides).  Without dither the S16 / S32 result IS the integer handles' pcm_out16 / pcm_out32.
template <int kBits>
__host__ __device__ __forceinline__ FinishSample finish_sample(double v, bool has_gain, double gain, bool dither, unsigned long long seed,
                                                               unsigned long long frame, unsigned long long c)
{
  constexpr double scale = double(1ull << kBits), lo = -scale, hi = scale - 1.0;
  FinishSample r;
  const double g = has_gain ? v * gain : v;
  r.a = fabs(g);
  double t = g * scale;
  if (dither) t = t + finish_dither(seed, frame, c);
  const double q = rint(t);
  r.clip = !(q >= lo && q <= hi);
  if (!dither && kBits == 15) r.q = pcm_out16(g);
  else if (!dither && kBits == 31) r.q = pcm_out32(g);
  else r.q = (int)fmin(fmax(q, lo), hi);
  return r;
}

// little-endian bytes of one quantised sample at p (2, 3 or 4 of them)
template <int kBits> __host__ __device__ __forceinline__ void finish_store_bytes(unsigned char *p, int q)
{
  p[0] = (unsigned char)q;
  p[1] = (unsigned char)(q >> 8);
  if (kBits > 15) p[2] = (unsigned char)(q >> 16);
  if (kBits > 23) p[3] = (unsigned char)(q >> 24);
}

// Channels up to here keep their statistics in registers and LDS and issue one global atomic per (workgroup, channel, statistic);
// above it (or when lcm(4, nch) exceeds the 1024 samples a workgroup takes per step) the kernel's atomics go straight to global memory.
constexpr int kFinishLdsChannels = 1024;

// Only enqueues on `stream`, split into as many launches as the grid limits ask for; the arguments are the caller's to validate.
hipError_t launch_finish(hipStream_t stream, const FinishArgs &a);
// The same results on host pointers, as one serial loop over finish_sample (test hook: RRX_debug_finish_host).
void finish_host(const FinishArgs &a);

} // namespace rsmp
