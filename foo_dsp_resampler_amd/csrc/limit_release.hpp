// Exponential release for the true-peak limiter ("Limiter: release"): between the window minimum and the box of
// RRX_limit_device a one-pole recursion towards the target, p = fmin(v, a * p + b * v), b = 1 - a.  One step is the map
// x -> min(t, a * x + u), and such maps are closed under composition:
//   min(t2, a2 * min(t1, a1 * x + u1) + u2) = min(min(t2, a2 * t1 + u2), a2 * a1 * x + (a2 * u1 + u2))
// so a block of entries collapses into three numbers (C, A, B): x -> fmin(C, A * x + B).  Every block is summarised from nothing,
// a serial carry over the summaries gives every block's start state, and every block is run again from it.  The block
// decomposition is the ABI of RRX_limit_release_device (include/ratelib_amd.h): fp64, every operation rounded on its own, no
// fused multiply-add.  The kernels (limit_release.hip) and the host twin behind RRX_debug_limit_release_host are both loops
// around the functions below, so they cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>

#include "limit.hpp"

namespace rsmp {

constexpr int kLimitReleaseMinBlock = 64, kLimitReleaseMaxBlock = 65536;

// the summary of a block's first entry v_0
__host__ __device__ __forceinline__ void limit_release_first(double v, double a, double b, double &C, double &A, double &B)
{
  C = v;
  A = a;
  B = b * v;
}

// the summary after one more entry v_t, t >= 1
__host__ __device__ __forceinline__ void limit_release_extend(double v, double a, double b, double &C, double &A, double &B)
{
  const double u = b * v;
  C = fmin(v, a * C + u);
  A = a * A;
  B = a * B + u;
}

// S_{i+1} from S_i and the summary of block i
__host__ __device__ __forceinline__ double limit_release_carry(double C, double A, double B, double S) { return fmin(C, A * S + B); }

// q of one entry v from the state p in front of it
__host__ __device__ __forceinline__ double limit_release_step(double v, double a, double b, double p)
{
  const double u = b * v;
  return fmin(v, a * p + u);
}

// blocks of a row with J entries
__host__ __device__ __forceinline__ unsigned long long limit_release_blocks(unsigned long long J, unsigned block)
{
  return (J + block - 1) / block;
}

// What the three launches between the window minimum and the product take.  Stream s owns work[s * stream_stride ...): m[j] at
// m_off, j in [0, J), J = N + lookahead - 1 for a row of N > 0 frames (0 for an empty one); C and A at c_off and c_off +
// sum_stride, B and S at b_off and b_off + sum_stride, sum_stride >= blocks of the longest row + 1.
struct LimitReleaseArgs {
  double *work;
  const Track *tracks;             // null: every row has `frames` frames; else stream t is track t's slice (tracks_slice) of row t
  unsigned long long frames;       // per stream (tracks: the rows' length)
  unsigned long long stream_stride, m_off, c_off, b_off, sum_stride;
  unsigned lookahead, block;
  double a, b;                     // the pole and 1.0 - a
  int nstreams;
};

// The whole call: limit.hip's detector and window minimum (launch_limit_passes), summary, carry, run, limit.hip's product.  `la`
// is the limiter's arguments with work_stride = half a stream's share of the work buffer, so that r lies at its start and m at
// `r.m_off` = la.work_stride.  Only enqueues.
hipError_t launch_limit_release(hipStream_t stream, const LimitArgs &la, const LimitReleaseArgs &r);
// the same on host pointers, as serial loops over the functions above and limit_host's (test hook: RRX_debug_limit_release_host)
void limit_release_host(const LimitArgs &la, const LimitReleaseArgs &r);

} // namespace rsmp
