// The loudness meter on top of the hop energies of loudness.hpp ("Loudness meter"): sliding block powers of any length
// and step with their maximum (momentary, short-term), the BS.1770 gate over the pooled blocks of GROUPS of streams (an album), and
// gated percentiles by exact selection (loudness range, EBU Tech 3342).  As in loudness.hpp the per-element arithmetic is in the
// functions below, and both the kernels (loudness_stats.hip) and the host twins behind RRX_debug_loudness_blocks_host /
// RRX_debug_loudness_gate_groups_host / RRX_debug_loudness_range_groups_host are loops around them.  The files that include this are
// compiled with -ffp-contract=off.
//
// With block_hops = 4 and step_hops = 1, loudness_stats_block has the bits of loudness.hpp's loudness_block: the same ascending
// sums per channel, the same ascending weighted sum over the channels, and inv = 1 / (4 hop).  A group of exactly one stream over
// those blocks has the bits of RRX_loudness_gate_device on that stream: the group's sums are +0.0 + x, which is x for the
// non-negative sums of the streams.  Streams run in parallel and only the per-group sums over the streams' results are serial, so
// a whole library in one group costs its longest stream's serial walk, not the library's.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

namespace rsmp {

// What RRX_loudness_blocks_device was given, after validation (pointers of the device, or of the host for the twin)
struct LoudnessBlocksArgs {
  const double *energy;            // channel c's hops at energy + c * energy_stride
  const unsigned long long *hops;  // [nstreams] or null: nhops for all
  const double *weights;           // [nch] or null: 1.0
  double *blocks;                  // [nstreams][blocks_stride] or null
  unsigned long long *nblocks;     // [nstreams] or null
  double *max;                     // [nstreams] or null
  unsigned long long energy_stride, nhops, blocks_stride;
  unsigned long long block_hops, step_hops; // L, P
  int nstreams, nch;
  double inv;                      // 1 / (L hop)
};

// the hops stream s has, and the blocks they give: 0 below L hops, else (n - L) / P + 1, clamped to the rows of `blocks`
__host__ __device__ __forceinline__ unsigned long long loudness_stats_count(const LoudnessBlocksArgs &a, unsigned long long s)
{
  unsigned long long n = a.nhops;
  if (a.hops && a.hops[s] < n) n = a.hops[s];
  unsigned long long nb = n < a.block_hops ? 0 : (n - a.block_hops) / a.step_hops + 1;
  if (a.blocks && nb > a.blocks_stride) nb = a.blocks_stride;
  return nb;
}

// z_j of one stream: e = the stream's channel 0, hop 0.  Block j begins at hop j P (j P + L <= nhops <= energy_stride).
__host__ __device__ __forceinline__ double loudness_stats_block(const LoudnessBlocksArgs &a, const double *e, unsigned long long j)
{
  double acc = 0.0;
  for (int ch = 0; ch < a.nch; ++ch) {
    const double *p = e + (unsigned long long)ch * a.energy_stride + j * a.step_hops;
    double q = p[0];
    for (unsigned long long i = 1; i < a.block_hops; ++i) q = q + p[i];
    acc = a.weights ? acc + a.weights[ch] * q : acc + q;
  }
  return acc * a.inv;
}

// the maximum's step: a NaN fails the comparison and is skipped; from +0.0 the result does not depend on the order
__host__ __device__ __forceinline__ double loudness_stats_max(double m, double z) { return z > m ? z : m; }

// What RRX_loudness_gate_groups_device / RRX_loudness_range_groups_device were given, after validation
struct LoudnessGroupsArgs {
  const double *blocks;               // [nstreams][blocks_stride]
  const unsigned long long *nblocks;  // [nstreams], read clamped to blocks_stride
  const int *group;                   // [nstreams]: stream s's group; outside [0, ngroups): in no group
  double *result;                     // [ngroups][4]
  double *work;                       // loudness_groups_work_doubles(...): see loudness_groups_*_at
  unsigned long long blocks_stride;
  int nstreams, ngroups;
  int pct_low, pct_high;              // the range call only
  double abs_threshold, rel_factor;
};

// work: per stream its sum and its count (the count as an unsigned 64-bit integer in the double's place), then T per group
inline unsigned long long loudness_groups_work_doubles(unsigned long long nstreams, unsigned long long ngroups)
{
  return 2ull * nstreams + ngroups;
}

__host__ __device__ __forceinline__ bool loudness_groups_member(const LoudnessGroupsArgs &a, unsigned long long s, int &g)
{
  g = a.group[s];
  return g >= 0 && g < a.ngroups;
}

__host__ __device__ __forceinline__ unsigned long long loudness_groups_count(const LoudnessGroupsArgs &a, unsigned long long s)
{
  const unsigned long long nb = a.nblocks[s];
  return nb < a.blocks_stride ? nb : a.blocks_stride;
}

// does block z count?  relative = false: the absolute gate alone; true: both gates, with the group's T
__host__ __device__ __forceinline__ bool loudness_groups_passes(const LoudnessGroupsArgs &a, double z, bool relative, double t)
{
  return z > a.abs_threshold && (!relative || z > t);
}

// T = rel_factor * (S1 / N1), the division correctly rounded; NaN for an empty group, which then passes nothing
__host__ __device__ __forceinline__ double loudness_groups_threshold(const LoudnessGroupsArgs &a, double s1, unsigned long long n1)
{
  return a.rel_factor * (s1 / (double)n1);
}

// 0-based index of percentile pct among n >= 1 sorted values: Tech 3342's round((n - 1) pct / 100 + 1), 1-based
__host__ __device__ __forceinline__ unsigned long long loudness_groups_rank(unsigned long long n, int pct)
{
  return ((n - 1) * (unsigned long long)pct + 50ull) / 100ull;
}

// All three only enqueue on `stream`, split into as many launches as the grid limits ask for; the arguments are the caller's to
// validate.  d_group and d_nblocks cannot be: the kernels take a group outside [0, ngroups) as "in no group" and clamp the counts.
hipError_t launch_loudness_blocks(hipStream_t stream, const LoudnessBlocksArgs &a);
hipError_t launch_loudness_gate_groups(hipStream_t stream, const LoudnessGroupsArgs &a);
hipError_t launch_loudness_range_groups(hipStream_t stream, const LoudnessGroupsArgs &a);
// The calls' results on host pointers, as serial loops over the functions above (test hooks); the range twin sorts.
void loudness_blocks_host(const LoudnessBlocksArgs &a);
void loudness_gate_groups_host(const LoudnessGroupsArgs &a);
void loudness_range_groups_host(const LoudnessGroupsArgs &a);

} // namespace rsmp
