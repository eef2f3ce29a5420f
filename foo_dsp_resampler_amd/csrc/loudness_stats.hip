// Block powers, the gate over groups of streams and the gated percentiles of the loudness meter ("Loudness meter").
// The arithmetic is loudness_stats.hpp's; this file is the lane layout around it.
//
//   blocks        one lane per (stream, block); the maximum is reduced per wave, per workgroup and then with one integer atomic
//                 maximum per workgroup on the bit pattern, which for the non-negative doubles it sees is the order of the values
//   gate, stream  one wave per stream: 64 blocks at a time, one per lane; the ones that pass are added up ascending, each read from
//                 its lane's register, once per gate stage; sum and count land in `work`
//   gate, group   one wave per group: it walks the streams ascending, 64 at a time, and adds the members' results in that order;
//                 after the first stage it leaves T in `work`
//   range         one workgroup per group: a radix select, most significant byte first, on the bit patterns of the blocks that
//                 pass both gates.  Every pass walks the group's streams, 256 at a time with their blocks as one pool for the
//                 lanes, and counts the next byte of the candidates of both ranks in LDS with integer atomics; a scan of the 256
//                 counts picks each rank's byte.  Eight passes, no sort, no buffer that grows with the block count.
// Nothing but blocks, nblocks, max, work and result is written.
#include "loudness_stats.hpp"

#include <algorithm>
#include <vector>

namespace rsmp {
namespace {

constexpr int kThreads = 256, kWave = 64, kWaves = kThreads / kWave;
constexpr unsigned kMaxGridX = 1u << 22;  // workgroups of 256 lanes in x: x * 256 stays under 2^32
constexpr int kMaxGridY = 32768;          // grid.y is a 16-bit count

__device__ __forceinline__ unsigned long long *work_counts(const LoudnessGroupsArgs &a)
{
  return reinterpret_cast<unsigned long long *>(a.work);
}

__global__ __launch_bounds__(kThreads) void loudness_blocks_kernel(LoudnessBlocksArgs a, int s0)
{
  __shared__ double wave_max[kWaves];
  const unsigned tid = threadIdx.x;
  const unsigned long long s = (unsigned long long)(s0 + (int)blockIdx.y);
  const unsigned long long nb = loudness_stats_count(a, s);
  const double *e = a.energy + s * (unsigned long long)a.nch * a.energy_stride;
  double m = 0.0;
  for (unsigned long long j = (unsigned long long)blockIdx.x * kThreads + tid; j < nb; j += (unsigned long long)gridDim.x * kThreads) {
    const double z = loudness_stats_block(a, e, j);
    if (a.blocks) a.blocks[s * a.blocks_stride + j] = z;
    m = loudness_stats_max(m, z);
  }
  if (a.nblocks && blockIdx.x == 0 && tid == 0) a.nblocks[s] = nb;
  if (!a.max) return;
  for (int off = kWave / 2; off; off >>= 1) m = loudness_stats_max(m, __shfl_xor(m, off));
  if ((tid & (kWave - 1)) == 0) wave_max[tid / kWave] = m;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kWaves; ++w) m = loudness_stats_max(m, wave_max[w]);
    // m is +0.0 or a positive double (+inf included), never a NaN: the unsigned order of the bits is the order of the values,
    // and the row was zeroed (+0.0) on the stream in front of this launch
    if (m > 0.0) atomicMax(reinterpret_cast<unsigned long long *>(a.max) + s, (unsigned long long)__double_as_longlong(m));
  }
}

// lane b's value in every lane; b is the same in every lane
__device__ __forceinline__ unsigned long long read_lane(unsigned long long x, int b)
{
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(x & 0xffffffffull), b);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(x >> 32), b);
  return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ double read_lane(double v, int b)
{
  return __longlong_as_double((long long)read_lane((unsigned long long)__double_as_longlong(v), b));
}

// stage 0: S1_s, N1_s; stage 1: S2_s, N2_s with the group's T.  A stream in no group is left out.  64 blocks at a time, one per
// lane, with the next 64 in flight; the lanes that pass are a mask, and the sum walks its bits from the lowest -- ascending j --
// in every lane alike.
__global__ __launch_bounds__(kWave) void loudness_groups_stream_kernel(LoudnessGroupsArgs a, int s0, int stage)
{
  const unsigned lane = threadIdx.x;
  const unsigned long long s = (unsigned long long)s0 + blockIdx.x;
  int g;
  if (!loudness_groups_member(a, s, g)) return;
  const unsigned long long nb = loudness_groups_count(a, s);
  const double *p = a.blocks + s * a.blocks_stride;
  const double t = stage ? a.work[2ull * (unsigned long long)a.nstreams + (unsigned long long)g] : 0.0;
  double sum = 0.0;
  unsigned long long count = 0;
  double next = lane < nb ? p[lane] : 0.0;
  for (unsigned long long j0 = 0; j0 < nb; j0 += kWave) {
    const double v = next;
    const bool have = j0 + lane < nb;
    const unsigned long long j1 = j0 + kWave + lane;
    next = j1 < nb ? p[j1] : 0.0;
    unsigned long long mask = __ballot(have && loudness_groups_passes(a, v, stage != 0, t));
    count += (unsigned long long)__popcll(mask);
    while (mask) {
      const int b = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      sum = sum + read_lane(v, b);
    }
  }
  if (lane == 0) {
    a.work[2 * s] = sum;
    work_counts(a)[2 * s + 1] = count;
  }
}

// one wave per group: the members' sums and counts, streams ascending
__global__ __launch_bounds__(kWave) void loudness_groups_sum_kernel(LoudnessGroupsArgs a, int g0, int stage)
{
  const unsigned lane = threadIdx.x;
  const int g = g0 + (int)blockIdx.x;
  const unsigned long long ns = (unsigned long long)a.nstreams;
  double sum = 0.0;
  unsigned long long count = 0;
  for (unsigned long long s0 = 0; s0 < ns; s0 += kWave) {
    const unsigned long long s = s0 + lane;
    const bool in = s < ns && a.group[s] == g;
    const double v = in ? a.work[2 * s] : 0.0;
    const unsigned long long c = in ? work_counts(a)[2 * s + 1] : 0ull;
    unsigned long long mask = __ballot(in);
    while (mask) { // the same for every lane: every lane holds the group's sums
      const int b = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      sum = sum + read_lane(v, b);
      count += read_lane(c, b);
    }
  }
  if (lane == 0) {
    double *out = a.result + (unsigned long long)g * 4 + (stage ? 0 : 2);
    out[0] = sum;
    out[1] = (double)count;
    if (!stage) a.work[2 * ns + (unsigned long long)g] = loudness_groups_threshold(a, sum, count);
  }
}

// one count of `digit` per lane with `on`; the lanes that share the first such lane's digit -- in the leading passes, and in a
// multiset of duplicates, nearly all of them -- go in as one addition.  Integer counts do not depend on the order of arrival.
__device__ __forceinline__ void count_digit(unsigned long long *hist, bool on, unsigned digit, unsigned lane)
{
  const unsigned long long mask = __ballot(on);
  if (!mask) return;
  const int leader = __ffsll((long long)mask) - 1;
  const unsigned first = (unsigned)__builtin_amdgcn_readlane((int)digit, leader);
  const unsigned long long peers = __ballot(on && digit == first);
  if (lane == (unsigned)leader) atomicAdd(&hist[first], (unsigned long long)__popcll(peers));
  if (on && digit != first) atomicAdd(&hist[digit], 1ull);
}

// inclusive sum of one count per lane over the workgroup's 256 lanes, and their total; the caller keeps a barrier between two
// uses of one `wave_total`
__device__ __forceinline__ unsigned long long scan_counts(unsigned long long c, unsigned long long *wave_total, unsigned lane, unsigned wave,
                                                          unsigned long long &total)
{
  unsigned long long incl = c;
  for (int off = 1; off < kWave; off <<= 1) {
    const unsigned long long up = __shfl_up(incl, off);
    if (lane >= (unsigned)off) incl += up;
  }
  if (lane == kWave - 1) wave_total[wave] = incl;
  __syncthreads();
  total = 0;
  for (unsigned w = 0; w < (unsigned)kWaves; ++w) {
    if (w < wave) incl += wave_total[w];
    total += wave_total[w];
  }
  return incl;
}

__global__ __launch_bounds__(kThreads) void loudness_range_kernel(LoudnessGroupsArgs a, int g0)
{
  __shared__ unsigned long long hist[2][256];
  __shared__ unsigned long long wave_total[3][kWaves];
  __shared__ unsigned long long picked_prefix[2], picked_rank[2];
  __shared__ unsigned long long first_block[kThreads]; // of the chunk's members: where each one's blocks begin in the chunk's pool
  __shared__ unsigned member[kThreads];
  __shared__ unsigned member_count;
  const unsigned tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int g = g0 + (int)blockIdx.x;
  const unsigned long long ns = (unsigned long long)a.nstreams;
  const double t = a.work[2 * ns + (unsigned long long)g];
  const int pct[2] = {a.pct_low, a.pct_high};
  unsigned long long prefix[2] = {0, 0}, rank[2] = {0, 0}, n = 0;

  for (int pass = 0; pass < 8; ++pass) {
    const bool one = prefix[0] == prefix[1]; // both ranks still look among the same candidates: one histogram serves both
    hist[0][tid] = 0;
    hist[1][tid] = 0;
    // the streams in chunks of 256: the chunk's members (in any order: integer counts do not depend on it), then their blocks
    // as ONE pool that the lanes stride over, so that a group of many short streams keeps every lane busy
    for (unsigned long long s0 = 0; s0 < ns; s0 += kThreads) {
      __syncthreads(); // the zeroed counts; the member list of the chunk before is no longer read
      if (tid == 0) member_count = 0;
      __syncthreads();
      if (s0 + tid < ns && a.group[s0 + tid] == g) member[atomicAdd(&member_count, 1u)] = tid;
      __syncthreads();
      const unsigned members = member_count;
      const unsigned long long mine = tid < members ? loudness_groups_count(a, s0 + member[tid]) : 0ull;
      unsigned long long pool;
      const unsigned long long incl = scan_counts(mine, wave_total[2], lane, wave, pool);
      first_block[tid] = incl - mine;
      __syncthreads();
      // block i of the pool: the member `at` with first_block[at] <= i < first_block[at + 1] (first_block[members] = pool; among
      // members with one first_block the last one holds the blocks, the others have none).  A lane's i only grows, so the search
      // begins at the member it found last: a long stream costs one look at its successor, and only a step beyond that a bisection.
      unsigned at = 0;
      auto locate = [&](unsigned long long i) -> unsigned long long { // where block i lies in a.blocks; behind the pool: 0, not used
        if (i >= pool) return 0ull;
        if (at + 1 < members && first_block[at + 1] <= i) {
          unsigned lo = at + 1, hi = members;
          while (hi - lo > 1) {
            const unsigned mid = (lo + hi) / 2;
            if (first_block[mid] <= i) lo = mid;
            else hi = mid;
          }
          at = lo;
        }
        return (s0 + member[at]) * a.blocks_stride + (i - first_block[at]);
      };
      for (unsigned long long i0 = 0; i0 < pool; i0 += kThreads) { // the same trips for every lane
        const bool have = i0 + tid < pool;
        const double z = a.blocks[locate(i0 + tid)];
        const bool on = have && loudness_groups_passes(a, z, true, t);
        const unsigned long long bits = (unsigned long long)__double_as_longlong(z);
        const unsigned long long head = pass ? bits >> (64 - 8 * pass) : 0ull;
        const unsigned digit = (unsigned)(bits >> (56 - 8 * pass)) & 255u;
        count_digit(hist[0], on && head == prefix[0], digit, lane);
        if (!one) count_digit(hist[1], on && head == prefix[1], digit, lane);
      }
    }
    __syncthreads();
    for (int r = 0; r < 2; ++r) {
      const unsigned long long c = hist[one ? 0 : r][tid];
      unsigned long long total;
      const unsigned long long incl = scan_counts(c, wave_total[r], lane, wave, total);
      if (pass == 0) {
        n = total; // every block of the group that passes both gates: N2
        rank[r] = n ? loudness_groups_rank(n, pct[r]) : 0;
      }
      if (c && incl - c <= rank[r] && rank[r] < incl) { // one lane, when there is any candidate
        picked_prefix[r] = (prefix[r] << 8) | tid;
        picked_rank[r] = rank[r] - (incl - c);
      }
    }
    if (!n) break; // (the same for every lane)
    __syncthreads();
    for (int r = 0; r < 2; ++r) {
      prefix[r] = picked_prefix[r];
      rank[r] = picked_rank[r];
    }
  }
  if (tid == 0) {
    double *out = a.result + (unsigned long long)g * 4;
    out[0] = n ? __longlong_as_double((long long)prefix[0]) : 0.0;
    out[1] = n ? __longlong_as_double((long long)prefix[1]) : 0.0;
    out[2] = (double)n;
    out[3] = t;
  }
}

hipError_t launch_streams(hipStream_t stream, const LoudnessGroupsArgs &a, int stage)
{
  for (int s0 = 0; s0 < a.nstreams;) {
    const unsigned ns = (unsigned)(a.nstreams - s0) < kMaxGridX ? (unsigned)(a.nstreams - s0) : kMaxGridX;
    hipLaunchKernelGGL(loudness_groups_stream_kernel, dim3(ns), dim3(kWave), 0, stream, a, s0, stage);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    s0 += (int)ns;
  }
  return hipSuccess;
}

hipError_t launch_sums(hipStream_t stream, const LoudnessGroupsArgs &a, int stage)
{
  for (int g0 = 0; g0 < a.ngroups;) {
    const unsigned ng = (unsigned)(a.ngroups - g0) < kMaxGridX ? (unsigned)(a.ngroups - g0) : kMaxGridX;
    hipLaunchKernelGGL(loudness_groups_sum_kernel, dim3(ng), dim3(kWave), 0, stream, a, g0, stage);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    g0 += (int)ng;
  }
  return hipSuccess;
}

} // namespace

hipError_t launch_loudness_blocks(hipStream_t stream, const LoudnessBlocksArgs &a)
{
  if (a.max) { // +0.0: "no block"
    const hipError_t e = hipMemsetAsync(a.max, 0, (size_t)a.nstreams * sizeof(double), stream);
    if (e != hipSuccess) return e;
  }
  unsigned long long most = a.nhops < a.block_hops ? 0 : (a.nhops - a.block_hops) / a.step_hops + 1; // what the longest stream can have
  if (a.blocks && most > a.blocks_stride) most = a.blocks_stride;
  const unsigned long long groups = (most + kThreads - 1) / kThreads;
  const unsigned gx = groups > kMaxGridX ? kMaxGridX : groups ? (unsigned)groups : 1u; // one workgroup at least: nblocks and max are written
  for (int s0 = 0; s0 < a.nstreams; s0 += kMaxGridY) {
    const int ns = a.nstreams - s0 < kMaxGridY ? a.nstreams - s0 : kMaxGridY;
    hipLaunchKernelGGL(loudness_blocks_kernel, dim3(gx, (unsigned)ns), dim3(kThreads), 0, stream, a, s0);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_loudness_gate_groups(hipStream_t stream, const LoudnessGroupsArgs &a)
{
  for (int stage = 0; stage < 2; ++stage) {
    hipError_t e = launch_streams(stream, a, stage);
    if (e != hipSuccess) return e;
    e = launch_sums(stream, a, stage);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_loudness_range_groups(hipStream_t stream, const LoudnessGroupsArgs &a)
{
  // stage 0 alone, for T; its S1 and N1 land in the result rows, which the selection then writes in full
  hipError_t e = launch_streams(stream, a, 0);
  if (e != hipSuccess) return e;
  e = launch_sums(stream, a, 0);
  if (e != hipSuccess) return e;
  for (int g0 = 0; g0 < a.ngroups;) {
    const unsigned ng = (unsigned)(a.ngroups - g0) < kMaxGridX ? (unsigned)(a.ngroups - g0) : kMaxGridX;
    hipLaunchKernelGGL(loudness_range_kernel, dim3(ng), dim3(kThreads), 0, stream, a, g0);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    g0 += (int)ng;
  }
  return hipSuccess;
}

void loudness_blocks_host(const LoudnessBlocksArgs &a)
{
  for (unsigned long long s = 0; s < (unsigned long long)a.nstreams; ++s) {
    const unsigned long long nb = loudness_stats_count(a, s);
    const double *e = a.energy + s * (unsigned long long)a.nch * a.energy_stride;
    double m = 0.0;
    for (unsigned long long j = 0; j < nb; ++j) {
      const double z = loudness_stats_block(a, e, j);
      if (a.blocks) a.blocks[s * a.blocks_stride + j] = z;
      m = loudness_stats_max(m, z);
    }
    if (a.nblocks) a.nblocks[s] = nb;
    if (a.max) a.max[s] = m;
  }
}

namespace {

// stage 0 or 1 of the gate on the host: per stream from +0.0 and 0, then per group over the member streams ascending
void groups_stage_host(const LoudnessGroupsArgs &a, int stage, double *sums, unsigned long long *counts)
{
  const unsigned long long ns = (unsigned long long)a.nstreams;
  double *t = a.work + 2 * ns;
  for (int g = 0; g < a.ngroups; ++g) {
    sums[g] = 0.0;
    counts[g] = 0;
  }
  for (unsigned long long s = 0; s < ns; ++s) {
    int g;
    if (!loudness_groups_member(a, s, g)) continue;
    const unsigned long long nb = loudness_groups_count(a, s);
    const double tg = stage ? t[g] : 0.0;
    double sum = 0.0;
    unsigned long long count = 0;
    for (unsigned long long j = 0; j < nb; ++j) {
      const double v = a.blocks[s * a.blocks_stride + j];
      if (loudness_groups_passes(a, v, stage != 0, tg)) {
        sum = sum + v;
        ++count;
      }
    }
    sums[g] = sums[g] + sum;
    counts[g] += count;
  }
  if (!stage)
    for (int g = 0; g < a.ngroups; ++g) t[g] = loudness_groups_threshold(a, sums[g], counts[g]);
}

} // namespace

void loudness_gate_groups_host(const LoudnessGroupsArgs &a)
{
  std::vector<double> sums((size_t)a.ngroups);
  std::vector<unsigned long long> counts((size_t)a.ngroups);
  for (int stage = 0; stage < 2; ++stage) {
    groups_stage_host(a, stage, sums.data(), counts.data());
    for (int g = 0; g < a.ngroups; ++g) {
      double *out = a.result + (size_t)g * 4 + (stage ? 0 : 2);
      out[0] = sums[(size_t)g];
      out[1] = (double)counts[(size_t)g];
    }
  }
}

void loudness_range_groups_host(const LoudnessGroupsArgs &a)
{
  const unsigned long long ns = (unsigned long long)a.nstreams;
  std::vector<double> sums((size_t)a.ngroups);
  std::vector<unsigned long long> counts((size_t)a.ngroups);
  groups_stage_host(a, 0, sums.data(), counts.data());
  const double *t = a.work + 2 * ns;
  std::vector<double> pool;
  for (int g = 0; g < a.ngroups; ++g) {
    pool.clear();
    for (unsigned long long s = 0; s < ns; ++s) {
      int sg;
      if (!loudness_groups_member(a, s, sg) || sg != g) continue;
      const unsigned long long nb = loudness_groups_count(a, s);
      for (unsigned long long j = 0; j < nb; ++j) {
        const double v = a.blocks[s * a.blocks_stride + j];
        if (loudness_groups_passes(a, v, true, t[g])) pool.push_back(v);
      }
    }
    std::sort(pool.begin(), pool.end());
    const unsigned long long n = pool.size();
    double *out = a.result + (size_t)g * 4;
    out[0] = n ? pool[(size_t)loudness_groups_rank(n, a.pct_low)] : 0.0;
    out[1] = n ? pool[(size_t)loudness_groups_rank(n, a.pct_high)] : 0.0;
    out[2] = (double)n;
    out[3] = t[g];
  }
}

} // namespace rsmp
