// The limiter's release ("Limiter: release"): RRX_limit_release_device and RRX_tracks_limit_release_device.  The
// arithmetic is limit_release.hpp's, shared with the host twin at the end of this file; the detector, the window minimum and the
// product are limit.hip's own launches, untouched.  Between the window minimum and the product, three launches on the entries
// m[j], j in [0, J), of every row, in blocks of `block` entries:
//   summary  one lane per (stream, block), 256 to a workgroup, grid = (pieces of the longest row, stream): (C, A, B) of the block
//            from nothing.
//   carry    one wave per stream, blocks ascending: S_0 = 1.0, S_{i+1} = fmin(C_i, A_i * S_i + B_i).  The wave loads the
//            summaries of 64 blocks at a time, a lane each, and hands them round through LDS; every lane runs the one serial
//            chain, and lane u keeps S_{i+u+1} for the store.  (One lane per stream with its own loads waited a memory latency
//            for every eight blocks and took more than the summary: DESIGN.md 10.)
//   run      the summary's lanes again: q over m in place, from S_i.
// A lane's block lies `block` doubles from its neighbour's, so a lane that loaded its own entries would share no cache line with
// its neighbours.  A workgroup therefore stages a tile of kTile entries of each of its 256 blocks through LDS: sixteen
// consecutive threads load one block's 128 bytes, sixteen blocks a thread, the next tile's loads issued before this tile is
// computed; a lane then reads its own kTile entries from LDS (rows kTile + 1 doubles apart), and the run hands q back the same
// way.  Against register tiles loaded by the lane itself -- the form loudness.hip prefers for its interleaved frames -- this
// takes 25 % less time for the three launches at block 1024 and less at every other block length.  The dependent
// chain per entry is a multiply, an add and a minimum.
#include "limit_release.hpp"

namespace rsmp {
namespace {

constexpr int kThreads = 256, kTile = 16, kPitch = kTile + 1, kSubs = kThreads / kTile;
constexpr int kCarryThreads = 64; // one wave: the carry's workgroup

struct Entries {
  double *m, *C, *A, *B, *S;
  unsigned long long J, nb;
};

__host__ __device__ __forceinline__ Entries entries_of(const LimitReleaseArgs &a, unsigned long long s)
{
  Entries e;
  const unsigned long long n = a.tracks ? tracks_slice(a.tracks[s], a.frames, 0, false).frames : a.frames;
  double *base = a.work + s * a.stream_stride;
  e.m = base + a.m_off;
  e.C = base + a.c_off;
  e.A = e.C + a.sum_stride;
  e.B = base + a.b_off;
  e.S = e.B + a.sum_stride;
  e.J = n ? n + (a.lookahead - 1) : 0;
  e.nb = limit_release_blocks(e.J, a.block);
  return e;
}

// kRun = false: the summary; true: the run.  Thread tid is lane tid of the workgroup's 256 blocks, and loads entry tt of the
// tiles of the blocks sub, sub + 16, ... (at).
template <bool kRun> __global__ __launch_bounds__(kThreads) void limit_release_pass_kernel(LimitReleaseArgs a, int s0)
{
  __shared__ double tile[kThreads * kPitch];
  const Entries e = entries_of(a, (unsigned long long)(s0 + (int)blockIdx.y));
  const unsigned block = a.block, tid = threadIdx.x, sub = tid / kTile, tt = tid % kTile;
  const double pole = a.a, b = a.b;
  for (unsigned long long g0 = (unsigned long long)blockIdx.x * kThreads; g0 < e.nb; g0 += (unsigned long long)gridDim.x * kThreads) {
    const unsigned long long i = g0 + tid;
    const unsigned n = i < e.nb ? (e.J - i * block < block ? (unsigned)(e.J - i * block) : block) : 0;
    double r[kTile];
    auto at = [&](int k, unsigned t0, unsigned long long &j) {
      const unsigned long long blk = g0 + sub + (unsigned)k * kSubs;
      j = blk * block + t0 + tt;
      return blk < e.nb && t0 + tt < block && j < e.J;
    };
    auto gload = [&](unsigned t0) {
#pragma unroll
      for (int k = 0; k < kTile; ++k) {
        unsigned long long j;
        r[k] = at(k, t0, j) ? e.m[j] : 1.0;
      }
    };
    auto put = [&]() {
#pragma unroll
      for (int k = 0; k < kTile; ++k) tile[(sub + (unsigned)k * kSubs) * kPitch + tt] = r[k];
    };
    gload(0);
    __syncthreads(); // the readers of the tile before are done
    put();
    __syncthreads();
    double C = 1.0, A = 1.0, B = 0.0, st = (kRun && n) ? e.S[i] : 0.0;
    for (unsigned t0 = 0; t0 < block; t0 += kTile) {
      if (t0 + kTile < block) gload(t0 + kTile); // in flight while this tile is computed; loaded before the run stores over anything
#pragma unroll
      for (int t = 0; t < kTile; ++t)
        if (t0 + t < n) {
          const double v = tile[tid * kPitch + t];
          if (kRun) {
            st = limit_release_step(v, pole, b, st);
            tile[tid * kPitch + t] = st;
          } else if (t0 + t == 0) limit_release_first(v, pole, b, C, A, B);
          else limit_release_extend(v, pole, b, C, A, B);
        }
      __syncthreads(); // every lane is done with its row of the tile
      if (kRun) { // q of this tile, as it was loaded: 128 bytes of a block to sixteen threads
#pragma unroll
        for (int k = 0; k < kTile; ++k) {
          unsigned long long j;
          if (at(k, t0, j)) e.m[j] = tile[(sub + (unsigned)k * kSubs) * kPitch + tt];
        }
        __syncthreads();
      }
      put(); // the next tile (behind the last one: what r still holds, which nobody reads)
      __syncthreads();
    }
    if (!kRun && n) {
      e.C[i] = C;
      e.A[i] = A;
      e.B[i] = B;
    }
  }
}

__global__ __launch_bounds__(kCarryThreads) void limit_release_carry_kernel(LimitReleaseArgs a)
{
  __shared__ double sh[3][kCarryThreads];
  const unsigned lane = threadIdx.x;
  for (unsigned long long s = blockIdx.x; s < (unsigned long long)a.nstreams; s += gridDim.x) { // (the whole wave)
    const Entries e = entries_of(a, s);
    if (!e.nb) continue;
    double S = 1.0, C = 1.0, A = 1.0, B = 0.0;
    if (!lane) e.S[0] = S;
    auto fetch = [&](unsigned long long i) {
      if (i + lane < e.nb) {
        C = e.C[i + lane];
        A = e.A[i + lane];
        B = e.B[i + lane];
      }
    };
    fetch(0);
    for (unsigned long long i = 0; i < e.nb; i += kCarryThreads) {
      __syncthreads(); // the readers of the batch before are done
      sh[0][lane] = C;
      sh[1][lane] = A;
      sh[2][lane] = B;
      __syncthreads();
      if (i + kCarryThreads < e.nb) fetch(i + kCarryThreads); // in flight while this batch is carried
      const unsigned n = e.nb - i < (unsigned long long)kCarryThreads ? (unsigned)(e.nb - i) : (unsigned)kCarryThreads;
      double mine = 0.0;
      for (unsigned u = 0; u < n; ++u) { // every lane the same chain
        S = limit_release_carry(sh[0][u], sh[1][u], sh[2][u], S);
        mine = u == lane ? S : mine;
      }
      if (lane < n) e.S[i + lane + 1] = mine;
    }
  }
}

hipError_t launch_release(hipStream_t stream, const LimitReleaseArgs &a)
{
  // lanes of the longest row: frames + lookahead - 1 < 2^60 + 2^10 entries, block >= 64
  const unsigned long long nb = limit_release_blocks(a.frames + (a.lookahead - 1), a.block), groups = (nb + kThreads - 1) / kThreads;
  const unsigned gx = groups > 0x7fffffffull ? 0x7fffffffu : (unsigned)groups;
  for (int pass = 0; pass < 3; ++pass) {
    if (pass == 1) {
      hipLaunchKernelGGL(limit_release_carry_kernel, dim3((unsigned)a.nstreams), dim3(kCarryThreads), 0, stream, a);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
      continue;
    }
    for (int s0 = 0; s0 < a.nstreams; s0 += 32768) { // grid.y is a 16-bit count
      const int ns = a.nstreams - s0 < 32768 ? a.nstreams - s0 : 32768;
      if (pass == 0) hipLaunchKernelGGL(limit_release_pass_kernel<false>, dim3(gx, (unsigned)ns), dim3(kThreads), 0, stream, a, s0);
      else hipLaunchKernelGGL(limit_release_pass_kernel<true>, dim3(gx, (unsigned)ns), dim3(kThreads), 0, stream, a, s0);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
    }
  }
  return hipSuccess;
}

} // namespace

hipError_t launch_limit_release(hipStream_t stream, const LimitArgs &la, const LimitReleaseArgs &r)
{
  hipError_t e = launch_limit_passes(stream, la, 0, 2);
  if (e != hipSuccess) return e;
  e = launch_release(stream, r);
  if (e != hipSuccess) return e;
  return launch_limit_passes(stream, la, 2, 3);
}

void limit_release_host(const LimitArgs &la, const LimitReleaseArgs &a)
{
  limit_host_passes(la, true, false);
  for (unsigned long long s = 0; s < (unsigned long long)a.nstreams; ++s) {
    const Entries e = entries_of(a, s);
    for (unsigned long long i = 0; i < e.nb; ++i) {
      const double *p = e.m + i * a.block;
      const unsigned long long n = e.J - i * a.block < a.block ? e.J - i * a.block : a.block;
      limit_release_first(p[0], a.a, a.b, e.C[i], e.A[i], e.B[i]);
      for (unsigned long long t = 1; t < n; ++t) limit_release_extend(p[t], a.a, a.b, e.C[i], e.A[i], e.B[i]);
    }
    if (e.nb) e.S[0] = 1.0;
    for (unsigned long long i = 0; i < e.nb; ++i) e.S[i + 1] = limit_release_carry(e.C[i], e.A[i], e.B[i], e.S[i]);
    for (unsigned long long i = 0; i < e.nb; ++i) {
      double *p = e.m + i * a.block, st = e.S[i];
      const unsigned long long n = e.J - i * a.block < a.block ? e.J - i * a.block : a.block;
      for (unsigned long long t = 0; t < n; ++t) p[t] = st = limit_release_step(p[t], a.a, a.b, st);
    }
  }
  limit_host_passes(la, false, true);
}

} // namespace rsmp
