// The limiter's release by windows ("Windows with the limiter's release"): RRX_tracks_limit_release_window_device.
// The arithmetic is limit_release.hpp's, the cut of a track and its pieces limit_release_window.hpp's, both shared with the host
// twin at the end of this file; the detector, the window minimum and the product are limit.hip's window launches, untouched.
// Between the window minimum and the product, three launches on the entries [e0, end) of every track that has a frame in the
// window, in pieces -- the track's absolute blocks cut to that range:
//   summary  one lane per (track, piece), 64 to a workgroup: (C, A, B) of the piece, from nothing or, for a first piece that
//            begins mid-block, going on from the state's.  The lane that passes e1 mid-block keeps its (C, A, B) of that
//            moment for the outgoing state and walks on: the piece is never split at e1.
//   carry    one wave per track, pieces ascending, from the state's S (1.0 at e0 == 0): S_{k+1} = fmin(C_k, A_k * S_k + B_k) for
//            every piece that reaches the end of its block, handed round through LDS as in limit_release.hip.  The wave also
//            writes what of the outgoing state no other lane does: S, the zeros, all of it where e1 lies on a block boundary,
//            and the copy of the incoming state for a track without a frame in the window.
//   run      the summary's lanes again: q over m in place, a first mid-block piece from the state's p, every other from its
//            S_k; the lane that passes e1 mid-block keeps q[e1 - 1] for the outgoing state.
// The tile walk is limit_release_pass_kernel's -- a tile of each of the workgroup's pieces goes through LDS, sixteen consecutive
// threads to 128 bytes of a piece, rows at an odd pitch, the next tile's loads issued before this tile is computed, q handed
// back the way it came -- with three changes, each measured.  A window holds few pieces a track (W / block + 2), so
// a launch is a handful of live lanes a workgroup and its time is the latency of one lane's serial walk over a block: tiles of 64
// entries make a quarter of the round trips to memory, 64 pieces to a workgroup keep the LDS tile at 33 KB and sixteen loads a
// thread, and the chain has no branch and no select in it.  A piece begins at an arbitrary entry of m, so the 128 bytes are no
// longer one aligned line but at most two; and the walk ends at the longest piece the window can hold, not at `block`.
#include "limit_release_window.hpp"

namespace rsmp {
namespace {

constexpr int kThreads = 256, kLine = 16;                  // sixteen threads load 128 bytes
constexpr int kPieces = 64, kTile = 64, kPitch = kTile + 1; // pieces of a workgroup, entries of a tile, doubles between two rows
constexpr int kSegs = kTile / kLine, kSubs = kThreads / kLine, kLoads = kPieces * kSegs / kSubs; // 128-byte segments: of a tile, a pass, a thread
static_assert(kTile % kLine == 0 && (kPieces * kSegs) % kSubs == 0 && kPieces <= kThreads, "whole passes over the tile");
constexpr int kCarryThreads = 64; // one wave: the carry's workgroup

struct Pieces {
  LimitReleaseCut c;
  double *m, *C, *A, *B, *S; // m[0] is entry e0
  const double *in;          // the track's incoming state, null when it is not to be read
  double *out;               // the track's outgoing state or null
};

__host__ __device__ __forceinline__ Pieces pieces_of(const LimitReleaseWindowArgs &a, unsigned long long t)
{
  Pieces p;
  p.c = limit_release_window_cut(a.tracks[t], a.row_frames, a.win_first, a.win_frames, a.lookahead, a.block);
  double *base = a.work + t * a.stream_stride;
  p.m = base + a.m_off;
  p.C = base + a.c_off;
  p.A = p.C + a.sum_stride;
  p.B = base + a.b_off;
  p.S = p.B + a.sum_stride;
  p.in = a.state_in ? a.state_in + t * kLimitReleaseWinState : nullptr;
  p.out = a.state_out ? a.state_out + t * kLimitReleaseWinState : nullptr;
  return p;
}

// the first piece goes on from the state (e0 > 0 then, and the state is there: capi_stage.cpp refuses a null one behind frame 0)
__host__ __device__ __forceinline__ bool continues(const Pieces &p, unsigned long long k) { return k == 0 && p.c.r0 > 0; }

// the entry t of piece k (which begins at `start`) behind which the state is taken, or ~0u: e1 - 1 lies in the piece, mid-block
__host__ __device__ __forceinline__ unsigned snapshot_at(const Pieces &p, unsigned long long k, unsigned long long start)
{
  return p.out && p.c.r1 > 0 && k == p.c.k1 ? (unsigned)(p.c.e1 - 1 - start) : ~0u;
}

// kRun = false: the summary; true: the run.  Thread tid < kPieces is the lane of piece g0 + tid; every thread loads entry tt of
// the segments sub, sub + 16, ... of the workgroup's tiles, segment g being entries [16 * (g % kSegs), +16) of piece g / kSegs (at).
template <bool kRun> __global__ __launch_bounds__(kThreads) void limit_release_window_pass_kernel(LimitReleaseWindowArgs a, int s0)
{
  __shared__ double tile[kPieces * kPitch];
  const Pieces e = pieces_of(a, (unsigned long long)(s0 + (int)blockIdx.y));
  if (!e.c.np) return; // (the whole workgroup)
  const unsigned block = a.block, tid = threadIdx.x, sub = tid / kLine, tt = tid % kLine;
  const double pole = a.a, b = a.b;
  const unsigned span = e.c.end - e.c.e0 < block ? (unsigned)(e.c.end - e.c.e0) : block; // no piece is longer
  for (unsigned long long g0 = (unsigned long long)blockIdx.x * kPieces; g0 < e.c.np; g0 += (unsigned long long)gridDim.x * kPieces) {
    const unsigned long long i = g0 + tid;
    unsigned long long start = 0;
    unsigned n = 0;
    if (tid < (unsigned)kPieces && i < e.c.np) limit_release_window_piece(e.c, block, i, start, n);
    const unsigned snap = n ? snapshot_at(e, i, start) : ~0u;
    double r[kLoads];
    auto at = [&](int k, unsigned t0, unsigned long long &o, unsigned &cell) { // o: the entry's place in m; cell: its place in the tile
      const unsigned g = sub + (unsigned)k * kSubs, row = g / kSegs, t = (g % kSegs) * kLine + tt;
      const unsigned long long pc = g0 + row;
      cell = row * kPitch + t;
      if (pc >= e.c.np) return false;
      unsigned long long ps;
      unsigned pn;
      limit_release_window_piece(e.c, block, pc, ps, pn);
      o = ps - e.c.e0 + t0 + t;
      return t0 + t < pn;
    };
    auto gload = [&](unsigned t0) {
#pragma unroll
      for (int k = 0; k < kLoads; ++k) {
        unsigned long long o;
        unsigned cell;
        r[k] = at(k, t0, o, cell) ? e.m[o] : 1.0;
      }
    };
    auto put = [&]() {
#pragma unroll
      for (int k = 0; k < kLoads; ++k) {
        const unsigned g = sub + (unsigned)k * kSubs;
        tile[(g / kSegs) * kPitch + (g % kSegs) * kLine + tt] = r[k];
      }
    };
    gload(0);
    __syncthreads(); // the readers of the tile before are done
    put();
    __syncthreads();
    const bool on = n && continues(e, i);
    // A summary from nothing starts at (+inf, 1.0, +0.0), from which limit_release_extend gives limit_release_first's bits:
    // fmin(v, a * inf + u) = v (a NaN where a == 0.0, which fmin drops too), a * 1.0 = a, a * 0.0 + u = u, for the v in [0, 1]
    // and the a in [0, 1) the call has.  So the chain is one function whatever the entry.
    double C = __builtin_inf(), A = 1.0, B = 0.0, st = 0.0;
    double sC = 0.0, sA = 0.0, sB = 0.0; // the snapshot at e1: (C, A, B) of the summary, p (in sC) of the run
    double fC = 0.0, fA = 0.0, fB = 0.0; // the summary at the piece's last entry
    if (kRun) st = on ? e.in[kLimitReleaseStateP] : n ? e.S[i] : 0.0;
    else if (on) {
      C = e.in[kLimitReleaseStateC];
      A = e.in[kLimitReleaseStateA];
      B = e.in[kLimitReleaseStateB];
    }
    for (unsigned t0 = 0; t0 < span; t0 += kTile) {
      if (t0 + kTile < span) gload(t0 + kTile); // in flight while this tile is computed; loaded before the run stores over anything
      // Every lane takes every step of the tile, with no branch and no select inside the serial chain: what the chain holds
      // behind the piece's last entry is nobody's (the store back is guarded by `at`), and what it held at that entry and at
      // e1 - 1 is picked off beside it.
      if (tid < (unsigned)kPieces) {
#pragma unroll 16
        for (int t = 0; t < kTile; ++t) {
          const unsigned at_t = t0 + (unsigned)t;
          const bool last = at_t + 1 == n, take = at_t == snap;
          const double v = tile[tid * kPitch + t];
          if (kRun) {
            st = limit_release_step(v, pole, b, st);
            tile[tid * kPitch + t] = st;
            sC = take ? st : sC;
          } else {
            limit_release_extend(v, pole, b, C, A, B);
            sC = take ? C : sC;
            sA = take ? A : sA;
            sB = take ? B : sB;
            fC = last ? C : fC;
            fA = last ? A : fA;
            fB = last ? B : fB;
          }
        }
      }
      __syncthreads(); // every lane is done with its row of the tile
      if (kRun) { // q of this tile, as it was loaded: 128 bytes of a piece to sixteen threads
#pragma unroll
        for (int k = 0; k < kLoads; ++k) {
          unsigned long long o;
          unsigned cell;
          if (at(k, t0, o, cell)) e.m[o] = tile[cell];
        }
        __syncthreads();
      }
      put(); // the next tile (behind the last one: what r still holds, which nobody reads)
      __syncthreads();
    }
    if (!kRun && n) {
      e.C[i] = fC;
      e.A[i] = fA;
      e.B[i] = fB;
    }
    if (snap != ~0u) { // (one lane of the track)
      if (kRun) e.out[kLimitReleaseStateP] = sC;
      else {
        e.out[kLimitReleaseStateC] = sC;
        e.out[kLimitReleaseStateA] = sA;
        e.out[kLimitReleaseStateB] = sB;
      }
    }
  }
}

// what of the outgoing state the carry leaves: `S` is S of the block of e1
__host__ __device__ __forceinline__ void state_from_carry(const Pieces &e, double S, unsigned w)
{
  const bool edge = e.c.r1 == 0; // (C, A, B) and p are the summary's and the run's otherwise
  if (w == kLimitReleaseStateS || (edge && w == kLimitReleaseStateP)) e.out[w] = S;
  else if (w > kLimitReleaseStateP || edge) e.out[w] = 0.0;
}

__global__ __launch_bounds__(kCarryThreads) void limit_release_window_carry_kernel(LimitReleaseWindowArgs a)
{
  __shared__ double sh[3][kCarryThreads];
  const unsigned lane = threadIdx.x;
  for (unsigned long long s = blockIdx.x; s < (unsigned long long)a.ntracks; s += gridDim.x) { // (the whole wave)
    const Pieces e = pieces_of(a, s);
    if (!e.c.np) { // no frame in the window: the state passes through
      if (e.out && lane < (unsigned)kLimitReleaseWinState) e.out[lane] = e.in ? e.in[lane] : 0.0;
      continue;
    }
    double S = e.c.e0 ? e.in[kLimitReleaseStateS] : 1.0, C = 1.0, A = 1.0, B = 0.0;
    double at_e1 = S; // S of the block of e1
    if (!lane) e.S[0] = S;
    auto fetch = [&](unsigned long long i) {
      if (i + lane < e.c.nc) {
        C = e.C[i + lane];
        A = e.A[i + lane];
        B = e.B[i + lane];
      }
    };
    fetch(0);
    for (unsigned long long i = 0; i < e.c.nc; i += kCarryThreads) {
      __syncthreads(); // the readers of the batch before are done
      sh[0][lane] = C;
      sh[1][lane] = A;
      sh[2][lane] = B;
      __syncthreads();
      if (i + kCarryThreads < e.c.nc) fetch(i + kCarryThreads); // in flight while this batch is carried
      const unsigned n = e.c.nc - i < (unsigned long long)kCarryThreads ? (unsigned)(e.c.nc - i) : (unsigned)kCarryThreads;
      double mine = 0.0;
      for (unsigned u = 0; u < n; ++u) { // every lane the same chain
        S = limit_release_carry(sh[0][u], sh[1][u], sh[2][u], S);
        mine = u == lane ? S : mine;
        at_e1 = i + u + 1 == e.c.k1 ? S : at_e1;
      }
      if (lane < n && i + lane + 1 < e.c.np) e.S[i + lane + 1] = mine;
    }
    if (e.out && lane < (unsigned)kLimitReleaseWinState) state_from_carry(e, at_e1, lane);
  }
}

hipError_t launch_release_window(hipStream_t stream, const LimitReleaseWindowArgs &a)
{
  const unsigned long long groups = (a.sum_stride + kPieces - 1) / kPieces; // lanes of the longest cut
  const unsigned gx = groups > 0x7fffffffull ? 0x7fffffffu : (unsigned)groups;
  for (int pass = 0; pass < 3; ++pass) {
    if (pass == 1) {
      hipLaunchKernelGGL(limit_release_window_carry_kernel, dim3((unsigned)a.ntracks), dim3(kCarryThreads), 0, stream, a);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
      continue;
    }
    for (int s0 = 0; s0 < a.ntracks; s0 += 32768) { // grid.y is a 16-bit count
      const int ns = a.ntracks - s0 < 32768 ? a.ntracks - s0 : 32768;
      if (pass == 0) hipLaunchKernelGGL(limit_release_window_pass_kernel<false>, dim3(gx, (unsigned)ns), dim3(kThreads), 0, stream, a, s0);
      else hipLaunchKernelGGL(limit_release_window_pass_kernel<true>, dim3(gx, (unsigned)ns), dim3(kThreads), 0, stream, a, s0);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
    }
  }
  return hipSuccess;
}

} // namespace

hipError_t launch_limit_release_window(hipStream_t stream, const LimitArgs &la, const LimitWindow &w, const LimitReleaseWindowArgs &r)
{
  hipError_t e = launch_limit_window_passes(stream, la, w, 0, 2);
  if (e != hipSuccess) return e;
  e = launch_release_window(stream, r);
  if (e != hipSuccess) return e;
  return launch_limit_window_passes(stream, la, w, 2, 3);
}

void limit_release_window_host(const LimitArgs &la, const LimitWindow &w, const LimitReleaseWindowArgs &a)
{
  limit_host_window_passes(la, w, true, false);
  for (unsigned long long s = 0; s < (unsigned long long)a.ntracks; ++s) {
    const Pieces e = pieces_of(a, s);
    if (!e.c.np) {
      for (unsigned x = 0; e.out && x < (unsigned)kLimitReleaseWinState; ++x) e.out[x] = e.in ? e.in[x] : 0.0;
      continue;
    }
    for (unsigned long long k = 0; k < e.c.np; ++k) {
      unsigned long long start;
      unsigned n;
      limit_release_window_piece(e.c, a.block, k, start, n);
      const double *p = e.m + (start - e.c.e0);
      const unsigned snap = snapshot_at(e, k, start);
      const bool on = continues(e, k);
      double C = 1.0, A = 1.0, B = 0.0;
      if (on) {
        C = e.in[kLimitReleaseStateC];
        A = e.in[kLimitReleaseStateA];
        B = e.in[kLimitReleaseStateB];
      }
      for (unsigned t = 0; t < n; ++t) {
        if (t == 0 && !on) limit_release_first(p[t], a.a, a.b, C, A, B);
        else limit_release_extend(p[t], a.a, a.b, C, A, B);
        if (t == snap) {
          e.out[kLimitReleaseStateC] = C;
          e.out[kLimitReleaseStateA] = A;
          e.out[kLimitReleaseStateB] = B;
        }
      }
      e.C[k] = C;
      e.A[k] = A;
      e.B[k] = B;
    }
    double S = e.c.e0 ? e.in[kLimitReleaseStateS] : 1.0, at_e1 = S;
    e.S[0] = S;
    for (unsigned long long k = 0; k < e.c.nc; ++k) {
      S = limit_release_carry(e.C[k], e.A[k], e.B[k], S);
      if (k + 1 < e.c.np) e.S[k + 1] = S;
      if (k + 1 == e.c.k1) at_e1 = S;
    }
    for (unsigned x = 0; e.out && x < (unsigned)kLimitReleaseWinState; ++x) state_from_carry(e, at_e1, x);
    for (unsigned long long k = 0; k < e.c.np; ++k) {
      unsigned long long start;
      unsigned n;
      limit_release_window_piece(e.c, a.block, k, start, n);
      double *p = e.m + (start - e.c.e0), st = continues(e, k) ? e.in[kLimitReleaseStateP] : e.S[k];
      const unsigned snap = snapshot_at(e, k, start);
      for (unsigned t = 0; t < n; ++t) {
        p[t] = st = limit_release_step(p[t], a.a, a.b, st);
        if (t == snap) e.out[kLimitReleaseStateP] = st;
      }
    }
  }
  limit_host_window_passes(la, w, false, true);
}

} // namespace rsmp
