// The limiter's release by windows ("Windows with the limiter's release"): RRX_tracks_limit_release_window_device.
// The per-step arithmetic is limit_release.hpp's; what is new is the geometry of a window on a track's ABSOLUTE block grid and
// the state that carries the scan across a cut.  A call works on the entries [e0, end) of a track, e0 = the slice frame of its
// first emitted frame, e1 the one behind its last, end = e1 + lookahead - 1; the "pieces" are the absolute blocks intersected
// with that range.  The state describes the scan at an entry e = i * block + r (include/ratelib_amd.h):
//   [0] S_i   [1..3] C, A, B of the entries [i * block, e), +0.0 at r == 0   [4] p = q[e - 1] run from S_i, S_i at r == 0   [5..7] +0.0
// It is read at e0 (only when e0 > 0) and written at e1.  The kernels (limit_release_window.hip) and the host twin behind
// RRX_debug_tracks_limit_release_window_host both take the cut and the pieces from the functions below.
#pragma once
#include <hip/hip_runtime.h>

#include "limit_release.hpp"

namespace rsmp {

constexpr int kLimitReleaseWinState = 8;
constexpr int kLimitReleaseStateS = 0, kLimitReleaseStateC = 1, kLimitReleaseStateA = 2, kLimitReleaseStateB = 3, kLimitReleaseStateP = 4;

// pieces a window of win_frames frames can meet in one track: a range of E entries meets at most E / block + 2 blocks
__host__ __device__ __forceinline__ unsigned long long limit_release_window_pieces(unsigned long long win_frames, unsigned lookahead, unsigned block)
{
  return (win_frames + (lookahead - 1)) / block + 2;
}

// What a window takes of one track.  np == 0: no frame of the track's slice lies in the window.
struct LimitReleaseCut {
  unsigned long long e0, e1; // the slice frames [e0, e1) are emitted: limit.hip's Row::lo and Row::hi
  unsigned long long end;    // the entries [e0, end) are released, end = e1 + lookahead - 1 <= J
  unsigned long long i0;     // the block of e0
  unsigned long long np;     // pieces: the blocks i0 .. i0 + np - 1, each cut to [e0, end)
  unsigned long long nc;     // of which the first nc reach the end of their block (np or np - 1)
  unsigned long long k1;     // the block of e1, counted from i0 (<= nc)
  unsigned r0, r1;           // e0 % block, e1 % block
};

__host__ __device__ __forceinline__ LimitReleaseCut limit_release_window_cut(const Track &tr, unsigned long long row_frames, unsigned long long win_first,
                                                                             unsigned long long win_frames, unsigned lookahead, unsigned block)
{
  LimitReleaseCut c = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  const TracksSlice sl = tracks_slice(tr, row_frames, 0, false);
  const unsigned long long wend = win_first + win_frames, top = sl.of + sl.frames;
  const unsigned long long lo = sl.of > win_first ? sl.of : win_first, hi = top < wend ? top : wend;
  if (hi <= lo) return c;
  c.e0 = lo - sl.of;
  c.e1 = hi - sl.of;
  c.end = c.e1 + (lookahead - 1);
  c.i0 = c.e0 / block;
  c.r0 = (unsigned)(c.e0 % block);
  c.r1 = (unsigned)(c.e1 % block);
  c.np = (c.end - 1) / block - c.i0 + 1;
  c.nc = c.end / block - c.i0;
  c.k1 = c.e1 / block - c.i0;
  return c;
}

// piece k < c.np: its first entry and how many it holds (1 .. block)
__host__ __device__ __forceinline__ void limit_release_window_piece(const LimitReleaseCut &c, unsigned block, unsigned long long k,
                                                                    unsigned long long &start, unsigned &n)
{
  const unsigned long long b0 = (c.i0 + k) * block, b1 = b0 + block;
  start = b0 > c.e0 ? b0 : c.e0;
  n = (unsigned)((b1 < c.end ? b1 : c.end) - start);
}

// What the three launches between the window minimum and the product take.  Track t owns work[t * stream_stride ...): the entry
// j of m at m_off + (j - e0); C and A of piece k at c_off + k and c_off + sum_stride + k, B and S at b_off + k and b_off +
// sum_stride + k, sum_stride = limit_release_window_pieces.
struct LimitReleaseWindowArgs {
  double *work;
  const Track *tracks;
  const double *state_in;          // [ntracks][kLimitReleaseWinState], null only with win_first == 0
  double *state_out;               // likewise, may be null
  unsigned long long row_frames, win_first, win_frames;
  unsigned long long stream_stride, m_off, c_off, b_off, sum_stride;
  unsigned lookahead, block;
  double a, b;                     // the pole and 1.0 - a
  int ntracks;
};

// The whole call: limit.hip's detector and window minimum on the window's sub-range (launch_limit_window_passes), summary, carry,
// run, limit.hip's product.  `la` and `w` are the window limiter's arguments with la.work_stride = half a track's share of the
// work buffer, so that r lies at its start and m at r.m_off = la.work_stride.  Only enqueues.
hipError_t launch_limit_release_window(hipStream_t stream, const LimitArgs &la, const LimitWindow &w, const LimitReleaseWindowArgs &r);
// the same on host pointers and a host table, as serial loops over the functions above, limit_release.hpp's and limit_host's
// (test hook: RRX_debug_tracks_limit_release_window_host)
void limit_release_window_host(const LimitArgs &la, const LimitWindow &w, const LimitReleaseWindowArgs &r);

} // namespace rsmp
