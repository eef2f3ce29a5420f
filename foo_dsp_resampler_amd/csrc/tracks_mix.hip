// Channel mixing on the device ("Channel mixing"): tracks_mix_sum (tracks_mix.hpp) per frame, in three places.
//
// Stage with a mix (RRX_tracks_stage_mix_device and its window form): tracks.hip's stage pass with the matrix applied on load.
// The packed source is [src_total][nch_src] of any TracksSrc, the rows are [ntracks][row_frames][nch] float32, and the regions
// of a row -- backward extension, the track, forward extension, zeros -- are tracks.hip's, from the same clamped table entries
// (tracks_entry / tracks_stage_cut).  tracks_mix_copy_kernel writes the track and the zeros, tracks_mix_lpc_kernel the two
// extensions, from base frames that are mixed as they are loaded: the rows are those of the un-mixed stage on the mixed source.
//
// The copy (mix_span): a workgroup takes tiles of mix_tile_frames consecutive frames.  A tile's source bytes are contiguous from
// any byte offset; all lanes bring them into LDS in aligned 16-byte pieces, the pieces at a tile's two ends dword by dword so
// that no dword is read that holds no byte of the tile's readable frames.  Then lane l takes frames l, l + 256, ... of the
// tile from LDS, one frame at a time: exact doubles, the matrix, one rounding, nch stores.  Consecutive lanes store consecutive
// frames.  The matrix is wave-uniform and stays in the launch arguments, compacted to its connected terms on the host.
//
// Rows (RRX_mix_device): the same span on plain rows of float32 or float64, where every frame is a source frame.
#include "tracks_mix.hpp"

#include "kernels.hpp"
#include "lpc_body.hpp"

namespace rsmp {
namespace {

typedef unsigned long long u64;

constexpr int kThreads = 256;
constexpr int kLdsPieces = kMixTileBytes / 16 + 2; // the tile, begun anywhere inside a 16-byte piece and ended anywhere inside one
__device__ __forceinline__ u64 min_u(u64 x, u64 y) { return x < y ? x : y; }
__device__ __forceinline__ u64 max_u(u64 x, u64 y) { return x > y ? x : y; }

// The n frames at `row` (a row, the window of one, or a stream's frames).  [c0, c1) is the track: frame c0 + j is the mix of
// source frame j, the frame at s + j * frame bytes, where j < have and zero from there; [z0, n) are zeros; what lies in front of
// c0 and between c1 and z0 is not written.  The workgroup takes tiles blockIdx.x * steps + [0, steps).
template <int kSrc, typename Out>
__device__ __forceinline__ void mix_span(uint4 *lds, const TracksMix &m, Out *row, u64 n, u64 c0, u64 c1, u64 z0, u64 have,
                                         const unsigned char *s, int steps)
{
  const unsigned tid = threadIdx.x;
  const u64 nsrc = (u64)m.nch_src, ndst = (u64)m.nch_dst;
  const u64 fb = nsrc * (u64)mix_src_bytes(kSrc);     // bytes of a source frame
  const u64 tile = (u64)kMixTileBytes / fb;           // mix_tile_frames
  for (int u = 0; u < steps; ++u) {
    const u64 k0 = ((u64)blockIdx.x * (unsigned)steps + (unsigned)u) * tile;
    if (k0 >= n) break;
    const u64 k1 = min_u(k0 + tile, n);
    // source frames [f0, f1) of the track are the tile's readable ones
    const u64 lo = max_u(k0, c0), hi = min_u(k1, c1);
    const u64 f0 = lo < hi ? lo - c0 : 0, f1 = lo < hi ? min_u(hi - c0, have) : 0;
    if (u) __syncthreads(); // the tile before has been read
    u64 off = 0;            // of source frame f0 in the LDS tile
    if (f1 > f0) {
      const u64 b0 = reinterpret_cast<u64>(s) + f0 * fb, b1 = reinterpret_cast<u64>(s) + f1 * fb; // its bytes: at most kMixTileBytes
      const u64 a0 = b0 & ~15ull, d0 = b0 & ~3ull, d1 = (b1 + 3) & ~3ull;                         // [d0, d1): the dwords that hold one
      off = b0 - a0;
      for (u64 p = a0 + tid * 16; p < d1; p += kThreads * 16) {
        uint4 v = {0u, 0u, 0u, 0u};
        if (p >= d0 && p + 16 <= d1) {
          v = *reinterpret_cast<const uint4 *>(p);
        } else {
          if (p >= d0) v.x = *reinterpret_cast<const unsigned *>(p);
          if (p + 4 >= d0 && p + 4 < d1) v.y = *reinterpret_cast<const unsigned *>(p + 4);
          if (p + 8 >= d0 && p + 8 < d1) v.z = *reinterpret_cast<const unsigned *>(p + 8);
          if (p + 12 >= d0 && p + 12 < d1) v.w = *reinterpret_cast<const unsigned *>(p + 12);
        }
        lds[(p - a0) >> 4] = v;
      }
    }
    __syncthreads();
    const unsigned char *base = reinterpret_cast<const unsigned char *>(lds) + off;
    for (u64 k = k0 + tid; k < k1; k += kThreads) {
      Out *y = row + k * ndst;
      if (k >= c0 && k < c1 && k - c0 < f1) { // (k - c0 >= f0: the tile begins there)
        const unsigned char *frame = base + (k - c0 - f0) * fb;
        for (int o = 0; o < m.nch_dst; ++o) y[o] = (Out)tracks_mix_sum(m, kSrc, frame, o);
      } else if ((k >= c0 && k < c1) || k >= z0) { // the track's frames that a wrong table puts past the source, and the zeros
        for (int o = 0; o < m.nch_dst; ++o) y[o] = (Out)0;
      }
    }
  }
}

__device__ __forceinline__ TracksEntry entry_of(const TracksStageArgs &a, u64 t) { return tracks_entry(a.tracks[t], a.row_frames, a.src_total); }

template <int kSrc> __global__ __launch_bounds__(kThreads) void tracks_mix_copy_kernel(TracksStageArgs a, TracksMix m, int t0, int steps)
{
  __shared__ uint4 lds[kLdsPieces];
  const u64 t = (u64)(t0 + (int)blockIdx.y), fb = (u64)m.nch_src * tracks_src_bytes(kSrc);
  const TracksEntry e = entry_of(a, t);
  const u64 c0 = e.lead, c1 = c0 + e.frames, z0 = c1 + e.fwd;
  const unsigned char *s = static_cast<const unsigned char *>(a.src) + e.first * fb;
  mix_span<kSrc, float>(lds, m, a.rows + t * a.row_frames * (u64)a.nch, a.row_frames, c0, c1, z0, e.have, s, steps);
}

// The window form: the regions are the row's cut to the window (tracks_stage_cut), and the tiles count from the window's first frame
template <int kSrc> __global__ __launch_bounds__(kThreads) void tracks_mix_copy_window_kernel(TracksStageArgs a, TracksMix m, TracksWindow w, int t0, int steps)
{
  __shared__ uint4 lds[kLdsPieces];
  const u64 t = (u64)(t0 + (int)blockIdx.y), fb = (u64)m.nch_src * tracks_src_bytes(kSrc);
  const TracksStageCut c = tracks_stage_cut(a.tracks[t], a.row_frames, a.src_total, w);
  const unsigned char *s = static_cast<const unsigned char *>(a.src) + c.src_frame * fb; // the frame that window frame cp[0] is the mix of
  mix_span<kSrc, float>(lds, m, a.rows + t * w.stride * (u64)a.nch, w.frames, c.cp[0], c.cp[1], c.z[0], c.readable, s, steps);
}

// One edge (0: backward, 1: forward) of OUTPUT channel ch of a track: tracks.hip's lpc_edge, with base frames that are mixed as
// they are loaded (tracks_mix_sample reads the connected channels of the packed frame, exactly their bytes).
template <int kSrc, bool kWin>
__device__ __forceinline__ void mix_lpc_edge(unsigned char *lds, const TracksStageArgs &a, const TracksMix &m, const TracksEntry &e, int edge, int ch,
                                             long long extra, float *y, long long org, long long lo, long long hi)
{
  const int lane = threadIdx.x, nch = a.nch;
  const u64 fb = (u64)m.nch_src * tracks_src_bytes(kSrc);
  const long long n = (long long)min_u(e.frames, (u64)a.prime_len);      // base frames: the track's first n, or its last n
  const u64 base = edge ? e.frames - (u64)n : 0;
  const long long readable = e.have > base ? (long long)(e.have - base) : 0; // (all n of them, unless the table is wrong)
  const unsigned char *x = static_cast<const unsigned char *>(a.src) + (e.first + min_u(base, e.have)) * fb; // base frame 0
  if (n <= kLpcMaxOrder) { // no table of RRX_tracks_plan: a lead means more than 64 frames.  Zeros, so that the row is written all the same.
    for (long long i = lane; i < extra; i += 64) {
      const long long k = org + (edge ? n + i : -1 - i);
      if (!kWin || (k >= lo && k < hi)) y[k * nch] = 0.0f;
    }
    return;
  }
  lpc_channel<true>(lds, lane, n, (float)(n + 1) / 2.0f, kLpcMaxOrder, edge ? 0 : extra, edge ? extra : 0,
                    [=, &m](long long i) { return i < readable ? tracks_mix_sample(m, kSrc, x + (u64)i * fb, ch) : 0.0f; },
                    [=](long long i, float v) {
                      const long long k = org + i;
                      if (!kWin || (k >= lo && k < hi)) y[k * nch] = v;
                    });
}

template <int kSrc> __global__ __launch_bounds__(64) void tracks_mix_lpc_kernel(TracksStageArgs a, TracksMix m)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char tracks_mix_lds[];
  const int edge = blockIdx.x & 1, nch = a.nch;
  const u64 t = (blockIdx.x >> 1) / (unsigned)nch, ch = (blockIdx.x >> 1) % (unsigned)nch;
  const TracksEntry e = entry_of(a, t);
  const long long extra = (long long)(edge ? e.fwd : e.lead);
  if (!extra) return;
  const u64 base = edge ? e.frames - min_u(e.frames, (u64)a.prime_len) : 0;
  float *y = a.rows + ((t * a.row_frames + e.lead + base) * nch + ch);
  mix_lpc_edge<kSrc, false>(tracks_mix_lds, a, m, e, edge, (int)ch, extra, y, 0, 0, 0);
}

// The window form, as tracks_lpc_window_kernel: the same grid; a workgroup whose extension does not meet the window returns
// before it loads a base frame, one that does runs from the track's edge as far as the window asks and stores what lies inside.
template <int kSrc> __global__ __launch_bounds__(64) void tracks_mix_lpc_window_kernel(TracksStageArgs a, TracksMix m, TracksWindow w)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char tracks_mix_lds[];
  const int edge = blockIdx.x & 1, nch = a.nch;
  const u64 t = (blockIdx.x >> 1) / (unsigned)nch, ch = (blockIdx.x >> 1) % (unsigned)nch;
  const TracksStageCut c = tracks_stage_cut(a.tracks[t], a.row_frames, a.src_total, w);
  const u64 *r = edge ? c.fw : c.bk;
  if (r[0] == r[1]) return;
  const TracksEntry &e = c.e;
  const long long extra = (long long)(edge ? w.first + r[1] - (e.lead + e.frames) : e.lead - (w.first + r[0]));
  const u64 base = edge ? e.frames - min_u(e.frames, (u64)a.prime_len) : 0;
  const long long org = (long long)(e.lead + base) - (long long)w.first; // base frame 0 as a window frame (before the window: negative)
  float *y = a.rows + (t * w.stride * nch + ch);                         // window frame 0 of this channel
  mix_lpc_edge<kSrc, true>(tracks_mix_lds, a, m, e, edge, (int)ch, extra, y, org, (long long)r[0], (long long)r[1]);
}

// Rows: stream blockIdx.y's frames, every one a source frame
template <int kSrc, typename S> __global__ __launch_bounds__(kThreads) void mix_rows_kernel(MixRowsArgs a, TracksMix m, int s0, int steps)
{
  __shared__ uint4 lds[kLdsPieces];
  const u64 st = (u64)(s0 + (int)blockIdx.y);
  const S *src = static_cast<const S *>(a.src) + st * a.src_stride;
  mix_span<kSrc, S>(lds, m, static_cast<S *>(a.dst) + st * a.dst_stride, a.frames, 0, a.frames, a.frames, a.frames,
                    reinterpret_cast<const unsigned char *>(src), steps);
}

// tiles per workgroup: 8 where there are that many, more only to stay inside the grid limit
void tile_grid(u64 frames, u64 tile, unsigned &gx, int &steps)
{
  const u64 tiles = (frames + tile - 1) / tile;
  u64 st = tiles < 8 ? 1 : 8;
  while ((tiles + st - 1) / st > 0x7fffffffull) st *= 2;
  gx = (unsigned)((tiles + st - 1) / st);
  if (!gx) gx = 1;
  steps = (int)st;
}

// w: the window form, or null
template <int kSrc> hipError_t stage_typed(hipStream_t stream, const TracksStageArgs &a, const TracksMix &m, const TracksWindow *w)
{
  unsigned gx;
  int steps;
  tile_grid(w ? w->frames : a.row_frames, (u64)mix_tile_frames(kSrc, m.nch_src), gx, steps);
  for (int t0 = 0; t0 < a.ntracks; t0 += 32768) { // grid.y is a 16-bit count
    const int nt = a.ntracks - t0 < 32768 ? a.ntracks - t0 : 32768;
    if (w) hipLaunchKernelGGL(tracks_mix_copy_window_kernel<kSrc>, dim3(gx, (unsigned)nt), dim3(kThreads), 0, stream, a, m, *w, t0, steps);
    else hipLaunchKernelGGL(tracks_mix_copy_kernel<kSrc>, dim3(gx, (unsigned)nt), dim3(kThreads), 0, stream, a, m, t0, steps);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  // the two extensions of every (track, output channel)
  static DynLdsOnce once, once_window; // (one per instance)
  const void *fn = w ? reinterpret_cast<const void *>(&tracks_mix_lpc_window_kernel<kSrc>) : reinterpret_cast<const void *>(&tracks_mix_lpc_kernel<kSrc>);
  const hipError_t e = (w ? once_window : once).set(fn, int(sizeof(LpcShared) + kLpcLdsFrames * sizeof(float)));
  if (e != hipSuccess) return e;
  const size_t lds = sizeof(LpcShared) + size_t(a.prime_len) * sizeof(float);
  const dim3 grid((unsigned)((long long)a.ntracks * a.nch * 2));
  if (w) hipLaunchKernelGGL(tracks_mix_lpc_window_kernel<kSrc>, grid, dim3(64), lds, stream, a, m, *w);
  else hipLaunchKernelGGL(tracks_mix_lpc_kernel<kSrc>, grid, dim3(64), lds, stream, a, m);
  return hipGetLastError();
}

hipError_t stage_kind(hipStream_t stream, const TracksStageArgs &a, const TracksMix &m, const TracksWindow *w)
{
  switch (a.src_kind) {
  case kTracksSrcF32: return stage_typed<kTracksSrcF32>(stream, a, m, w);
  case kTracksSrcS16: return stage_typed<kTracksSrcS16>(stream, a, m, w);
  case kTracksSrcS24: return stage_typed<kTracksSrcS24>(stream, a, m, w);
  case kTracksSrcS32: return stage_typed<kTracksSrcS32>(stream, a, m, w);
  default: return hipErrorInvalidValue; // a missing kernel is an error, never another kernel
  }
}

template <int kSrc, typename S> hipError_t rows_typed(hipStream_t stream, const MixRowsArgs &a, const TracksMix &m)
{
  unsigned gx;
  int steps;
  tile_grid(a.frames, (u64)mix_tile_frames(kSrc, m.nch_src), gx, steps);
  for (int s0 = 0; s0 < a.nstreams; s0 += 32768) { // grid.y is a 16-bit count
    const int ns = a.nstreams - s0 < 32768 ? a.nstreams - s0 : 32768;
    hipLaunchKernelGGL((mix_rows_kernel<kSrc, S>), dim3(gx, (unsigned)ns), dim3(kThreads), 0, stream, a, m, s0, steps);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

template <int kSrc, typename S> void rows_host(const MixRowsArgs &a, const TracksMix &m)
{
  for (int st = 0; st < a.nstreams; ++st) {
    const S *src = static_cast<const S *>(a.src) + (u64)st * a.src_stride;
    S *dst = static_cast<S *>(a.dst) + (u64)st * a.dst_stride;
    for (u64 k = 0; k < a.frames; ++k)
      for (int o = 0; o < m.nch_dst; ++o) dst[k * m.nch_dst + o] = (S)tracks_mix_sum(m, kSrc, src + k * m.nch_src, o);
  }
}

} // namespace

hipError_t launch_tracks_stage_mix(hipStream_t stream, const TracksStageArgs &a, const TracksMix &m) { return stage_kind(stream, a, m, nullptr); }
hipError_t launch_tracks_stage_mix_window(hipStream_t stream, const TracksStageArgs &a, const TracksMix &m, const TracksWindow &w)
{
  return stage_kind(stream, a, m, &w);
}

hipError_t launch_mix_rows(hipStream_t stream, const MixRowsArgs &a, const TracksMix &m)
{
  return a.is_double ? rows_typed<kMixSrcF64, double>(stream, a, m) : rows_typed<kTracksSrcF32, float>(stream, a, m);
}

void mix_rows_host(const MixRowsArgs &a, const TracksMix &m)
{
  if (a.is_double) rows_host<kMixSrcF64, double>(a, m);
  else rows_host<kTracksSrcF32, float>(a, m);
}

} // namespace rsmp
