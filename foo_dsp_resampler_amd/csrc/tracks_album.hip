// Gapless albums ("Gapless albums"): the stage pass of tracks.hip for tracks with links (tracks_album.hpp).
//
// Row t, with b / a the frames of its neighbours that tracks_album_cut lets it hold:
//   linked backward edge   [0, lead - b) zeros, [lead - b, lead) the b frames in front of the track in the packed source
//   extrapolated           [0, lead) backward LPC extension, as tracks.hip writes it
//   [lead, lead + frames)  the track
//   linked forward edge    [.., .. + a) the a frames behind the track, zeros from there to the end of the row
//   extrapolated           [.., .. + fwd) forward LPC extension, zeros behind it
// so a linked row is one contiguous run of the source, [first - b, first + frames + a), between two runs of zeros, and
// tracks_album_copy_kernel is tracks_copy_kernel with a wider copy range and zeros in front: the same head / groups of 4 / tail by
// the destination's alignment, 16 bytes stored per lane, and for integer PCM the aligned dwords that cover a group, realigned by
// the run's misalignment (one value per workgroup) and unpacked.  No lane loads single bytes from global memory outside the at
// most 2 x 3 + 2 x 3 samples of a row's ends and region borders (DESIGN.md 10 measured byte loads at 2.4 times the dword form).
// tracks_album_lpc_kernel is tracks_lpc_window_kernel around the same lpc_edge body; a workgroup whose edge is linked returns
// when it has read its entry and link (a workgroup-uniform branch, in front of every base-frame load), so a linked edge costs no
// LPC work, and no host synchronisation picks the workgroups.  Both kernels are window forms: whole rows are the window
// [0, row_frames), for which the LPC kernel has an instance without the window checks.  They write disjoint frames and only read
// the source.
#include "tracks_album.hpp"

#include "kernels.hpp"
#include "lpc_body.hpp"

namespace rsmp {
namespace {

typedef unsigned long long u64;

constexpr int kThreads = kAlbumThreads;

__device__ __forceinline__ u64 min_u(u64 x, u64 y) { return x < y ? x : y; }

// the packed source as the kernels address it (tracks.hip): floats as floats, integer PCM as bytes, kStep of them a sample
template <int kSrc> struct Src {
  typedef unsigned char T;
  static constexpr u64 kStep = tracks_src_bytes(kSrc);
};
template <> struct Src<kTracksSrcF32> {
  typedef float T;
  static constexpr u64 kStep = 1;
};

// tracks.hip's lpc_edge: one edge (0: backward, 1: forward) of channel ch, `extra` frames counted outwards from the track's edge;
// extrapolated frame i (from base frame 0) is frame k = org + i of y; kWin: stored only where lo <= k < hi.  The same calls of
// lpc_channel with the same arguments, so the same bits.
template <int kSrc, bool kWin>
__device__ __forceinline__ void lpc_edge(unsigned char *lds, const TracksStageArgs &a, const TracksEntry &e, int edge, u64 ch, long long extra,
                                         float *y, long long org, long long lo, long long hi)
{
  typedef typename Src<kSrc>::T T;
  const int lane = threadIdx.x, nch = a.nch;
  const long long n = (long long)min_u(e.frames, (u64)a.prime_len); // base frames: the track's first n, or its last n
  const u64 base = edge ? e.frames - (u64)n : 0;
  const long long readable = e.have > base ? (long long)(e.have - base) : 0;
  const T *x = static_cast<const T *>(a.src) + ((e.first + min_u(base, e.have)) * nch + ch) * Src<kSrc>::kStep;
  if (n <= kLpcMaxOrder) { // too short to extrapolate from: zeros, as tracks.hip writes them
    for (long long i = lane; i < extra; i += 64) {
      const long long k = org + (edge ? n + i : -1 - i);
      if (!kWin || (k >= lo && k < hi)) y[k * nch] = 0.0f;
    }
    return;
  }
  lpc_channel<true>(lds, lane, n, (float)(n + 1) / 2.0f, kLpcMaxOrder, edge ? 0 : extra, edge ? extra : 0,
                    [=](long long i) { return i < readable ? tracks_load_sample(kSrc, x, (u64)(i * nch)) : 0.0f; },
                    [=](long long i, float v) {
                      const long long k = org + i;
                      if (!kWin || (k >= lo && k < hi)) y[k * nch] = v;
                    });
}

// kWin = false: the window is the whole row, so every store lies inside it and none is checked -- the recursion is one wave's
// serial chain, and what is issued per step is what the step costs (tracks.hip keeps a whole-row instance for the same reason).
template <int kSrc, bool kWin> __global__ __launch_bounds__(64) void tracks_album_lpc_kernel(TracksAlbumArgs a, TracksWindow w)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char tracks_album_lds[];
  const int edge = blockIdx.x & 1, nch = a.s.nch;
  const u64 t = (blockIdx.x >> 1) / (unsigned)nch, ch = (blockIdx.x >> 1) % (unsigned)nch;
  const TrackLink ln = a.links[t];
  if ((edge ? ln.ahead : ln.back) != kLinkNone) return; // a linked edge: the copy kernel's
  const TracksAlbumCut c = tracks_album_cut(a.s.tracks[t], ln, a.s.row_frames, a.s.src_total, w);
  const u64 *r = edge ? c.fw : c.bk;
  if (r[0] == r[1]) return;
  const TracksEntry &e = c.e;
  const long long extra = (long long)(edge ? w.first + r[1] - (e.lead + e.frames) : e.lead - (w.first + r[0]));
  const u64 base = edge ? e.frames - min_u(e.frames, (u64)a.s.prime_len) : 0;
  const long long org = (long long)(e.lead + base) - (long long)w.first; // base frame 0 as a window frame (in front of it: negative)
  if (!kWin) { // w.first == 0: base frame 0 is row frame org, and the stores count from it
    lpc_edge<kSrc, false>(tracks_album_lds, a.s, e, edge, ch, extra, a.s.rows + ((t * w.stride + (u64)org) * nch + ch), 0, 0, 0);
    return;
  }
  float *y = a.s.rows + (t * w.stride * nch + ch);
  lpc_edge<kSrc, true>(tracks_album_lds, a.s, e, edge, ch, extra, y, org, (long long)r[0], (long long)r[1]);
}

// tracks.hip's unpack4: four consecutive samples of an integer source as integers, from the aligned dwords that cover them.  p is
// the address of the first, mis = p & 3, one value per workgroup.  Reads [p - mis, p - mis + 4 * ceil((mis + bytes) / 4)): no dword
// that does not hold a byte of the group.
template <int kSrc> __device__ __forceinline__ void unpack4(const unsigned char *p, unsigned mis, int *q)
{
  const unsigned *w = reinterpret_cast<const unsigned *>(p - mis); // dword aligned
  const unsigned sh = mis * 8;
  unsigned v[4] = {0u, 0u, 0u, 0u}, d[3];
  if (kSrc == kTracksSrcS16) {
    if (mis) __builtin_memcpy(v, w, 12);
    else __builtin_memcpy(v, w, 8);
    for (int j = 0; j < 2; ++j) d[j] = __builtin_amdgcn_alignbit(v[j + 1], v[j], sh);
    q[0] = (short)d[0];
    q[1] = (int)d[0] >> 16;
    q[2] = (short)d[1];
    q[3] = (int)d[1] >> 16;
  } else if (kSrc == kTracksSrcS24) {
    if (mis) __builtin_memcpy(v, w, 16);
    else __builtin_memcpy(v, w, 12);
    for (int j = 0; j < 3; ++j) d[j] = __builtin_amdgcn_alignbit(v[j + 1], v[j], sh);
    q[0] = (int)(d[0] << 8) >> 8;
    q[1] = (int)(__builtin_amdgcn_alignbit(d[1], d[0], 24) << 8) >> 8;
    q[2] = (int)(__builtin_amdgcn_alignbit(d[2], d[1], 16) << 8) >> 8;
    q[3] = (int)d[2] >> 8;
  } else {
    __builtin_memcpy(q, p, 16); // S32: dword aligned as it is
  }
}

// The n samples of a window row at `row`: [0, zb) zeros, [c0, c1) the run -- sample c0 + j is sample j of s where j < have and zero
// from there -- and [z0, n) zeros; what lies in [zb, c0) and [c1, z0) belongs to the LPC kernel.
template <int kSrc>
__device__ __forceinline__ void album_span(float *row, u64 n, u64 zb, u64 c0, u64 c1, u64 z0, u64 have, const typename Src<kSrc>::T *s, int steps)
{
  constexpr u64 kStep = Src<kSrc>::kStep;
  const unsigned tid = threadIdx.x;
  auto one = [&](u64 k) {
    if (k >= c0 && k < c1) row[k] = k - c0 < have ? tracks_load_sample(kSrc, s, k - c0) : 0.0f;
    else if (k < zb || k >= z0) row[k] = 0.0f;
  };
  u64 head = ((16 - (reinterpret_cast<u64>(row) & 15)) & 15) >> 2; // samples in front of the row's first 16-byte boundary
  if (head > n) head = n;
  const u64 ngroups = (n - head) >> 2;
  // where the groups of this run begin within a dword of the source (the groups are 8, 12 or 16 bytes apart: one value)
  const unsigned mis = kSrc == kTracksSrcS16 || kSrc == kTracksSrcS24 ? (unsigned)(reinterpret_cast<u64>(s) + (head - c0) * kStep) & 3u : 0u;
  if (blockIdx.x == 0) { // head and tail samples, one lane each
    const u64 ntail = n - head - (ngroups << 2);
    if (tid < head) one(tid);
    else if (tid >= 64 && tid < 64 + ntail) one(head + (ngroups << 2) + (tid - 64));
  }
  for (int u = 0; u < steps; ++u) {
    const u64 g = ((u64)blockIdx.x * (unsigned)steps + (unsigned)u) * kThreads + tid;
    if (g >= ngroups) break;
    const u64 k = head + (g << 2);
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (k >= c0 && k + 4 <= c1 && k - c0 + 4 <= have) {
      if (kSrc == kTracksSrcF32) {
        __builtin_memcpy(v, s + (k - c0) * kStep, sizeof(v)); // 16 bytes, dword aligned
      } else {
        constexpr float scale = kSrc == kTracksSrcS16 ? 0x1p-15f : kSrc == kTracksSrcS24 ? 0x1p-23f : 0x1p-31f;
        int q[4];
        unpack4<kSrc>(reinterpret_cast<const unsigned char *>(s + (k - c0) * kStep), mis, q);
        for (int j = 0; j < 4; ++j) v[j] = (float)q[j] * scale;
      }
    } else if ((k >= zb && k + 4 <= c0) || (k >= c1 && k + 4 <= z0)) continue; // extension frames only
    else if (k + 4 > zb && k < z0) { // a group across two regions, or frames of the run that a wrong table puts past the source
      for (int j = 0; j < 4; ++j) one(k + j);
      continue;
    }
    __builtin_memcpy(__builtin_assume_aligned(row + k, 16), v, sizeof(v));
  }
}

template <int kSrc> __global__ __launch_bounds__(kThreads) void tracks_album_copy_kernel(TracksAlbumArgs a, TracksWindow w, int t0, int steps)
{
  typedef typename Src<kSrc>::T T;
  constexpr u64 kStep = Src<kSrc>::kStep;
  const u64 t = (u64)(t0 + (int)blockIdx.y), nch = (u64)a.s.nch;
  const TracksAlbumCut c = tracks_album_cut(a.s.tracks[t], a.links[t], a.s.row_frames, a.s.src_total, w);
  const T *s = static_cast<const T *>(a.s.src) + c.src_frame * nch * kStep; // the sample that window sample cp[0] * nch is a copy of
  album_span<kSrc>(a.s.rows + t * w.stride * nch, w.frames * nch, c.zb[1] * nch, c.cp[0] * nch, c.cp[1] * nch, c.z[0] * nch, c.readable * nch, s,
                   steps);
}

template <int kSrc> hipError_t stage_typed(hipStream_t stream, const TracksAlbumArgs &a, const TracksWindow &w)
{
  // copy and zero fill: kAlbumSteps steps of 256 groups per workgroup, more only to stay inside the grid limit
  const u64 groups = (w.frames * (u64)a.s.nch + 3) / 4 + 1; // (+1: the head can move the last samples into one more group)
  u64 steps = kAlbumSteps;
  while ((groups + steps * kThreads - 1) / (steps * kThreads) > 0x7fffffffull) steps *= 2;
  const unsigned gx = (unsigned)((groups + steps * kThreads - 1) / (steps * kThreads));
  for (int t0 = 0; t0 < a.s.ntracks; t0 += 32768) { // grid.y is a 16-bit count
    const int nt = a.s.ntracks - t0 < 32768 ? a.s.ntracks - t0 : 32768;
    hipLaunchKernelGGL(tracks_album_copy_kernel<kSrc>, dim3(gx, (unsigned)nt), dim3(kThreads), 0, stream, a, w, t0, (int)steps);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  // the extrapolated edges of every (track, channel)
  static DynLdsOnce once, once_window; // (one per instance)
  const bool whole = w.first == 0 && w.frames == a.s.row_frames;
  const void *fn = whole ? reinterpret_cast<const void *>(&tracks_album_lpc_kernel<kSrc, false>)
                         : reinterpret_cast<const void *>(&tracks_album_lpc_kernel<kSrc, true>);
  const hipError_t e = (whole ? once : once_window).set(fn, int(sizeof(LpcShared) + kLpcLdsFrames * sizeof(float)));
  if (e != hipSuccess) return e;
  const size_t lds = sizeof(LpcShared) + size_t(a.s.prime_len) * sizeof(float);
  const dim3 grid((unsigned)((long long)a.s.ntracks * a.s.nch * 2));
  if (whole) hipLaunchKernelGGL((tracks_album_lpc_kernel<kSrc, false>), grid, dim3(64), lds, stream, a, w);
  else hipLaunchKernelGGL((tracks_album_lpc_kernel<kSrc, true>), grid, dim3(64), lds, stream, a, w);
  return hipGetLastError();
}

} // namespace

hipError_t launch_tracks_stage_album(hipStream_t stream, const TracksAlbumArgs &a, const TracksWindow &w)
{
  switch (a.s.src_kind) {
  case kTracksSrcF32: return stage_typed<kTracksSrcF32>(stream, a, w);
  case kTracksSrcS16: return stage_typed<kTracksSrcS16>(stream, a, w);
  case kTracksSrcS24: return stage_typed<kTracksSrcS24>(stream, a, w);
  case kTracksSrcS32: return stage_typed<kTracksSrcS32>(stream, a, w);
  default: return hipErrorInvalidValue; // a missing kernel is an error, never another kernel
  }
}

void tracks_stage_album_host(const TracksAlbumArgs &a, const TracksWindow &w)
{
  const u64 nch = (u64)a.s.nch, step = (u64)tracks_src_bytes(a.s.src_kind);
  for (u64 t = 0; t < (u64)a.s.ntracks; ++t) {
    const TracksAlbumCut c = tracks_album_cut(a.s.tracks[t], a.links[t], a.s.row_frames, a.s.src_total, w);
    float *row = a.s.rows + t * w.stride * nch;
    const unsigned char *s = static_cast<const unsigned char *>(a.s.src) + c.src_frame * nch * step;
    for (u64 k = c.zb[0] * nch; k < c.zb[1] * nch; ++k) row[k] = 0.0f;
    for (u64 k = c.cp[0] * nch, j = 0; k < c.cp[1] * nch; ++k, ++j) row[k] = j < c.readable * nch ? tracks_load_sample(a.s.src_kind, s, j) : 0.0f;
    for (u64 k = c.z[0] * nch; k < c.z[1] * nch; ++k) row[k] = 0.0f;
  }
}

} // namespace rsmp
