// Ragged track batches: the kernels around a batch handle whose streams hold tracks of unequal length.
//
// Stage (RRX_tracks_stage_device_samples): packed tracks [sum of frames][nch] -> rows [ntracks][row_frames][nch].  Row t is
//   [0, lead)                      backward LPC extension from the track's first min(frames, prime_len) frames   tracks_lpc_kernel
//   [lead, lead + frames)          the track                                                                       tracks_copy_kernel
//   [lead + frames, ext)           forward LPC extension from its last min(frames, prime_len) frames             tracks_lpc_kernel
//   [ext, row_frames)              zeros: the track's drain                                         tracks_copy_kernel
// with ext = lead + frames + lead.  tracks_lpc_kernel is one 64-lane workgroup per (track, channel, edge) around lpc_channel
// (lpc_body.hpp), the body of lpc.hip's kernel: the two edges of a channel are sums over different base frames read from the
// packed source, so they run side by side.  tracks_copy_kernel is uniform, bandwidth-bound work: grid = (chunk of a row, track),
// every row has row_frames * nch samples to look at.  A row is cut into a head of 0..3 samples up to the first 16-byte boundary
// of the DESTINATION, groups of 4 samples (one lane each: 16 bytes loaded, which needs dword alignment only, 16 aligned bytes
// stored) and a tail of 0..3 samples; a group that straddles two regions goes sample by sample.  The two kernels write disjoint
// frames and read only the source, so their order does not matter.
// Both are templates on what the packed source holds (TracksSrc, tracks.hpp): float32, or S16 / packed 3-byte S24 / S32 PCM, which
// is converted on load by tracks_load_sample's rule; everything about the rows is the same.  An integer group is 8, 12 or 16 source
// bytes at sample alignment (tracks are adjacent, so for S24 at any byte offset): the lane loads the 2 to 4 aligned dwords that
// cover them, realigns by the track's misalignment (one value per workgroup), unpacks and converts (unpack4).  So the group path may
// read the whole aligned dword that holds the first or the last byte of the source, and nothing further out; the sample-by-sample
// paths and the LPC loads read exactly their samples' bytes.
//
// Output stage (RRX_tracks_finish_device): finish_sample (finish.hpp) per track, finish.hip's shape with a per-track prologue --
// grid = (chunk of a row, track), head / groups of 4 / tail decided per track from where ITS bytes begin in the packed
// destination, statistics in registers and LDS where lcm(4, nch) <= 1024.  The grid is sized for a full row; the workgroups past
// a shorter track's end exit at once.
//
// Windows (RRX_tracks_stage_window_device / RRX_tracks_finish_window_device; DESIGN.md 11, "Windows"): the same passes on frames
// [first, first + frames) of rows that exist nowhere as a whole, so that a batch runs in memory proportional to the window.  Each
// kernel has a window form with the same body (copy_span, lpc_edge, finish_span) behind another prologue: the regions of the row,
// or the track's slice, cut to the window by tracks_stage_cut / tracks_finish_cut (tracks.hpp).  The copy and finish grids are
// sized by the window; the LPC grid is not (see tracks_lpc_window_kernel).
//
// The table is the caller's, on the device, and is not validated: every value taken from it is clamped first (tracks_entry and
// tracks_slice, tracks.hpp, and the cut functions built on them), so
// a wrong table gives wrong samples and never an access outside the source, the track's own row or window, or the destination.
#include "tracks.hpp"

#include "finish.hpp"
#include "lpc_body.hpp"

namespace rsmp {
namespace {

typedef unsigned long long u64;

constexpr int kThreads = 256, kSpanMax = kThreads * 4;

__device__ __forceinline__ u64 min_u(u64 x, u64 y) { return x < y ? x : y; }

// Track t's input side, clamped (tracks_entry, tracks.hpp)
__device__ __forceinline__ TracksEntry entry_of(const TracksStageArgs &a, u64 t) { return tracks_entry(a.tracks[t], a.row_frames, a.src_total); }

// The packed source as the kernels address it: floats as floats (the float instances are the kernels they were before the
// integer sources came), integer PCM as bytes, kStep of them a sample
template <int kSrc> struct Src {
  typedef unsigned char T;
  static constexpr u64 kStep = tracks_src_bytes(kSrc);
};
template <> struct Src<kTracksSrcF32> {
  typedef float T;
  static constexpr u64 kStep = 1;
};

// One edge (0: backward, 1: forward) of channel ch of a track: `extra` frames of extrapolation, counted outwards from the track's
// edge.  Extrapolated frame i (lpc_channel's count, from base frame 0) is frame k = org + i of y; kWin: stored only where lo <= k < hi.
template <int kSrc, bool kWin>
__device__ __forceinline__ void lpc_edge(unsigned char *lds, const TracksStageArgs &a, const TracksEntry &e, int edge, u64 ch, long long extra,
                                         float *y, long long org, long long lo, long long hi)
{
  typedef typename Src<kSrc>::T T;
  const int lane = threadIdx.x, nch = a.nch;
  const long long n = (long long)min_u(e.frames, (u64)a.prime_len);      // base frames: the track's first n, or its last n
  const u64 base = edge ? e.frames - (u64)n : 0;
  const long long readable = e.have > base ? (long long)(e.have - base) : 0; // (all n of them, unless the table is wrong)
  // base frame 0 of this channel: strided single samples, read once (into LDS) through tracks_load_sample
  const T *x = static_cast<const T *>(a.src) + ((e.first + min_u(base, e.have)) * nch + ch) * Src<kSrc>::kStep;
  if (n <= kLpcMaxOrder) { // no table of RRX_tracks_plan: a lead means more than 64 frames.  Zeros, so that the row is written all the same.
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

template <int kSrc> __global__ __launch_bounds__(64) void tracks_lpc_kernel(TracksStageArgs a)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char tracks_lds[];
  const int edge = blockIdx.x & 1, nch = a.nch;
  const u64 t = (blockIdx.x >> 1) / (unsigned)nch, ch = (blockIdx.x >> 1) % (unsigned)nch;
  const TracksEntry e = entry_of(a, t);
  const long long extra = (long long)(edge ? e.fwd : e.lead);
  if (!extra) return;
  const u64 base = edge ? e.frames - min_u(e.frames, (u64)a.prime_len) : 0;
  float *y = a.rows + ((t * a.row_frames + e.lead + base) * nch + ch);
  lpc_edge<kSrc, false>(tracks_lds, a, e, edge, ch, extra, y, 0, 0, 0);
}

// The window form: same grid, because the table is on the device and the host cannot pick the workgroups that have work.  One whose
// extension does not meet the window returns before it loads a base frame.  The recursion is serial from the track's edge outwards,
// so one that does starts there whatever the window is, runs as far as the window's far end asks for, and stores what lies inside.
template <int kSrc> __global__ __launch_bounds__(64) void tracks_lpc_window_kernel(TracksStageArgs a, TracksWindow w)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char tracks_lds[];
  const int edge = blockIdx.x & 1, nch = a.nch;
  const u64 t = (blockIdx.x >> 1) / (unsigned)nch, ch = (blockIdx.x >> 1) % (unsigned)nch;
  const TracksStageCut c = tracks_stage_cut(a.tracks[t], a.row_frames, a.src_total, w);
  const u64 *r = edge ? c.fw : c.bk;
  if (r[0] == r[1]) return;
  const TracksEntry &e = c.e;
  // in row frames: the backward recursion comes down from lead - 1 to the window's first extension frame, the forward one goes up
  // from lead + frames to its last
  const long long extra = (long long)(edge ? w.first + r[1] - (e.lead + e.frames) : e.lead - (w.first + r[0]));
  const u64 base = edge ? e.frames - min_u(e.frames, (u64)a.prime_len) : 0;
  // base frame 0 is row frame lead + base, which is window frame org (before the window: negative)
  const long long org = (long long)(e.lead + base) - (long long)w.first;
  float *y = a.rows + (t * w.stride * nch + ch); // window frame 0 of this channel
  lpc_edge<kSrc, true>(tracks_lds, a, e, edge, ch, extra, y, org, (long long)r[0], (long long)r[1]);
}

// Four consecutive samples of an integer source as integers, from the aligned dwords that cover them: the inverse of Pack<bits>
// (below).  p is the address of the first sample, mis = p & 3 -- the same for every group of a track, because a group is 8, 12 or
// 16 bytes further than the one before, and so decided once per workgroup: the branches on it are wave-uniform.  Reads
// [p - mis, p - mis + 4 * ceil((mis + bytes) / 4)): no dword that does not hold a byte of the group.
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

// The n samples at `row` (a row, or the window of one).  [c0, c1) is the track: sample c0 + j is sample j of s where j < have and
// zero from there; [z0, n) are zeros; what lies in front of c0 and between c1 and z0 belongs to the LPC kernel.
template <int kSrc>
__device__ __forceinline__ void copy_span(float *row, u64 n, u64 c0, u64 c1, u64 z0, u64 have, const typename Src<kSrc>::T *s, int steps)
{
  constexpr u64 kStep = Src<kSrc>::kStep;
  const unsigned tid = threadIdx.x;
  auto one = [&](u64 k) {
    if (k >= c0 && k < c1) row[k] = k - c0 < have ? tracks_load_sample(kSrc, s, k - c0) : 0.0f;
    else if (k >= z0) row[k] = 0.0f;
  };
  u64 head = ((16 - (reinterpret_cast<u64>(row) & 15)) & 15) >> 2; // samples in front of the row's first 16-byte boundary
  if (head > n) head = n;
  const u64 ngroups = (n - head) >> 2;
  // where the groups of this track begin within a dword of the source (integer sources; see unpack4)
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
      } else { // the aligned dwords that cover the group, realigned, unpacked, sign-extended, converted
        constexpr float scale = kSrc == kTracksSrcS16 ? 0x1p-15f : kSrc == kTracksSrcS24 ? 0x1p-23f : 0x1p-31f;
        int q[4];
        unpack4<kSrc>(reinterpret_cast<const unsigned char *>(s + (k - c0) * kStep), mis, q);
        for (int j = 0; j < 4; ++j) v[j] = (float)q[j] * scale;
      }
    } else if (k + 4 <= c0 || (k >= c1 && k + 4 <= z0)) continue; // extension frames only
    else if (k < z0) { // a group across two regions, or the track's frames that a wrong table puts past the source
      for (int j = 0; j < 4; ++j) one(k + j);
      continue;
    }
    __builtin_memcpy(__builtin_assume_aligned(row + k, 16), v, sizeof(v));
  }
}

template <int kSrc> __global__ __launch_bounds__(kThreads) void tracks_copy_kernel(TracksStageArgs a, int t0, int steps)
{
  typedef typename Src<kSrc>::T T;
  constexpr u64 kStep = Src<kSrc>::kStep;
  const u64 t = (u64)(t0 + (int)blockIdx.y), nch = (u64)a.nch, n = a.row_frames * nch; // n: samples of a row
  const TracksEntry e = entry_of(a, t);
  // in samples of the row: [c0, c1) is the track, [z0, n) the zeros; what lies between belongs to tracks_lpc_kernel
  const u64 c0 = e.lead * nch, c1 = c0 + e.frames * nch, z0 = c1 + e.fwd * nch, have = e.have * nch;
  const T *s = static_cast<const T *>(a.src) + e.first * nch * kStep; // sample j of the track, j < have, is kStep * j further
  copy_span<kSrc>(a.rows + t * n, n, c0, c1, z0, have, s, steps);
}

// The window form: the grid covers the window's samples, and the regions are the row's cut to the window (tracks_stage_cut).  Head,
// groups and tail follow the alignment of the WINDOW row, per track; the misalignment of an integer source is still one value per
// workgroup, because the groups of a window row are a whole number of groups apart as those of a row are.
template <int kSrc> __global__ __launch_bounds__(kThreads) void tracks_copy_window_kernel(TracksStageArgs a, TracksWindow w, int t0, int steps)
{
  typedef typename Src<kSrc>::T T;
  constexpr u64 kStep = Src<kSrc>::kStep;
  const u64 t = (u64)(t0 + (int)blockIdx.y), nch = (u64)a.nch;
  const TracksStageCut c = tracks_stage_cut(a.tracks[t], a.row_frames, a.src_total, w);
  const T *s = static_cast<const T *>(a.src) + c.src_frame * nch * kStep; // the sample that window sample cp[0] * nch is a copy of
  copy_span<kSrc>(a.rows + t * w.stride * nch, w.frames * nch, c.cp[0] * nch, c.cp[1] * nch, c.z[0] * nch, c.readable * nch, s, steps);
}

// ---------------------------------------------------------------------------------------------------------------- output stage

__device__ __forceinline__ u64 peak_bits(double a) { return (u64)__double_as_longlong(a); }

// bits of a non-negative double order as unsigned integers (a NaN, sign cleared by fabs, lies above +inf and stays)
__device__ __forceinline__ void global_stats(const TracksFinishArgs &a, u64 c, u64 pk, u64 cl)
{
  if (a.peak && pk) {
    u64 *p = reinterpret_cast<u64 *>(a.peak) + c;
    if (pk > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, pk); // the value only ever grows
  }
  if (a.clipped && cl) atomicAdd(a.clipped + c, cl);
}

// four consecutive quantised samples as whole dwords
template <int kBits> struct Pack;
template <> struct Pack<15> {
  static constexpr int kBytes = 2, kWords = 2;
  static __device__ __forceinline__ void words(const int *q, unsigned *w)
  {
    w[0] = ((unsigned)q[0] & 0xffffu) | ((unsigned)q[1] << 16);
    w[1] = ((unsigned)q[2] & 0xffffu) | ((unsigned)q[3] << 16);
  }
};
template <> struct Pack<23> {
  static constexpr int kBytes = 3, kWords = 3;
  static __device__ __forceinline__ void words(const int *q, unsigned *w)
  {
    const unsigned a = (unsigned)q[0] & 0xffffffu, b = (unsigned)q[1] & 0xffffffu, c = (unsigned)q[2] & 0xffffffu, d = (unsigned)q[3] & 0xffffffu;
    w[0] = a | (b << 24);
    w[1] = (b >> 8) | (c << 16);
    w[2] = (c >> 16) | (d << 8);
  }
};
template <> struct Pack<31> {
  static constexpr int kBytes = 4, kWords = 4;
  static __device__ __forceinline__ void words(const int *q, unsigned *w)
  {
    for (int j = 0; j < 4; ++j) w[j] = (unsigned)q[j];
  }
};

// S: float or double rows.  kWrite = false: measure only.  kReg: statistics in registers and LDS (finish.hip).
// Track t is stream t of RRX_finish_device: gain[t], statistics and dither channel t * nch + ch, frame 0 = its first output frame.
// finish_span: n samples of track t from src to dst (kWrite); the first of them belongs to frame i0 of the track.
template <typename S, int kBits, bool kWrite, bool kReg>
__device__ __forceinline__ void finish_span(const TracksFinishArgs &a, u64 t, const S *src, unsigned char *dst, u64 n, u64 i0, int span, unsigned fps,
                                            int steps, u64 *sh_peak, unsigned *sh_clip)
{
  using P = Pack<kBits>;
  const unsigned tid = threadIdx.x;
  const unsigned nch = (unsigned)a.nch;
  const u64 cbase = t * nch;
  const bool has_gain = a.gain != nullptr, dither = a.dither != 0;

  // the track's head: samples in front of the first dword boundary of the destination
  const u64 addr = reinterpret_cast<u64>(dst);
  unsigned head = !kWrite ? 0u : kBits == 15 ? (unsigned)(addr >> 1) & 1u : kBits == 23 ? (unsigned)addr & 3u : 0u;
  if (head > n) head = (unsigned)n;
  const u64 ngroups = (n - head) >> 2;
  const unsigned gps = (unsigned)span >> 2; // groups (= lanes at work) per step
  const u64 step0 = (u64)blockIdx.x * (unsigned)steps;
  if (blockIdx.x != 0 && step0 * gps >= ngroups) return; // past the end of a track shorter than the row
  const double gain = has_gain ? a.gain[t] : 1.0;

  if (kReg) {
    for (unsigned c = tid; c < nch; c += kThreads) {
      sh_peak[c] = 0;
      sh_clip[c] = 0;
    }
    __syncthreads();
  }

  // head and tail samples: workgroup 0, one lane each, channel and frame by division
  if (blockIdx.x == 0) {
    const unsigned ntail = (unsigned)(n - head - (ngroups << 2));
    const bool is_head = tid < head, is_tail = tid >= 64 && tid < 64 + ntail;
    if (is_head || is_tail) {
      const u64 k = is_head ? tid : head + (ngroups << 2) + (tid - 64);
      const u64 fr = k / nch;
      const unsigned ch = (unsigned)(k - fr * nch);
      const FinishSample r = finish_sample<kBits>((double)src[k], has_gain, gain, dither, a.seed, i0 + fr, cbase + ch);
      if (kWrite) finish_store_bytes<kBits>(dst + k * P::kBytes, r.q);
      if (kReg) {
        atomicMax(&sh_peak[ch], peak_bits(r.a));
        if (r.clip) atomicAdd(&sh_clip[ch], 1u);
      } else {
        global_stats(a, cbase + ch, peak_bits(r.a), r.clip ? 1ull : 0ull);
      }
    }
  }

  if (tid < gps) {
    // kReg: the lane's 4 samples are samples head + 4 tid + j of every step's span, a whole number of frames (fps) further each step
    unsigned chj[4];
    u64 frj[4], pk[4] = {0, 0, 0, 0};
    unsigned cl[4] = {0, 0, 0, 0};
    if (kReg) {
      const unsigned k0 = head + 4 * tid, f0 = k0 / nch;
      unsigned ch = k0 - f0 * nch;
      u64 fr = i0 + f0 + step0 * fps;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        chj[j] = ch;
        frj[j] = fr;
        if (++ch == nch) ch = 0, ++fr;
      }
    }
    for (int u = 0; u < steps; ++u) {
      const u64 gi = (step0 + u) * gps + tid;
      if (gi >= ngroups) break;
      const u64 k = head + (gi << 2);
      S x[4];
      __builtin_memcpy(x, src + k, sizeof(x)); // 16-byte loads: one for float, two for double
      if (!kReg) {
        const u64 f0 = k / nch;
        unsigned ch = (unsigned)(k - f0 * nch);
        u64 fr = i0 + f0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          chj[j] = ch;
          frj[j] = fr;
          if (++ch == nch) ch = 0, ++fr;
        }
      }
      int q[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const FinishSample r = finish_sample<kBits>((double)x[j], has_gain, gain, dither, a.seed, frj[j], cbase + chj[j]);
        q[j] = r.q;
        if (kReg) {
          const u64 b = peak_bits(r.a);
          pk[j] = b > pk[j] ? b : pk[j];
          cl[j] += r.clip ? 1u : 0u;
          frj[j] += fps;
        } else {
          global_stats(a, cbase + chj[j], peak_bits(r.a), r.clip ? 1ull : 0ull);
        }
      }
      if (kWrite) {
        unsigned w[P::kWords];
        P::words(q, w);
        __builtin_memcpy(reinterpret_cast<unsigned *>(dst + k * P::kBytes), w, sizeof(w)); // dword aligned: that is what the head is for
      }
    }
    if (kReg) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (pk[j]) atomicMax(&sh_peak[chj[j]], pk[j]);
        if (cl[j]) atomicAdd(&sh_clip[chj[j]], cl[j]);
      }
    }
  }

  if (kReg) {
    __syncthreads();
    for (unsigned c = tid; c < nch; c += kThreads) global_stats(a, cbase + c, sh_peak[c], sh_clip[c]);
  }
}

template <typename S, int kBits, bool kWrite, bool kReg>
__global__ __launch_bounds__(kThreads) void tracks_finish_kernel(TracksFinishArgs a, int t0, int span, unsigned fps, int steps)
{
  __shared__ u64 sh_peak[kReg ? kFinishLdsChannels : 1];
  __shared__ unsigned sh_clip[kReg ? kFinishLdsChannels : 1];
  const unsigned nch = (unsigned)a.nch;
  const u64 t = (u64)(t0 + (int)blockIdx.y);
  // the track's slice, clamped: inside its row, and (when written) inside the destination
  const TracksSlice s = tracks_slice(a.tracks[t], a.row_frames, a.dst_total, kWrite);
  const S *src = static_cast<const S *>(a.src) + (t * a.row_frames + s.of) * nch;
  unsigned char *dst = kWrite ? static_cast<unsigned char *>(a.dst) + s.df * nch * Pack<kBits>::kBytes : nullptr;
  finish_span<S, kBits, kWrite, kReg>(a, t, src, dst, s.frames * nch, 0, span, fps, steps, sh_peak, sh_clip);
}

// The window form: a.src holds frames [w.first, w.first + w.frames) of every output row, pitch w.stride.  The part of the track's
// slice inside the window is processed (tracks_finish_cut); head, groups and tail follow where ITS bytes begin in the destination,
// and the frame number finish_sample gets counts from the track's first output frame, as in the whole-row kernel.
template <typename S, int kBits, bool kWrite, bool kReg>
__global__ __launch_bounds__(kThreads) void tracks_finish_window_kernel(TracksFinishArgs a, TracksWindow w, int t0, int span, unsigned fps, int steps)
{
  __shared__ u64 sh_peak[kReg ? kFinishLdsChannels : 1];
  __shared__ unsigned sh_clip[kReg ? kFinishLdsChannels : 1];
  const unsigned nch = (unsigned)a.nch;
  const u64 t = (u64)(t0 + (int)blockIdx.y);
  const TracksFinishCut c = tracks_finish_cut(a.tracks[t], a.row_frames, a.dst_total, kWrite, w);
  const S *src = static_cast<const S *>(a.src) + (t * w.stride + c.w0) * nch;
  unsigned char *dst = kWrite ? static_cast<unsigned char *>(a.dst) + c.dst_frame * nch * Pack<kBits>::kBytes : nullptr;
  finish_span<S, kBits, kWrite, kReg>(a, t, src, dst, (c.w1 - c.w0) * nch, c.index, span, fps, steps, sh_peak, sh_clip);
}

u64 gcd_u(u64 x, u64 y)
{
  while (y) {
    const u64 r = x % y;
    x = y;
    y = r;
  }
  return x;
}

// w: the window form, or null
template <typename S, int kBits, bool kWrite>
hipError_t finish_typed(hipStream_t stream, const TracksFinishArgs &a, const TracksWindow *w)
{
  const u64 nch = (u64)a.nch, lcm4 = nch / gcd_u(nch, 4) * 4, n = (w ? w->frames : a.row_frames) * nch; // n: the most samples a track can have
  static_assert(kFinishLdsChannels >= kSpanMax, "nch <= lcm(4, nch) <= kSpanMax has to fit the LDS table");
  const bool reg = lcm4 <= (u64)kSpanMax;
  const int span = reg ? int(kSpanMax / lcm4 * lcm4) : kSpanMax;
  const unsigned fps = reg ? unsigned(span / a.nch) : 0u;
  const u64 row_steps = ((n + 3) / 4 + span / 4 - 1) / (span / 4);
  // steps per workgroup as in finish.hip: about 16 workgroups per CU, at most 32 steps, more only to stay inside the grid limit
  // (n < 2^60, so a workgroup sees fewer than 2^31 samples, which its 32-bit clip counts hold)
  u64 steps = row_steps * (u64)a.ntracks / 4096;
  steps = steps < 1 ? 1 : steps > 32 ? 32 : steps;
  while ((row_steps + steps - 1) / steps > 0x7fffffffull) steps *= 2;
  const unsigned gx = (unsigned)((row_steps + steps - 1) / steps);
  for (int t0 = 0; t0 < a.ntracks; t0 += 32768) { // grid.y is a 16-bit count
    const int nt = a.ntracks - t0 < 32768 ? a.ntracks - t0 : 32768;
    const dim3 grid(gx ? gx : 1, (unsigned)nt), block(kThreads);
    if (w && reg) hipLaunchKernelGGL((tracks_finish_window_kernel<S, kBits, kWrite, true>), grid, block, 0, stream, a, *w, t0, span, fps, (int)steps);
    else if (w) hipLaunchKernelGGL((tracks_finish_window_kernel<S, kBits, kWrite, false>), grid, block, 0, stream, a, *w, t0, span, fps, (int)steps);
    else if (reg) hipLaunchKernelGGL((tracks_finish_kernel<S, kBits, kWrite, true>), grid, block, 0, stream, a, t0, span, fps, (int)steps);
    else hipLaunchKernelGGL((tracks_finish_kernel<S, kBits, kWrite, false>), grid, block, 0, stream, a, t0, span, fps, (int)steps);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

template <typename S> hipError_t finish_src(hipStream_t stream, const TracksFinishArgs &a, const TracksWindow *w)
{
  if (!a.dst) return finish_typed<S, 31, false>(stream, a, w);
  switch (a.bits) {
  case 15: return finish_typed<S, 15, true>(stream, a, w);
  case 23: return finish_typed<S, 23, true>(stream, a, w);
  default: return finish_typed<S, 31, true>(stream, a, w);
  }
}

// w: the window form, or null
template <int kSrc> hipError_t stage_typed(hipStream_t stream, const TracksStageArgs &a, const TracksWindow *w)
{
  // copy and zero fill: 8 steps of 256 groups (32 KiB written) per workgroup, more only to stay inside the grid limit
  const u64 groups = ((w ? w->frames : a.row_frames) * (u64)a.nch + 3) / 4 + 1; // (+1: the head can move the last samples into one more group)
  u64 steps = 8;
  while ((groups + steps * kThreads - 1) / (steps * kThreads) > 0x7fffffffull) steps *= 2;
  const unsigned gx = (unsigned)((groups + steps * kThreads - 1) / (steps * kThreads));
  for (int t0 = 0; t0 < a.ntracks; t0 += 32768) { // grid.y is a 16-bit count
    const int nt = a.ntracks - t0 < 32768 ? a.ntracks - t0 : 32768;
    if (w) hipLaunchKernelGGL(tracks_copy_window_kernel<kSrc>, dim3(gx, (unsigned)nt), dim3(kThreads), 0, stream, a, *w, t0, (int)steps);
    else hipLaunchKernelGGL(tracks_copy_kernel<kSrc>, dim3(gx, (unsigned)nt), dim3(kThreads), 0, stream, a, t0, (int)steps);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  // the two extensions of every (track, channel)
  static DynLdsOnce once, once_window; // (one per instance)
  const void *fn = w ? reinterpret_cast<const void *>(&tracks_lpc_window_kernel<kSrc>) : reinterpret_cast<const void *>(&tracks_lpc_kernel<kSrc>);
  const hipError_t e = (w ? once_window : once).set(fn, int(sizeof(LpcShared) + kLpcLdsFrames * sizeof(float)));
  if (e != hipSuccess) return e;
  const size_t lds = sizeof(LpcShared) + size_t(a.prime_len) * sizeof(float);
  const dim3 grid((unsigned)((long long)a.ntracks * a.nch * 2));
  if (w) hipLaunchKernelGGL(tracks_lpc_window_kernel<kSrc>, grid, dim3(64), lds, stream, a, *w);
  else hipLaunchKernelGGL(tracks_lpc_kernel<kSrc>, grid, dim3(64), lds, stream, a);
  return hipGetLastError();
}

} // namespace

namespace {

hipError_t stage_kind(hipStream_t stream, const TracksStageArgs &a, const TracksWindow *w)
{
  switch (a.src_kind) {
  case kTracksSrcF32: return stage_typed<kTracksSrcF32>(stream, a, w);
  case kTracksSrcS16: return stage_typed<kTracksSrcS16>(stream, a, w);
  case kTracksSrcS24: return stage_typed<kTracksSrcS24>(stream, a, w);
  case kTracksSrcS32: return stage_typed<kTracksSrcS32>(stream, a, w);
  default: return hipErrorInvalidValue; // a missing kernel is an error, never another kernel
  }
}

} // namespace

hipError_t launch_tracks_stage(hipStream_t stream, const TracksStageArgs &a) { return stage_kind(stream, a, nullptr); }
hipError_t launch_tracks_stage_window(hipStream_t stream, const TracksStageArgs &a, const TracksWindow &w) { return stage_kind(stream, a, &w); }

hipError_t launch_tracks_finish(hipStream_t stream, const TracksFinishArgs &a)
{
  return a.src_double ? finish_src<double>(stream, a, nullptr) : finish_src<float>(stream, a, nullptr);
}

hipError_t launch_tracks_finish_window(hipStream_t stream, const TracksFinishArgs &a, const TracksWindow &w)
{
  return a.src_double ? finish_src<double>(stream, a, &w) : finish_src<float>(stream, a, &w);
}

} // namespace rsmp
