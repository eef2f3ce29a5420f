// True-peak limiter for device-resident frames ("Limiter"): RRX_limit_device and RRX_tracks_limit_device.  The
// arithmetic is limit.hpp's and true_peak.hpp's, shared with the host twin at the end of this file.
//
// A row is one stream of RRX_limit_device or one track's slice of RRX_tracks_limit_device (clamped by tracks_slice); it has N
// frames, D = taps - 1, L = lookahead, H = hold, and two arrays in the work buffer: r[F], F in [0, N + D), and m[j], j in
// [0, N + L - 1), where m[j] is the header's m[k] with k = j - (L - 1).  Three launches, grid = (pieces of a row, stream), every
// kernel walking the pieces a full grid leaves over:
//   detect   one lane per detector frame F, 256 to a workgroup, which stages their gained samples in LDS behind a halo of D frames,
//            up to 15 channels at a time: per channel the taps from LDS, true_peak_frame, the maximum with |g[F]|; then
//            r[F] = limit_reduction.  (The first form read its taps from global memory, one lane per frame looping over the
//            channels, and took 2.1 times the true-peak pass on stereo rows and more on wide ones: DESIGN.md 10.)
//   window   m[j] = min r[F] over F in [j - (L - 1) - H, j + D], 1.0 outside the row: a workgroup loads a tile of r into LDS and
//            doubles the width of the minimum held in every entry (a pass per power of two below the window, read - barrier -
//            write - barrier), then one minimum of two overlapping entries gives any width.  A minimum is exact in any order.
//            A tile holds kLimitMinTile entries, of which L + H + D - 1 are halo: kLimitMinTile - (L + H + D - 1) values of m.
//   apply    kLimitLaneFrames consecutive frames to a lane, kLimitApplyFrames to a workgroup: every entry of the LDS tile of m is
//            read once and added to the sums of the frames it belongs to (limit_smooth_frames), the gains go to LDS, then the
//            workgroup's samples y = g * s in the order they lie in memory, a lane per sample.  The statistics are merged in LDS
//            and leave as at most one atomic per (workgroup, stream, statistic), issued only where it changes the value.
// Nothing outside the rows is read; nothing but the rows' frames of the destination, the work buffer and the two result arrays is
// written.  In place the apply kernel reads a sample in the lane that writes it, after the detector is done with the rows.
//
// The window form (RRX_tracks_limit_window_device, DESIGN.md 11 "Windows with the limiter") runs the same three bodies on a
// sub-range of every row: with [lo, hi) the window's cut of the slice, the detector covers F in [max(0, lo - (L - 1) - H),
// min(N + D, hi + L - 1 + D)), the minimum the entries j in [lo, hi + L - 1), the product the frames [lo, hi); r and m are
// stored from their first entry of that range.  Row (below) carries the ranges, and for a whole row they are constants that
// fold away: every kernel is a template over kWin, instantiated once for each form, so the two cannot drift apart.  (The window
// is a kernel argument of its own behind the others, all zeros for whole rows: their arguments stay where they were.)
#include "limit.hpp"

#include <cstring>

namespace rsmp {
namespace {

constexpr int kThreads = 256;
constexpr int kMinPerLane = kLimitMinTile / kThreads;
constexpr int kDetectTile = 4096; // doubles of LDS the detector stages gained samples in
constexpr int kApplyPitch = (kLimitApplyFrames + kLimitMaxLookahead - 1 + kLimitLaneFrames - 1) / kLimitLaneFrames;
static_assert(kLimitMinTile % kThreads == 0 && kLimitApplyFrames == kThreads * kLimitLaneFrames, "whole passes over the tiles");
static_assert(kLimitMaxLookahead + kLimitMaxHold + kTpMaxTaps - 1 < kLimitMinTile, "a tile holds the widest window and a value of m");

// one row of work
struct Row {
  unsigned long long src_at, dst_at; // sample 0 of the row's frame 0, in samples from a.src / a.dst
  unsigned long long frames;
  double *r, *m;
  double gain;
  bool has_gain;
  // what of the row this call works on (a whole row: lo = fa = 0, hi = frames, fb = frames + D, every frame readable)
  unsigned long long lo, hi; // the frames that are emitted; m[0] is entry j = lo
  unsigned long long fa, fb; // the detector frames F that are evaluated; r[0] is r[fa]
  unsigned long long s_lo, s_hi; // the frames the source holds: the others read as +0.0
};

template <bool kWin> __host__ __device__ __forceinline__ Row row_of(const LimitArgs &a, const LimitWindow &w, unsigned long long s)
{
  Row r;
  const unsigned long long nch = (unsigned long long)a.nch;
  if (kWin) {
    // the slice, clamped into the virtual row; the sums below stay under 2 * row_frames + 2^14
    const TracksSlice sl = tracks_slice(a.tracks[s], a.frames, 0, false);
    const unsigned long long end = w.win_first + w.win_frames, top = sl.of + sl.frames, buf_end = w.buf_first + w.buf_frames;
    const unsigned long long lo = sl.of > w.win_first ? sl.of : w.win_first, hi = top < end ? top : end;
    const unsigned long long D = (unsigned long long)(a.f.taps - 1), reach = (unsigned long long)(a.lookahead - 1) + a.hold;
    r.frames = sl.frames;
    r.lo = hi > lo ? lo - sl.of : 0;
    r.hi = hi > lo ? hi - sl.of : 0;
    r.fa = r.lo > reach ? r.lo - reach : 0;
    r.fb = r.hi + (a.lookahead - 1) + D < sl.frames + D ? r.hi + (a.lookahead - 1) + D : sl.frames + D;
    r.s_lo = w.buf_first > sl.of ? w.buf_first - sl.of : 0;
    r.s_hi = buf_end > sl.of ? (buf_end - sl.of < sl.frames ? buf_end - sl.of : sl.frames) : 0;
    // frame 0 of the slice may lie in front of the buffer: the sums wrap, and wrap back at every frame that is read or written
    r.src_at = s * a.src_stride + (sl.of - w.buf_first) * nch;
    r.dst_at = s * a.dst_stride + (sl.of - w.win_first) * nch;
  } else if (a.tracks) {
    const TracksSlice sl = tracks_slice(a.tracks[s], a.frames, 0, false);
    r.src_at = r.dst_at = (s * a.frames + sl.of) * nch;
    r.frames = sl.frames;
  } else {
    r.src_at = s * a.src_stride;
    r.dst_at = s * a.dst_stride;
    r.frames = a.frames;
  }
  if (!kWin) {
    r.lo = r.fa = r.s_lo = 0;
    r.hi = r.s_hi = r.frames;
    r.fb = r.frames + (unsigned long long)(a.f.taps - 1);
  }
  r.r = a.work + s * 2 * a.work_stride;
  r.m = r.r + a.work_stride;
  r.has_gain = a.gain != nullptr;
  r.gain = r.has_gain ? a.gain[s] : 1.0;
  return r;
}

// RRX_finish_device's g for frame fr of the row, fr < r.frames
template <typename S> __host__ __device__ __forceinline__ double gained(const LimitArgs &a, const Row &r, unsigned long long fr, unsigned ch)
{
  const double v = (double)static_cast<const S *>(a.src)[r.src_at + fr * (unsigned)a.nch + ch];
  return r.has_gain ? v * r.gain : v;
}

// the same, +0.0 for a frame the source does not hold (the window form; a whole row holds all of its frames)
template <typename S, bool kWin> __host__ __device__ __forceinline__ double gained_held(const LimitArgs &a, const Row &r, unsigned long long fr, unsigned ch)
{
  if (kWin && (fr < r.s_lo || fr >= r.s_hi)) return 0.0;
  return gained<S>(a, r, fr, ch);
}

// One channel's share of a detector frame's level: h as true_peak_frame takes it, h[0] the frame itself (+0.0 behind the row)
template <int kP, int kT> __host__ __device__ __forceinline__ unsigned long long level_of(const LimitArgs &a, const double (&h)[kTpMaxTaps])
{
  const unsigned long long tp = true_peak_frame<kP, kT>(a.f.c, kP ? kP : a.f.phases, kT ? kT : a.f.taps, h), pk = true_peak_bits(fabs(h[0]));
  return tp > pk ? tp : pk;
}

// frame n of the row under the gain s
template <typename S, typename T> __host__ __device__ __forceinline__ void apply(const LimitArgs &a, const Row &r, unsigned long long n, double s)
{
  T *dst = static_cast<T *>(a.dst) + (r.dst_at + n * (unsigned)a.nch);
  for (unsigned ch = 0; ch < (unsigned)a.nch; ++ch) dst[ch] = limit_output<T>(gained<S>(a, r, n, ch), s);
}

// A workgroup takes kThreads detector frames at a time, one lane each, and stages their gained samples in LDS behind a halo of
// taps - 1 frames, as many channels at a time as kDetectTile doubles hold; the level is the maximum over the channel groups.
template <typename S, int kP, int kT, bool kWin> __global__ __launch_bounds__(kThreads) void limit_detect_kernel(LimitArgs a, int s0, LimitWindow w)
{
  __shared__ double tile[kDetectTile];
  const Row r = row_of<kWin>(a, w, (unsigned long long)(s0 + (int)blockIdx.y));
  if (kWin ? r.lo >= r.hi : !r.frames) return; // (the whole workgroup)
  const int taps = kT ? kT : a.f.taps;
  const unsigned tid = threadIdx.x, nch = (unsigned)a.nch, halo = (unsigned)(taps - 1);
  const unsigned most = (unsigned)kDetectTile / ((unsigned)kThreads + halo); // channels a tile holds: 15 (16 without a halo)
  const unsigned long long evals = kWin ? r.fb : r.frames + halo; // (r.fb of a whole row, from the kernel's own tap count)
  const unsigned long long first = kWin ? r.fa : 0;
  for (unsigned long long F0 = first + (unsigned long long)blockIdx.x * kThreads; F0 < evals; F0 += (unsigned long long)gridDim.x * kThreads) {
    const unsigned nf = evals - F0 < (unsigned long long)kThreads ? (unsigned)(evals - F0) : (unsigned)kThreads;
    unsigned long long lev = 0;
    for (unsigned c0 = 0; c0 < nch; c0 += most) {
      const unsigned cc = nch - c0 < most ? nch - c0 : most, count = (nf + halo) * cc;
      __syncthreads(); // the readers of the tile before are done
      for (unsigned j = tid; j < count; j += kThreads) {
        const unsigned fi = j / cc, c = j - fi * cc;
        const unsigned long long at = F0 + fi; // the frame, counted from halo frames in front of the row
        tile[j] = at >= halo && at - halo < r.frames ? gained_held<S, kWin>(a, r, at - halo, c0 + c) : 0.0;
      }
      __syncthreads();
      if (tid < nf) {
        for (unsigned c = 0; c < cc; ++c) {
          double h[kTpMaxTaps];
#pragma unroll
          for (int k = 0; k < kTpMaxTaps; ++k) h[k] = k < taps ? tile[(tid + halo - (unsigned)k) * cc + c] : 0.0;
          const unsigned long long b = level_of<kP, kT>(a, h);
          lev = b > lev ? b : lev;
        }
      }
    }
    if (tid < nf) r.r[F0 - first + tid] = limit_reduction(lev, a.ceiling);
  }
}

template <bool kWin> __global__ __launch_bounds__(kThreads) void limit_window_kernel(LimitArgs a, int s0, LimitWindow w)
{
  __shared__ double tile[kLimitMinTile];
  const Row r = row_of<kWin>(a, w, (unsigned long long)(s0 + (int)blockIdx.y));
  if (r.lo >= r.hi) return; // (the whole workgroup)
  const unsigned tid = threadIdx.x, L = a.lookahead, D = (unsigned)(a.f.taps - 1);
  const unsigned width = L + a.hold + D;                     // entries of r under one value of m
  const unsigned per = (unsigned)kLimitMinTile - (width - 1); // values of m a tile gives
  const unsigned long long outs = r.hi - r.lo + (L - 1), evals = r.frames + D; // the entries j = r.lo + o, o < outs
  const unsigned long long back = (unsigned long long)(L - 1) + a.hold; // m[j] begins at F = j - back
  for (unsigned long long t = blockIdx.x; t * per < outs; t += gridDim.x) {
    const unsigned long long o0 = t * per, j0 = r.lo + o0;
    const unsigned no = outs - o0 < per ? (unsigned)(outs - o0) : per, count = no + width - 1;
    if (t != blockIdx.x) __syncthreads(); // the readers of the tile before are done
    for (unsigned e = tid; e < count; e += kThreads) {
      const unsigned long long at = j0 + e; // F + back: every F of the row that is asked for lies in [r.fa, r.fb)
      tile[e] = at >= back && at - back < evals ? r.r[at - back - r.fa] : 1.0;
    }
    __syncthreads();
    unsigned w = 1; // entry e holds the minimum of [e, e + w) wherever e + w <= count
    for (; 2 * w <= width; w *= 2) {
      double v[kMinPerLane];
#pragma unroll
      for (int q = 0; q < kMinPerLane; ++q) {
        const unsigned e = tid + (unsigned)q * kThreads;
        if (e + w < count) {
          const double x = tile[e], y = tile[e + w];
          v[q] = y < x ? y : x;
        }
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < kMinPerLane; ++q) {
        const unsigned e = tid + (unsigned)q * kThreads;
        if (e + w < count) tile[e] = v[q];
      }
      __syncthreads();
    }
    for (unsigned i = tid; i < no; i += kThreads) { // [i, i + width) = [i, i + w) and [i + width - w, i + width), width < 2 w
      const double x = tile[i], y = tile[i + width - w];
      r.m[o0 + i] = y < x ? y : x;
    }
  }
}

template <typename S, typename T, bool kWin> __global__ __launch_bounds__(kThreads) void limit_apply_kernel(LimitArgs a, int s0, LimitWindow w)
{
  // entry e of the tile lies at (e % kLimitLaneFrames) * kApplyPitch + e / kLimitLaneFrames: a lane's frames are consecutive, and
  // the lanes of a wave then read consecutive doubles
  __shared__ double tile[kLimitLaneFrames * kApplyPitch];
  __shared__ double sh_gain[kLimitApplyFrames];
  __shared__ unsigned long long sh_min;
  __shared__ unsigned sh_count;
  const unsigned long long s = (unsigned long long)(s0 + (int)blockIdx.y);
  const Row r = row_of<kWin>(a, w, s);
  if (r.lo >= r.hi) return; // (the whole workgroup)
  const unsigned tid = threadIdx.x, L = a.lookahead;
  const unsigned long long one = true_peak_bits(1.0);
  if (!tid) {
    sh_min = one;
    sh_count = 0;
  }
  for (unsigned long long n0 = r.lo + (unsigned long long)blockIdx.x * kLimitApplyFrames; n0 < r.hi;
       n0 += (unsigned long long)gridDim.x * kLimitApplyFrames) {
    const unsigned nf = r.hi - n0 < (unsigned long long)kLimitApplyFrames ? (unsigned)(r.hi - n0) : (unsigned)kLimitApplyFrames;
    __syncthreads(); // sh_min is set; the readers of the tile and of the gains before are done
    for (unsigned e = tid; e < (unsigned)kLimitApplyFrames + L - 1; e += kThreads) // m[j], j = n0 + e: frame n reads j in [n, n + L)
      tile[(e % kLimitLaneFrames) * kApplyPitch + e / kLimitLaneFrames] = e < nf + L - 1 ? r.m[n0 - r.lo + e] : 1.0;
    __syncthreads();
    const unsigned f0 = tid * kLimitLaneFrames; // the lane's first frame in the tile
    if (f0 < nf) {
      double g[kLimitLaneFrames];
      limit_smooth_frames<kLimitLaneFrames>(
          [&](unsigned t) { return tile[(t % kLimitLaneFrames) * kApplyPitch + tid + t / kLimitLaneFrames]; }, L, a.inv_l, g);
      unsigned long long low = one;
      unsigned count = 0;
#pragma unroll
      for (int j = 0; j < kLimitLaneFrames; ++j) {
        if (f0 + (unsigned)j < nf) {
          sh_gain[f0 + (unsigned)j] = g[j];
          if (g[j] < 1.0) {
            const unsigned long long b = true_peak_bits(g[j]);
            low = b < low ? b : low;
            ++count;
          }
        }
      }
      if (count) {
        if (low < sh_min) atomicMin(&sh_min, low);
        atomicAdd(&sh_count, count);
      }
    }
    __syncthreads();
    // the tile's samples in the order they lie in memory, whatever the channel count: apply()'s product
    const unsigned long long nch = (unsigned long long)a.nch, total = nf * nch, at = n0 * nch;
    const S *src = static_cast<const S *>(a.src) + (r.src_at + at); // (the sum first: in the window form r.src_at may have wrapped)
    T *dst = static_cast<T *>(a.dst) + (r.dst_at + at);
    for (unsigned long long j = tid; j < total; j += kThreads) {
      const double v = (double)src[j];
      dst[j] = limit_output<T>(r.has_gain ? v * r.gain : v, sh_gain[j / nch]);
    }
  }
  __syncthreads();
  if (!tid) { // (a workgroup without a frame holds 1.0, which no frame's gain exceeds)
    if (a.reduction) {
      unsigned long long *p = reinterpret_cast<unsigned long long *>(a.reduction) + s;
      if (sh_min < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, sh_min);
    }
    if (a.limited && sh_count) atomicAdd(a.limited + s, (unsigned long long)sh_count);
  }
}

unsigned grid_x(unsigned long long pieces) { return pieces < 1 ? 1u : pieces > 0x7fffffffull ? 0x7fffffffu : (unsigned)pieces; }

// the passes [first, last) of detect, window, apply: all three for the calls of this file, the first two and the last one around
// the release (limit_release.hip)
template <typename S, typename T, bool kWin>
hipError_t launch_typed(hipStream_t stream, const LimitArgs &a, const LimitWindow &w, int first = 0, int last = 3)
{
  // the longest row, or the longest cut of one by the window.  The caller keeps frames * nch below 2^60, so nothing here wraps.
  const unsigned long long D = (unsigned long long)(a.f.taps - 1), L = a.lookahead;
  const unsigned long long per = (unsigned long long)kLimitMinTile - (L + a.hold + D - 1);
  const unsigned long long emit = kWin ? w.win_frames : a.frames, evals = kWin ? emit + 2 * (L - 1) + a.hold + D : emit + D;
  const unsigned gx1 = grid_x((evals + kThreads - 1) / kThreads), gx2 = grid_x((emit + L - 1 + per - 1) / per),
                 gx3 = grid_x((emit + kLimitApplyFrames - 1) / kLimitApplyFrames);
  const bool bs1770 = a.f.phases == 4 && a.f.taps == 12;
  const dim3 block(kThreads);
  for (int pass = first; pass < last; ++pass) {
    for (int s0 = 0; s0 < a.nstreams; s0 += 32768) { // grid.y is a 16-bit count
      const unsigned ns = (unsigned)(a.nstreams - s0 < 32768 ? a.nstreams - s0 : 32768);
      if (pass == 0 && bs1770) hipLaunchKernelGGL((limit_detect_kernel<S, 4, 12, kWin>), dim3(gx1, ns), block, 0, stream, a, s0, w);
      else if (pass == 0) hipLaunchKernelGGL((limit_detect_kernel<S, 0, 0, kWin>), dim3(gx1, ns), block, 0, stream, a, s0, w);
      else if (pass == 1) hipLaunchKernelGGL(limit_window_kernel<kWin>, dim3(gx2, ns), block, 0, stream, a, s0, w);
      else hipLaunchKernelGGL((limit_apply_kernel<S, T, kWin>), dim3(gx3, ns), block, 0, stream, a, s0, w);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
    }
  }
  return hipSuccess;
}

// head: r and m; tail: the gains, the product and the statistics (both for the calls of this file, one each around the release)
template <typename S, typename T, bool kWin> void host_typed(const LimitArgs &a, const LimitWindow &w, bool head = true, bool tail = true)
{
  const unsigned L = a.lookahead, D = (unsigned)(a.f.taps - 1);
  const unsigned long long back = (unsigned long long)(L - 1) + a.hold, width = (unsigned long long)L + a.hold + D;
  for (unsigned long long s = 0; s < (unsigned long long)a.nstreams; ++s) {
    const Row r = row_of<kWin>(a, w, s);
    if (r.lo >= r.hi) continue;
    const unsigned long long evals = r.frames + D, outs = r.hi - r.lo + (L - 1);
    for (unsigned long long F = r.fa; head && F < r.fb; ++F) {
      unsigned long long lev = 0;
      for (unsigned ch = 0; ch < (unsigned)a.nch; ++ch) {
        double h[kTpMaxTaps];
        for (unsigned k = 0; k < (unsigned)kTpMaxTaps; ++k) h[k] = k <= D && F >= k && F - k < r.frames ? gained_held<S, kWin>(a, r, F - k, ch) : 0.0;
        const unsigned long long b = level_of<0, 0>(a, h);
        lev = b > lev ? b : lev;
      }
      r.r[F - r.fa] = limit_reduction(lev, a.ceiling);
    }
    for (unsigned long long o = 0; head && o < outs; ++o) { // entry j = r.lo + o
      double least = 1.0; // what lies outside the row
      for (unsigned long long at = r.lo + o; at < r.lo + o + width; ++at)
        if (at >= back && at - back < evals && r.r[at - back - r.fa] < least) least = r.r[at - back - r.fa];
      r.m[o] = least;
    }
    if (!tail) continue;
    unsigned long long lowest = true_peak_bits(1.0), count = 0;
    for (unsigned long long n = r.lo; n < r.hi; ++n) {
      const double g = limit_smooth(r.m + (n - r.lo), L, a.inv_l);
      apply<S, T>(a, r, n, g);
      if (g < 1.0) {
        const unsigned long long b = true_peak_bits(g);
        lowest = b < lowest ? b : lowest;
        ++count;
      }
    }
    if (a.reduction) {
      unsigned long long have;
      std::memcpy(&have, a.reduction + s, 8);
      if (lowest < have) std::memcpy(a.reduction + s, &lowest, 8);
    }
    if (a.limited) a.limited[s] += count;
  }
}

} // namespace

namespace {

template <bool kWin> hipError_t launch_form(hipStream_t stream, const LimitArgs &a, const LimitWindow &w, int first = 0, int last = 3)
{
  if (a.src_double)
    return a.dst_double ? launch_typed<double, double, kWin>(stream, a, w, first, last) : launch_typed<double, float, kWin>(stream, a, w, first, last);
  return a.dst_double ? launch_typed<float, double, kWin>(stream, a, w, first, last) : launch_typed<float, float, kWin>(stream, a, w, first, last);
}

template <bool kWin> void host_form(const LimitArgs &a, const LimitWindow &w, bool head = true, bool tail = true)
{
  if (a.src_double) a.dst_double ? host_typed<double, double, kWin>(a, w, head, tail) : host_typed<double, float, kWin>(a, w, head, tail);
  else a.dst_double ? host_typed<float, double, kWin>(a, w, head, tail) : host_typed<float, float, kWin>(a, w, head, tail);
}

} // namespace

hipError_t launch_limit(hipStream_t stream, const LimitArgs &a, const LimitWindow *w)
{
  return w ? launch_form<true>(stream, a, *w) : launch_form<false>(stream, a, LimitWindow());
}

void limit_host(const LimitArgs &a, const LimitWindow *w) { w ? host_form<true>(a, *w) : host_form<false>(a, LimitWindow()); }

hipError_t launch_limit_passes(hipStream_t stream, const LimitArgs &a, int first, int last)
{
  return launch_form<false>(stream, a, LimitWindow(), first, last);
}

void limit_host_passes(const LimitArgs &a, bool head, bool tail) { host_form<false>(a, LimitWindow(), head, tail); }

hipError_t launch_limit_window_passes(hipStream_t stream, const LimitArgs &a, const LimitWindow &w, int first, int last)
{
  return launch_form<true>(stream, a, w, first, last);
}

void limit_host_window_passes(const LimitArgs &a, const LimitWindow &w, bool head, bool tail) { host_form<true>(a, w, head, tail); }

} // namespace rsmp
