// Noise-shaped dither for device-resident frames ("Noise-shaped dither"): the output stage of finish.hip with the
// requantisation error fed back through an FIR filter.  The recursion holds a rint, so a channel is a serial chain; the ABI
// clears the error history at every absolute frame that is a multiple of `segment`, which makes the segments independent chains.
//
// Shape: one lane is one (stream or track, segment, channel), channel fastest, so the lanes that share a line of interleaved
// frames are neighbours in a wave; grid = (lanes of a stream in workgroups of one wave, stream).  A lane walks the frames of its
// segment that lie inside the call in order, kBlock at a time: the loads of the NEXT kBlock frames are issued first, then gain,
// scale and the dither hash of this block's frames (shaped_front: nothing in it depends on an earlier error), then the chain
// (shaped_step: per sample one multiply, add, subtract, add, rint and subtract behind the previous error), then the stores.
// The history is an array of kK = 4 / 8 / 16 doubles indexed by constants only -- registers, no scratch; a filter shorter than kK
// is padded with zero coefficients, which changes no bit (finish_shaped.hpp).  bits is a run-time value: the kernel is bound by
// the latency of the chain, not by instruction count.
// Every lane reads its own samples at the sample type's alignment and writes each output sample with stores of that sample's own
// width (S24: three byte stores), so no byte outside the frames * nch samples of a destination row is touched, at any alignment.
// Peak and clip count stay in registers and leave as one atomic each per lane (a peak only when it beats the value there).
// The lane of a call's first segment loads its history from state_in when the call begins inside a segment; the lane of the last
// segment stores its history to state_out.
// The window form of the tracks kernel (tracks_finish_shaped_window_kernel) is the same lane around the part of a track's slice
// that lies inside a window (tracks_finish_cut): segments are still counted from the track's first output frame, so a window
// cuts every track's segments somewhere else, and the history crosses from window to window in a per-(track, channel) state.
#include "finish_shaped.hpp"

#include <cstring>

namespace rsmp {
namespace {

using u64 = unsigned long long;

constexpr int kThreads = 64, kBlock = 8;
constexpr unsigned kMaxGridX = 1u << 24; // beyond it the lanes of a row are taken in a grid-stride loop

__device__ __forceinline__ u64 peak_bits(double a) { return (u64)__double_as_longlong(a); }

// finish.hip's global_stats: bits of a non-negative double order as unsigned integers
__device__ __forceinline__ void lane_stats(double *peak, u64 *clipped, u64 c, u64 pk, u64 cl)
{
  if (peak && pk) {
    u64 *p = reinterpret_cast<u64 *>(peak) + c;
    if (pk > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, pk); // the value only ever grows
  }
  if (clipped && cl) atomicAdd(clipped + c, cl);
}

__device__ __forceinline__ void store_sample(unsigned char *p, int bits, int q)
{
  if (bits == 15) *reinterpret_cast<short *>(p) = (short)q;
  else if (bits == 23) finish_store_bytes<23>(p, q);
  else *reinterpret_cast<int *>(p) = q;
}

// What a lane needs besides its samples
struct LaneParams {
  double gain, scale, lo, hi;
  u64 seed, c;
  unsigned nch;
  int bits, bytes;
  bool has_gain, dither;
};

// n frames of one channel: src points at the lane's first sample, dst (or null) at its first output byte, F0 is the absolute
// frame of that sample.  Updates the history e and the lane's statistics.
template <typename S, int kK>
__device__ __forceinline__ void shaped_lane(const LaneParams &p, const S *src, unsigned char *dst, u64 n, u64 F0, const double (&coef)[kK],
                                            double (&e)[kK], u64 &pk, u64 &cl)
{
  const u64 nch = p.nch, nblk = n / kBlock;
  S x[kBlock];
  if (nblk) {
#pragma unroll
    for (int j = 0; j < kBlock; ++j) x[j] = src[(u64)j * nch];
  }
  for (u64 b = 0; b < nblk; ++b) {
    const u64 i = b * kBlock;
    // The next block's loads run ahead of this block's chain.  The last block loads itself again instead of branching around the
    // loads: with a branch the wait in front of the chain has to cover the path without them and comes out as "everything".
    const u64 inext = b + 1 < nblk ? i + kBlock : i;
    S xn[kBlock];
#pragma unroll
    for (int j = 0; j < kBlock; ++j) xn[j] = src[(inext + j) * nch];
    ShapedFront f[kBlock];
#pragma unroll
    for (int j = 0; j < kBlock; ++j) f[j] = shaped_front((double)x[j], p.has_gain, p.gain, p.scale, p.dither, p.seed, F0 + i + j, p.c);
    int q[kBlock];
#pragma unroll
    for (int j = 0; j < kBlock; ++j) {
      const FinishSample r = shaped_step<kK>(f[j], p.dither, p.lo, p.hi, coef, e);
      q[j] = r.q;
      const u64 bits = peak_bits(r.a);
      pk = bits > pk ? bits : pk;
      cl += r.clip ? 1u : 0u;
    }
    if (dst) {
      unsigned char *o = dst + i * nch * p.bytes;
#pragma unroll
      for (int j = 0; j < kBlock; ++j) store_sample(o + (u64)j * nch * p.bytes, p.bits, q[j]);
    }
#pragma unroll
    for (int j = 0; j < kBlock; ++j) x[j] = xn[j];
  }
  for (u64 i = nblk * kBlock; i < n; ++i) {
    const ShapedFront f = shaped_front((double)src[i * nch], p.has_gain, p.gain, p.scale, p.dither, p.seed, F0 + i, p.c);
    const FinishSample r = shaped_step<kK>(f, p.dither, p.lo, p.hi, coef, e);
    const u64 bits = peak_bits(r.a);
    pk = bits > pk ? bits : pk;
    cl += r.clip ? 1u : 0u;
    if (dst) store_sample(dst + i * nch * p.bytes, p.bits, r.q);
  }
}

__device__ __forceinline__ LaneParams lane_params(int bits, bool dither, u64 seed, unsigned nch)
{
  LaneParams p;
  p.scale = bits == 15 ? 0x1p15 : bits == 23 ? 0x1p23 : 0x1p31;
  p.lo = -p.scale;
  p.hi = p.scale - 1.0;
  p.bits = bits;
  p.bytes = bits == 15 ? 2 : bits == 23 ? 3 : 4;
  p.dither = dither;
  p.seed = seed;
  p.nch = nch;
  p.gain = 1.0;
  p.has_gain = false;
  p.c = 0;
  return p;
}

// S: float or double source.  kK: the filter order rounded up to 4, 8 or 16.
template <typename S, int kK>
__global__ __launch_bounds__(kThreads) void finish_shaped_kernel(ShapedArgs a, int s0)
{
  const unsigned nch = (unsigned)a.nch;
  const u64 s = (u64)(s0 + (int)blockIdx.y), seg = a.segment, last = a.first_frame + (a.frames - 1);
  const u64 seg0 = seg ? a.first_frame / seg : 0, nseg = seg ? last / seg - seg0 + 1 : 1, lanes = nseg * nch;
  double coef[kK];
#pragma unroll
  for (int k = 0; k < kK; ++k) coef[k] = a.coefs[k];
  LaneParams p = lane_params(a.bits, a.dither != 0, a.seed, nch);
  p.has_gain = a.gain != nullptr;
  if (p.has_gain) p.gain = a.gain[s];
  const S *row = static_cast<const S *>(a.src) + s * a.src_stride;
  unsigned char *out = a.dst ? static_cast<unsigned char *>(a.dst) + s * a.dst_stride * p.bytes : nullptr;
  const bool inside = !shaped_restarts(a.first_frame, seg); // the call begins inside a segment: its first lanes take the state

  for (u64 L = (u64)blockIdx.x * kThreads + threadIdx.x; L < lanes; L += (u64)gridDim.x * kThreads) {
    const u64 j = L / nch, ch = L - j * nch;
    const u64 A = seg ? (seg0 + j) * seg : 0;                 // the segment's first absolute frame, <= last
    const u64 F0 = A > a.first_frame ? A : a.first_frame;     // the lane's first frame
    const u64 rem = last - F0 + 1;                            // frames to the end of the call
    const u64 n = seg && seg - (F0 - A) < rem ? seg - (F0 - A) : rem;
    const u64 k0 = (F0 - a.first_frame) * nch + ch;
    p.c = s * nch + ch;
    double e[kK];
#pragma unroll
    for (int k = 0; k < kK; ++k) e[k] = 0.0;
    if (j == 0 && inside) {
      const double *st = a.state_in + p.c * kShapeMaxOrder;
#pragma unroll
      for (int k = 0; k < kK; ++k)
        if (k < a.order) e[k] = st[k];
    }
    u64 pk = 0, cl = 0;
    shaped_lane<S, kK>(p, row + k0, out ? out + k0 * p.bytes : nullptr, n, F0, coef, e, pk, cl);
    if (a.state_out && j == nseg - 1) {
      double *st = a.state_out + p.c * kShapeMaxOrder;
#pragma unroll
      for (int k = 0; k < kShapeMaxOrder; ++k) st[k] = k < kK && k < a.order ? e[k < kK ? k : 0] : 0.0;
    }
    lane_stats(a.peak, a.clipped, p.c, pk, cl);
  }
}

// Track t is stream t of finish_shaped_kernel with first_frame = 0 and no state: its slice of row t, clamped (tracks_slice), in
// segments counted from its own first output frame.  `lanes` comes from the pitch of the rows; a lane whose segment lies outside
// the slice has nothing to do.
template <typename S, int kK>
__global__ __launch_bounds__(kThreads) void tracks_finish_shaped_kernel(TracksShapedArgs a, int t0, u64 lanes)
{
  const unsigned nch = (unsigned)a.t.nch;
  const u64 t = (u64)(t0 + (int)blockIdx.y), seg = a.segment;
  const TracksSlice sl = tracks_slice(a.t.tracks[t], a.t.row_frames, a.t.dst_total, a.t.dst != nullptr);
  double coef[kK];
#pragma unroll
  for (int k = 0; k < kK; ++k) coef[k] = a.coefs[k];
  LaneParams p = lane_params(a.t.bits, a.t.dither != 0, a.t.seed, nch);
  p.has_gain = a.t.gain != nullptr;
  if (p.has_gain) p.gain = a.t.gain[t];
  const S *row = static_cast<const S *>(a.t.src) + (t * a.t.row_frames + sl.of) * nch;
  unsigned char *out = a.t.dst ? static_cast<unsigned char *>(a.t.dst) + sl.df * nch * p.bytes : nullptr;

  for (u64 L = (u64)blockIdx.x * kThreads + threadIdx.x; L < lanes; L += (u64)gridDim.x * kThreads) {
    const u64 j = L / nch, ch = L - j * nch;
    const u64 A = j * seg; // j <= row_frames / seg: no wrap
    if (A >= sl.frames) continue;
    const u64 n = seg && seg < sl.frames - A ? seg : sl.frames - A;
    const u64 k0 = A * nch + ch;
    p.c = t * nch + ch;
    double e[kK];
#pragma unroll
    for (int k = 0; k < kK; ++k) e[k] = 0.0;
    u64 pk = 0, cl = 0;
    shaped_lane<S, kK>(p, row + k0, out ? out + k0 * p.bytes : nullptr, n, A, coef, e, pk, cl);
    lane_stats(a.t.peak, a.t.clipped, p.c, pk, cl);
  }
}

// The window form.  a.s.t.src holds frames [w.first, w.first + w.frames) of every output row, pitch w.stride.  Track t's processed
// frames (tracks_finish_cut) are stream t of finish_shaped_kernel with first_frame = their index in the track, frames = their
// count and the track's entries of the state; the launch is sized from the window (a range of n frames meets at most
// ceil(n / segment) + 1 segments), and the loop below takes whatever segments the track's range really has.  A track with no
// frame in the window hands its state on unchanged: the lanes of segment slot 0, one per channel, copy it (zeros without a state).
template <typename S, int kK>
__global__ __launch_bounds__(kThreads) void tracks_finish_shaped_window_kernel(TracksShapedWindowArgs a, int t0)
{
  const TracksFinishArgs &ta = a.s.t;
  const unsigned nch = (unsigned)ta.nch;
  const u64 t = (u64)(t0 + (int)blockIdx.y), seg = a.s.segment;
  const TracksFinishCut c = tracks_finish_cut(ta.tracks[t], ta.row_frames, ta.dst_total, ta.dst != nullptr, a.w);
  const u64 frames = c.w1 - c.w0;
  if (!frames) {
    if (a.state_out)
      for (u64 L = (u64)blockIdx.x * kThreads + threadIdx.x; L < nch; L += (u64)gridDim.x * kThreads) {
        const u64 o = (t * nch + L) * kShapeMaxOrder;
#pragma unroll
        for (int k = 0; k < kShapeMaxOrder; ++k) a.state_out[o + k] = a.state_in ? a.state_in[o + k] : 0.0;
      }
    return;
  }
  const u64 first = c.index, last = c.index + (frames - 1); // frames of the track's slice, below row_frames
  const u64 seg0 = seg ? first / seg : 0, nseg = seg ? last / seg - seg0 + 1 : 1, lanes = nseg * nch;
  double coef[kK];
#pragma unroll
  for (int k = 0; k < kK; ++k) coef[k] = a.s.coefs[k];
  LaneParams p = lane_params(ta.bits, ta.dither != 0, ta.seed, nch);
  p.has_gain = ta.gain != nullptr;
  if (p.has_gain) p.gain = ta.gain[t];
  const S *row = static_cast<const S *>(ta.src) + (t * a.w.stride + c.w0) * nch;
  unsigned char *out = ta.dst ? static_cast<unsigned char *>(ta.dst) + c.dst_frame * nch * p.bytes : nullptr;
  // the range begins inside a segment: its first lanes take the state (first > 0 only behind w.first > 0, which has a state)
  const bool inside = !shaped_restarts(first, seg) && a.state_in;

  for (u64 L = (u64)blockIdx.x * kThreads + threadIdx.x; L < lanes; L += (u64)gridDim.x * kThreads) {
    const u64 j = L / nch, ch = L - j * nch;
    const u64 A = seg ? (seg0 + j) * seg : 0;                 // the segment's first frame of the track, <= last
    const u64 F0 = A > first ? A : first;                     // the lane's first frame
    const u64 rem = last - F0 + 1;                            // frames to the end of the range
    const u64 n = seg && seg - (F0 - A) < rem ? seg - (F0 - A) : rem;
    const u64 k0 = (F0 - first) * nch + ch;
    p.c = t * nch + ch;
    double e[kK];
#pragma unroll
    for (int k = 0; k < kK; ++k) e[k] = 0.0;
    if (j == 0 && inside) {
      const double *st = a.state_in + p.c * kShapeMaxOrder;
#pragma unroll
      for (int k = 0; k < kK; ++k)
        if (k < a.s.order) e[k] = st[k];
    }
    u64 pk = 0, cl = 0;
    shaped_lane<S, kK>(p, row + k0, out ? out + k0 * p.bytes : nullptr, n, F0, coef, e, pk, cl);
    if (a.state_out && j == nseg - 1) {
      double *st = a.state_out + p.c * kShapeMaxOrder;
#pragma unroll
      for (int k = 0; k < kShapeMaxOrder; ++k) st[k] = k < kK && k < a.s.order ? e[k < kK ? k : 0] : 0.0;
    }
    lane_stats(ta.peak, ta.clipped, p.c, pk, cl);
  }
}

unsigned grid_x(u64 lanes)
{
  const u64 wg = (lanes + kThreads - 1) / kThreads;
  return wg > kMaxGridX ? kMaxGridX : wg ? (unsigned)wg : 1u;
}

template <typename S, int kK> hipError_t launch_typed(hipStream_t stream, const ShapedArgs &a)
{
  const u64 seg = a.segment, last = a.first_frame + (a.frames - 1);
  const u64 nseg = seg ? last / seg - a.first_frame / seg + 1 : 1; // <= frames, and frames * nch < 2^60 (capi_stage.cpp)
  const unsigned gx = grid_x(nseg * (u64)a.nch);
  for (int s0 = 0; s0 < a.nstreams; s0 += 32768) { // grid.y is a 16-bit count
    const int ns = a.nstreams - s0 < 32768 ? a.nstreams - s0 : 32768;
    hipLaunchKernelGGL((finish_shaped_kernel<S, kK>), dim3(gx, (unsigned)ns), dim3(kThreads), 0, stream, a, s0);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

template <typename S> hipError_t launch_src(hipStream_t stream, const ShapedArgs &a)
{
  return a.order <= 4 ? launch_typed<S, 4>(stream, a) : a.order <= 8 ? launch_typed<S, 8>(stream, a) : launch_typed<S, 16>(stream, a);
}

template <typename S, int kK> hipError_t tracks_typed(hipStream_t stream, const TracksShapedArgs &a)
{
  const u64 seg = a.segment, nseg = seg ? (a.t.row_frames + seg - 1) / seg : 1; // row_frames * nch < 2^60 (capi_stage.cpp)
  const u64 lanes = nseg * (u64)a.t.nch;
  const unsigned gx = grid_x(lanes);
  for (int t0 = 0; t0 < a.t.ntracks; t0 += 32768) {
    const int nt = a.t.ntracks - t0 < 32768 ? a.t.ntracks - t0 : 32768;
    hipLaunchKernelGGL((tracks_finish_shaped_kernel<S, kK>), dim3(gx, (unsigned)nt), dim3(kThreads), 0, stream, a, t0, lanes);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

template <typename S> hipError_t tracks_src(hipStream_t stream, const TracksShapedArgs &a)
{
  return a.order <= 4 ? tracks_typed<S, 4>(stream, a) : a.order <= 8 ? tracks_typed<S, 8>(stream, a) : tracks_typed<S, 16>(stream, a);
}

template <typename S, int kK> hipError_t tracks_window_typed(hipStream_t stream, const TracksShapedWindowArgs &a)
{
  const u64 seg = a.s.segment, n = a.w.frames;
  u64 nseg = seg ? n / seg + (n % seg ? 1 : 0) + 1 : 1; // what n frames can meet, wherever the track's segments lie
  if (nseg > n) nseg = n;                               // (never more segments than frames); n * nch < 2^60 (capi_stage.cpp)
  const unsigned gx = grid_x(nseg * (u64)a.s.t.nch);
  for (int t0 = 0; t0 < a.s.t.ntracks; t0 += 32768) {
    const int nt = a.s.t.ntracks - t0 < 32768 ? a.s.t.ntracks - t0 : 32768;
    hipLaunchKernelGGL((tracks_finish_shaped_window_kernel<S, kK>), dim3(gx, (unsigned)nt), dim3(kThreads), 0, stream, a, t0);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

template <typename S> hipError_t tracks_window_src(hipStream_t stream, const TracksShapedWindowArgs &a)
{
  return a.s.order <= 4   ? tracks_window_typed<S, 4>(stream, a)
         : a.s.order <= 8 ? tracks_window_typed<S, 8>(stream, a)
                          : tracks_window_typed<S, 16>(stream, a);
}

// One channel on the host: n frames from absolute frame F0 on, x0 at the channel's first sample and o0 (or null) at its first
// output byte, both nch samples a frame.  The history starts from st_in when F0 lies inside a segment and goes to st_out.
template <typename S>
void host_chain(const S *x0, unsigned char *o0, u64 nch, u64 n, u64 F0, bool has_gain, double gain, int bits, bool dither, u64 seed, u64 c,
                const double (&coefs)[kShapeMaxOrder], int order, u64 segment, const double *st_in, double *st_out, double *peak, u64 *clipped)
{
  const double scale = bits == 15 ? 0x1p15 : bits == 23 ? 0x1p23 : 0x1p31, lo = -scale, hi = scale - 1.0;
  const int bytes = bits == 15 ? 2 : bits == 23 ? 3 : 4;
  double e[kShapeMaxOrder] = {};
  if (!shaped_restarts(F0, segment) && st_in)
    for (int k = 0; k < order; ++k) e[k] = st_in[c * kShapeMaxOrder + k];
  for (u64 i = 0; i < n; ++i) {
    const u64 F = F0 + i;
    if (i && shaped_restarts(F, segment))
      for (double &v : e) v = 0.0;
    const ShapedFront f = shaped_front((double)x0[i * nch], has_gain, gain, scale, dither, seed, F, c);
    const FinishSample r = shaped_step<kShapeMaxOrder>(f, dither, lo, hi, coefs, e);
    if (o0) {
      unsigned char *o = o0 + i * nch * bytes;
      if (bits == 15) finish_store_bytes<15>(o, r.q);
      else if (bits == 23) finish_store_bytes<23>(o, r.q);
      else finish_store_bytes<31>(o, r.q);
    }
    if (peak) {
      u64 have, now;
      std::memcpy(&have, peak + c, 8);
      std::memcpy(&now, &r.a, 8);
      if (now > have) std::memcpy(peak + c, &now, 8);
    }
    if (clipped && r.clip) ++clipped[c];
  }
  if (st_out)
    for (int k = 0; k < kShapeMaxOrder; ++k) st_out[c * kShapeMaxOrder + k] = k < order ? e[k] : 0.0;
}

template <typename S> void host_src(const ShapedArgs &a)
{
  const u64 nch = (u64)a.nch;
  const int bytes = a.bits == 15 ? 2 : a.bits == 23 ? 3 : 4;
  for (u64 s = 0; s < (u64)a.nstreams; ++s) {
    const S *src = static_cast<const S *>(a.src) + s * a.src_stride;
    unsigned char *dst = a.dst ? static_cast<unsigned char *>(a.dst) + s * a.dst_stride * bytes : nullptr;
    for (u64 ch = 0; ch < nch; ++ch)
      host_chain<S>(src + ch, dst ? dst + ch * bytes : nullptr, nch, a.frames, a.first_frame, a.gain != nullptr, a.gain ? a.gain[s] : 1.0, a.bits,
                    a.dither != 0, a.seed, s * nch + ch, a.coefs, a.order, a.segment, a.state_in, a.state_out, a.peak, a.clipped);
  }
}

template <typename S> void tracks_window_host_src(const TracksShapedWindowArgs &a)
{
  const TracksFinishArgs &ta = a.s.t;
  const u64 nch = (u64)ta.nch;
  const int bytes = ta.bits == 15 ? 2 : ta.bits == 23 ? 3 : 4;
  for (u64 t = 0; t < (u64)ta.ntracks; ++t) {
    const TracksFinishCut c = tracks_finish_cut(ta.tracks[t], ta.row_frames, ta.dst_total, ta.dst != nullptr, a.w);
    const S *src = static_cast<const S *>(ta.src) + (t * a.w.stride + c.w0) * nch;
    unsigned char *dst = ta.dst ? static_cast<unsigned char *>(ta.dst) + c.dst_frame * nch * bytes : nullptr;
    for (u64 ch = 0; ch < nch; ++ch) {
      const u64 o = (t * nch + ch) * kShapeMaxOrder;
      if (c.w1 > c.w0)
        host_chain<S>(src + ch, dst ? dst + ch * bytes : nullptr, nch, c.w1 - c.w0, c.index, ta.gain != nullptr, ta.gain ? ta.gain[t] : 1.0, ta.bits,
                      ta.dither != 0, ta.seed, t * nch + ch, a.s.coefs, a.s.order, a.s.segment, a.state_in, a.state_out, ta.peak, ta.clipped);
      else if (a.state_out)
        for (int k = 0; k < kShapeMaxOrder; ++k) a.state_out[o + k] = a.state_in ? a.state_in[o + k] : 0.0;
    }
  }
}

} // namespace

hipError_t launch_finish_shaped(hipStream_t stream, const ShapedArgs &a)
{
  return a.src_double ? launch_src<double>(stream, a) : launch_src<float>(stream, a);
}

hipError_t launch_tracks_finish_shaped(hipStream_t stream, const TracksShapedArgs &a)
{
  return a.t.src_double ? tracks_src<double>(stream, a) : tracks_src<float>(stream, a);
}

hipError_t launch_tracks_finish_shaped_window(hipStream_t stream, const TracksShapedWindowArgs &a)
{
  return a.s.t.src_double ? tracks_window_src<double>(stream, a) : tracks_window_src<float>(stream, a);
}

void finish_shaped_host(const ShapedArgs &a)
{
  if (a.src_double) host_src<double>(a);
  else host_src<float>(a);
}

void tracks_finish_shaped_window_host(const TracksShapedWindowArgs &a)
{
  if (a.s.t.src_double) tracks_window_host_src<double>(a);
  else tracks_window_host_src<float>(a);
}

} // namespace rsmp
