// True-peak measurement for device-resident frames ("True peak"): one pass over the float32 / float64 frames that
// takes, per (stream, channel), the peak of the gained frames oversampled by a polyphase filter and the sample peak.  The
// arithmetic is true_peak_frame (true_peak.hpp), shared with the host twin at the end of this file.
//
// Shape: grid = (chunk of a row's frames, stream); a row is one stream of RRX_true_peak_device or one track's slice of
// RRX_tracks_true_peak_device (clamped by tracks_slice, flushed, without a state).  A row has E = frames + (flush ? taps - 1 : 0)
// frames to evaluate; the ones behind the last real frame are +0.0 and enter the true peak only.
//   LDS form (nch * taps <= kTpLdsDoubles, nch <= kTpLdsChannels): a workgroup takes `steps` consecutive tiles of `fpt` frames.
//     It stages the tile's gained doubles in LDS with taps - 1 halo frames in front of them -- read from the source and gained
//     again, which gives the same bits, or taken from d_state_in / +0.0 in front of the call's first frame -- and every lane
//     takes (frame, channel) pairs of ONE channel per pass over the tile: taps LDS loads into registers, the serial sums of all
//     phases, a running maximum in registers.  The maxima are merged per channel in LDS (an atomic only where the lane beats
//     what is there) and leave as at most one global atomic per (workgroup, channel, statistic), issued only when it beats the
//     stored value.  The workgroup whose tile holds the row's last real frame writes d_state_out from its LDS.
//   Direct form (any other channel count): one lane per (frame, channel) by division, taps read from global memory, atomics
//     straight to global memory (only when they beat the value there); workgroup 0 of a row writes d_state_out.
// A row can also be a track at rest in a packed source of float32, S16, packed S24 or S32 (RRX_tracks_true_peak_packed_device):
// the same kernels instantiated on TracksPacked<R>, whose row is tracks_packed_cut's clamp of the table entry and whose samples
// come through tracks_load_value (tracks.hpp), one load of the sample's own bytes per sample, while the tile is staged.
// The coefficients travel in the launch arguments.  Nothing outside the rows is read; nothing but the two result arrays and
// d_state_out is written.
#include "true_peak.hpp"

#include <cstring>

namespace rsmp {
namespace {

constexpr int kThreads = 256;

// the value only ever grows
__device__ __forceinline__ void global_max(double *dst, unsigned long long c, unsigned long long v)
{
  if (!dst || !v) return;
  unsigned long long *p = reinterpret_cast<unsigned long long *>(dst) + c;
  if (v > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, v);
}

// one row of work: S = float / double, a stream or a track's slice of its row; S = TracksPacked<R>, a track at rest in a packed
// source of samples stored as R (tracks.hpp)
template <typename S> struct Row {
  const typename TracksSrcOf<S>::raw *src; // sample 0 of the row's frame 0
  const double *state;          // channel 0 of the row in d_state_in, or null
  unsigned long long frames, n; // real frames, and frames * nch
  unsigned long long evals;     // frames to evaluate: frames, plus taps - 1 when flushed
  unsigned long long cbase;     // stream * nch
  double gain;
  bool has_gain;
};

template <typename S> __host__ __device__ __forceinline__ Row<S> row_of(const TruePeakArgs &a, unsigned long long s, int taps)
{
  using R = typename TracksSrcOf<S>::raw;
  Row<S> r;
  const unsigned long long nch = (unsigned long long)a.nch;
  bool flush;
  if (TracksSrcOf<S>::packed) { // src_stride: the source's frames, frames: max_frames
    const TracksPackedCut pc = tracks_packed_cut(a.tracks[s], a.src_stride, a.frames);
    r.src = static_cast<const R *>(a.src) + pc.first * nch;
    r.frames = pc.frames;
    r.state = nullptr;
    flush = true;
  } else if (a.tracks) {
    const TracksSlice sl = tracks_slice(a.tracks[s], a.frames, 0, false);
    r.src = static_cast<const R *>(a.src) + (s * a.frames + sl.of) * nch;
    r.frames = sl.frames;
    r.state = nullptr;
    flush = true;
  } else {
    r.src = static_cast<const R *>(a.src) + s * a.src_stride;
    r.frames = a.frames;
    r.state = a.state_in ? a.state_in + s * nch * kTpMaxTaps : nullptr;
    flush = a.flush != 0;
  }
  r.n = r.frames * nch;
  r.evals = !r.frames ? 0 : r.frames + (flush ? (unsigned long long)(taps - 1) : 0ull);
  r.cbase = s * nch;
  r.has_gain = a.gain != nullptr;
  r.gain = r.has_gain ? a.gain[s] : 1.0;
  return r;
}

// Gained sample k of the row, k counted in samples from frame 0, channel 0 and at least -(taps - 1) * nch: RRX_finish_device's
// g inside the row, +0.0 behind it, the state (or +0.0) in front of it.
template <typename S> __host__ __device__ __forceinline__ double gained(const Row<S> &r, long long k, unsigned nch)
{
  if (k >= 0) {
    if ((unsigned long long)k >= r.n) return 0.0;
    double v;
    if constexpr (TracksSrcOf<S>::packed) v = tracks_load_value(tracks_kind_of<typename TracksSrcOf<S>::raw>(), r.src, (unsigned long long)k);
    else v = (double)r.src[k];
    return r.has_gain ? v * r.gain : v;
  }
  if (!r.state) return 0.0;
  const unsigned long long q = (unsigned long long)(-(k + 1)), back = q / nch; // back = 0: the frame in front of frame 0
  const unsigned ch = nch - 1u - (unsigned)(q - back * nch);
  return r.state[(unsigned long long)ch * kTpMaxTaps + back];
}

// entry j of every channel: the gained sample j + 1 frames before the frame behind the row's last one; zeros from taps - 1 on
template <typename S, typename F>
__device__ __forceinline__ void write_state(const TruePeakArgs &a, const Row<S> &r, int taps, F &&sample_back)
{
  double *out = a.state_out + r.cbase * kTpMaxTaps;
  const unsigned total = (unsigned)a.nch * kTpMaxTaps;
  for (unsigned i = threadIdx.x; i < total; i += kThreads) {
    const unsigned ch = i / kTpMaxTaps, j = i % kTpMaxTaps;
    out[i] = (int)j < taps - 1 ? sample_back(ch, j) : 0.0;
  }
}

// kP, kT: the filter's shape, 0 = the launch arguments'
template <typename S, int kP, int kT>
__global__ __launch_bounds__(kThreads) void true_peak_kernel(TruePeakArgs a, int s0, unsigned fpt, unsigned steps)
{
  __shared__ double tile[kTpLdsDoubles];
  __shared__ unsigned long long sh_tp[kTpLdsChannels], sh_pk[kTpLdsChannels];
  const unsigned tid = threadIdx.x, nch = (unsigned)a.nch;
  const int phases = kP ? kP : a.f.phases, taps = kT ? kT : a.f.taps;
  const unsigned halo = (unsigned)(taps - 1);
  const Row<S> r = row_of<S>(a, (unsigned long long)(s0 + (int)blockIdx.y), taps);
  const unsigned long long tile0 = (unsigned long long)blockIdx.x * steps;
  if (tile0 * fpt >= r.evals) return; // (the whole workgroup: a short track, or a row without frames)

  for (unsigned c = tid; c < nch; c += kThreads) {
    sh_tp[c] = 0;
    sh_pk[c] = 0;
  }
  // lanes_ch channels side by side, fs frames of them at a time; the lanes left over (256 is no multiple of nch) idle
  const unsigned lanes_ch = nch < (unsigned)kThreads ? nch : (unsigned)kThreads, fs = (unsigned)kThreads / lanes_ch;
  const unsigned lf = tid / lanes_ch, lc = tid - lf * lanes_ch;

  for (unsigned u = 0; u < steps; ++u) {
    const unsigned long long t0 = (tile0 + u) * fpt;
    if (t0 >= r.evals) break;
    const unsigned nf = r.evals - t0 < fpt ? (unsigned)(r.evals - t0) : fpt;
    const long long k0 = ((long long)t0 - (long long)halo) * (long long)nch;
    const unsigned count = (nf + halo) * nch; // <= kTpLdsDoubles by the choice of fpt
    if (u) __syncthreads();                   // the readers of the tile before are done
    for (unsigned j = tid; j < count; j += kThreads) tile[j] = gained(r, k0 + (long long)j, nch);
    __syncthreads();

    if (a.state_out && !a.tracks && r.frames - 1 >= t0 && r.frames - 1 - t0 < nf) { // the tile of the last real frame
      const unsigned last = (unsigned)(r.frames - 1 - t0) + halo;                    // its frame index in the tile
      write_state(a, r, taps, [&](unsigned ch, unsigned j) { return tile[(last - j) * nch + ch]; });
    }

    if (lf < fs) {
      for (unsigned ch = lc; ch < nch; ch += lanes_ch) {
        unsigned long long tp = 0, pk = 0;
        for (unsigned fr = lf; fr < nf; fr += fs) {
          const unsigned base = (fr + halo) * nch + ch;
          double h[kTpMaxTaps];
#pragma unroll
          for (int k = 0; k < kTpMaxTaps; ++k) h[k] = k < taps ? tile[base - (unsigned)k * nch] : 0.0;
          const unsigned long long b = true_peak_frame<kP, kT>(a.f.c, phases, taps, h);
          tp = b > tp ? b : tp;
          if (t0 + fr < r.frames) { // the flushed frames enter the true peak only
            const unsigned long long m = true_peak_bits(fabs(h[0]));
            pk = m > pk ? m : pk;
          }
        }
        if (tp > sh_tp[ch]) atomicMax(&sh_tp[ch], tp);
        if (pk > sh_pk[ch]) atomicMax(&sh_pk[ch], pk);
      }
    }
  }

  __syncthreads();
  for (unsigned c = tid; c < nch; c += kThreads) {
    global_max(a.true_peak, r.cbase + c, sh_tp[c]);
    global_max(a.peak, r.cbase + c, sh_pk[c]);
  }
}

// the direct form: any channel count, any filter shape
template <typename S> __global__ __launch_bounds__(kThreads) void true_peak_direct_kernel(TruePeakArgs a, int s0)
{
  const unsigned nch = (unsigned)a.nch;
  const int phases = a.f.phases, taps = a.f.taps;
  const Row<S> r = row_of<S>(a, (unsigned long long)(s0 + (int)blockIdx.y), taps);
  if (!r.evals) return;
  if (blockIdx.x == 0 && a.state_out && !a.tracks) {
    write_state(a, r, taps, [&](unsigned ch, unsigned j) {
      return gained(r, ((long long)r.frames - 1 - (long long)j) * (long long)nch + (long long)ch, nch);
    });
  }
  const unsigned long long total = r.evals * nch, stride = (unsigned long long)gridDim.x * kThreads;
  for (unsigned long long i = (unsigned long long)blockIdx.x * kThreads + threadIdx.x; i < total; i += stride) {
    const unsigned long long fr = i / nch;
    const unsigned ch = (unsigned)(i - fr * nch);
    double h[kTpMaxTaps];
#pragma unroll
    for (int k = 0; k < kTpMaxTaps; ++k) h[k] = k < taps ? gained(r, (long long)i - (long long)k * (long long)nch, nch) : 0.0;
    global_max(a.true_peak, r.cbase + ch, true_peak_frame<0, 0>(a.f.c, phases, taps, h));
    if (fr < r.frames) global_max(a.peak, r.cbase + ch, true_peak_bits(fabs(h[0])));
  }
}

template <typename S> hipError_t launch_src(hipStream_t stream, const TruePeakArgs &a)
{
  const unsigned long long nch = (unsigned long long)a.nch, halo = (unsigned long long)(a.f.taps - 1);
  // frames to evaluate in the longest row.  The caller keeps frames * nch below 2^60, so nothing here wraps.
  const unsigned long long evals = a.frames + ((a.tracks || a.flush) ? halo : 0ull);
  const bool lds = true_peak_lds_form(a.nch, a.f.taps), bs1770 = a.f.phases == 4 && a.f.taps == 12;
  unsigned fpt = 0, steps = 1;
  unsigned long long gx;
  if (lds) {
    fpt = (unsigned)(((unsigned long long)kTpLdsDoubles - halo * nch) / nch); // >= 1: nch * taps <= kTpLdsDoubles
    const unsigned long long row_tiles = (evals + fpt - 1) / fpt;
    // tiles per workgroup: as many as leave about 8 workgroups per CU on the chip, at most 16; more only to stay inside the grid limit
    unsigned long long st = row_tiles * (unsigned long long)a.nstreams / 2048;
    st = st < 1 ? 1 : st > 16 ? 16 : st;
    while ((row_tiles + st - 1) / st > 0x7fffffffull) st *= 2;
    steps = (unsigned)st;
    gx = (row_tiles + st - 1) / st;
  } else {
    gx = (evals * nch + kThreads - 1) / kThreads; // (the kernel strides over what a full grid leaves)
    if (gx > 0x7fffffffull) gx = 0x7fffffffull;
  }
  for (int s0 = 0; s0 < a.nstreams; s0 += 32768) { // grid.y is a 16-bit count
    const int ns = a.nstreams - s0 < 32768 ? a.nstreams - s0 : 32768;
    const dim3 grid((unsigned)(gx ? gx : 1), (unsigned)ns), block(kThreads);
    if (!lds) hipLaunchKernelGGL((true_peak_direct_kernel<S>), grid, block, 0, stream, a, s0);
    else if (bs1770) hipLaunchKernelGGL((true_peak_kernel<S, 4, 12>), grid, block, 0, stream, a, s0, fpt, steps);
    else hipLaunchKernelGGL((true_peak_kernel<S, 0, 0>), grid, block, 0, stream, a, s0, fpt, steps);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

template <typename S> void host_src(const TruePeakArgs &a)
{
  const unsigned long long nch = (unsigned long long)a.nch;
  const int taps = a.f.taps;
  auto take = [](double *dst, unsigned long long c, unsigned long long now) {
    unsigned long long have;
    std::memcpy(&have, dst + c, 8);
    if (now > have) std::memcpy(dst + c, &now, 8);
  };
  for (unsigned long long s = 0; s < (unsigned long long)a.nstreams; ++s) {
    const Row<S> r = row_of<S>(a, s, taps); // the kernels' row: a stream, or a track's clamped slice
    for (unsigned long long ch = 0; ch < nch; ++ch) {
      const unsigned long long c = s * nch + ch;
      double h[kTpMaxTaps];
      for (int k = 0; k < kTpMaxTaps; ++k) h[k] = 0.0;
      for (int j = 0; j + 1 < taps; ++j) h[j + 1] = r.state ? r.state[ch * kTpMaxTaps + j] : 0.0; // h[0] is the frame to come
      for (unsigned long long i = 0; i < r.evals; ++i) {
        const bool real = i < r.frames; // the flushed frames are +0.0 and enter the true peak only
        h[0] = real ? gained(r, (long long)(i * nch + ch), (unsigned)nch) : 0.0;
        if (a.true_peak) take(a.true_peak, c, true_peak_frame<0, 0>(a.f.c, a.f.phases, taps, h));
        if (real && a.peak) take(a.peak, c, true_peak_bits(fabs(h[0])));
        for (int k = kTpMaxTaps - 1; k > 0; --k) h[k] = h[k - 1];
        if (i + 1 == r.frames && a.state_out && !a.tracks) // the history after the last real frame
          for (int j = 0; j < kTpMaxTaps; ++j) a.state_out[c * kTpMaxTaps + j] = j + 1 < taps ? h[j + 1] : 0.0;
      }
    }
  }
}

} // namespace

hipError_t launch_true_peak(hipStream_t stream, const TruePeakArgs &a)
{
  return a.src_double ? launch_src<double>(stream, a) : launch_src<float>(stream, a);
}

void true_peak_host(const TruePeakArgs &a)
{
  if (a.src_double) host_src<double>(a);
  else host_src<float>(a);
}

hipError_t launch_true_peak_packed(hipStream_t stream, const TruePeakArgs &a, int kind)
{
  switch (kind) {
  case kTracksSrcS16: return launch_src<TracksPacked<short>>(stream, a);
  case kTracksSrcS24: return launch_src<TracksPacked<TracksS24>>(stream, a);
  case kTracksSrcS32: return launch_src<TracksPacked<int>>(stream, a);
  default: return launch_src<TracksPacked<float>>(stream, a);
  }
}

void true_peak_packed_host(const TruePeakArgs &a, int kind)
{
  switch (kind) {
  case kTracksSrcS16: return host_src<TracksPacked<short>>(a);
  case kTracksSrcS24: return host_src<TracksPacked<TracksS24>>(a);
  case kTracksSrcS32: return host_src<TracksPacked<int>>(a);
  default: return host_src<TracksPacked<float>>(a);
  }
}

} // namespace rsmp
