// True peak and loudness of a ragged batch by windows ("Windows with true peak and loudness").  The arithmetic is
// true_peak.hpp's and loudness.hpp's; this file is the lane layouts of true_peak.hip and loudness.hip around rows that a window
// cuts: a row is what a window holds of one track's slice (true_peak_window_cut / loudness_window_cut, measure_window.hpp), and
// what lies in front of it comes from a per-track state.
//
// True peak: the two forms of true_peak.hip.  A row has E = frames + (flush ? taps - 1 : 0) frames to evaluate, flush exactly when
// the window holds the slice's last frame.  The halo in front of the row's first frame is the track's state (+0.0 at index 0),
// elsewhere the window buffer gained again.  The workgroup that holds the row's last frame writes the track's state from its LDS
// (direct form: workgroup 0 of the row, from global memory); workgroup 0 of a track the window does not touch copies its state,
// one lane per (channel, entry).
//
// Loudness: the three launches of loudness.hip.  A track's range meets `pieces` hops, the first and the last of them possibly in
// part (loudness_piece):
//   launch 1   one lane per (track, channel, piece) runs the piece from Z_in (a first piece that begins mid-hop) or from zeros and
//              leaves the end state in `work`
//   launch 2   one lane per (track, channel) walks the pieces ascending from S_in: work <- the start state of the piece's hop,
//              S = M S + z for every hop that completes; writes the state (S, the Z of an unfinished last piece) and hops_out,
//              or copies the state of a track without a frame in the range
//   launch 3   the lanes of launch 1 run their piece again, from C_in, E_in (a first piece mid-hop) or from its S_k and +0.0;
//              a piece whose hop completes writes the energy, an unfinished last one C and E of the state
// Nothing outside the frames [w0, w0 + frames) of the window rows is read; nothing but the result arrays, work and state_out is
// written.
#include "measure_window.hpp"

#include <cstring>

namespace rsmp {
namespace {

constexpr int kThreads = 256, kTile = 16;
constexpr int kCarryThreads = 64;

// ================================================================================================================== true peak

// the value only ever grows
__device__ __forceinline__ void global_max(double *dst, unsigned long long c, unsigned long long v)
{
  if (!dst || !v) return;
  unsigned long long *p = reinterpret_cast<unsigned long long *>(dst) + c;
  if (v > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, v);
}

// one row of work: what the window holds of one track's slice
template <typename S> struct TpRow {
  const S *src;                 // sample 0 of the row's frame 0
  const double *state;          // channel 0 of the track in d_state_in, or null (index 0: +0.0 lies in front)
  unsigned long long frames, n; // real frames, and frames * nch
  unsigned long long evals;     // frames to evaluate: frames, plus taps - 1 when flushed
  unsigned long long cbase;     // track * nch
  double gain;
  bool has_gain;
};

template <typename S> __device__ __forceinline__ TpRow<S> tp_row_of(const TruePeakWindowArgs &a, unsigned long long t, int taps)
{
  TpRow<S> r;
  const unsigned long long nch = (unsigned long long)a.nch;
  const TruePeakWindowCut c = true_peak_window_cut(a.tracks[t], a.row_frames, a.w);
  r.src = static_cast<const S *>(a.src) + (t * a.w.stride + c.w0) * nch;
  r.frames = c.frames;
  r.cbase = t * nch;
  r.state = c.index && a.state_in ? a.state_in + r.cbase * kTpMaxTaps : nullptr;
  r.n = r.frames * nch;
  r.evals = !r.frames ? 0 : r.frames + (c.flush ? (unsigned long long)(taps - 1) : 0ull);
  r.has_gain = a.gain != nullptr;
  r.gain = r.has_gain ? a.gain[t] : 1.0;
  return r;
}

// Gained sample k of the row, k counted in samples from frame 0, channel 0 and at least -(taps - 1) * nch: RRX_finish_device's
// g inside the row, +0.0 behind it, the state (or +0.0) in front of it.
template <typename S> __device__ __forceinline__ double tp_gained(const TpRow<S> &r, long long k, unsigned nch)
{
  if (k >= 0) {
    if ((unsigned long long)k >= r.n) return 0.0;
    const double v = (double)r.src[k];
    return r.has_gain ? v * r.gain : v;
  }
  if (!r.state) return 0.0;
  const unsigned long long q = (unsigned long long)(-(k + 1)), back = q / nch; // back = 0: the frame in front of frame 0
  const unsigned ch = nch - 1u - (unsigned)(q - back * nch);
  return r.state[(unsigned long long)ch * kTpMaxTaps + back];
}

// entry j of every channel: the gained sample j + 1 frames before the frame behind the row's last one; zeros from taps - 1 on
template <typename S, typename F>
__device__ __forceinline__ void tp_write_state(const TruePeakWindowArgs &a, const TpRow<S> &r, int taps, F &&sample_back)
{
  double *out = a.state_out + r.cbase * kTpMaxTaps;
  const unsigned total = (unsigned)a.nch * kTpMaxTaps;
  for (unsigned i = threadIdx.x; i < total; i += kThreads) {
    const unsigned ch = i / kTpMaxTaps, j = i % kTpMaxTaps;
    out[i] = (int)j < taps - 1 ? sample_back(ch, j) : 0.0;
  }
}

// a track the window does not touch: its state is handed on as it came in (zeros without one)
__device__ __forceinline__ void tp_copy_state(const TruePeakWindowArgs &a, unsigned long long cbase)
{
  const unsigned long long base = cbase * kTpMaxTaps;
  const unsigned total = (unsigned)a.nch * kTpMaxTaps;
  for (unsigned i = threadIdx.x; i < total; i += kThreads) a.state_out[base + i] = a.state_in ? a.state_in[base + i] : 0.0;
}

// kP, kT: the filter's shape, 0 = the launch arguments'
template <typename S, int kP, int kT>
__global__ __launch_bounds__(kThreads) void true_peak_window_kernel(TruePeakWindowArgs a, int t0s, unsigned fpt, unsigned steps)
{
  __shared__ double tile[kTpLdsDoubles];
  __shared__ unsigned long long sh_tp[kTpLdsChannels], sh_pk[kTpLdsChannels];
  const unsigned tid = threadIdx.x, nch = (unsigned)a.nch;
  const int phases = kP ? kP : a.f.phases, taps = kT ? kT : a.f.taps;
  const unsigned halo = (unsigned)(taps - 1);
  const TpRow<S> r = tp_row_of<S>(a, (unsigned long long)(t0s + (int)blockIdx.y), taps);
  if (!r.frames) {
    if (blockIdx.x == 0 && a.state_out) tp_copy_state(a, r.cbase);
    return;
  }
  const unsigned long long tile0 = (unsigned long long)blockIdx.x * steps;
  if (tile0 * fpt >= r.evals) return; // (the whole workgroup: a track with few frames in the window)

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
    for (unsigned j = tid; j < count; j += kThreads) tile[j] = tp_gained(r, k0 + (long long)j, nch);
    __syncthreads();

    if (a.state_out && r.frames - 1 >= t0 && r.frames - 1 - t0 < nf) { // the tile of the last real frame
      const unsigned last = (unsigned)(r.frames - 1 - t0) + halo;     // its frame index in the tile
      tp_write_state(a, r, taps, [&](unsigned ch, unsigned j) { return tile[(last - j) * nch + ch]; });
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
template <typename S> __global__ __launch_bounds__(kThreads) void true_peak_window_direct_kernel(TruePeakWindowArgs a, int t0s)
{
  const unsigned nch = (unsigned)a.nch;
  const int phases = a.f.phases, taps = a.f.taps;
  const TpRow<S> r = tp_row_of<S>(a, (unsigned long long)(t0s + (int)blockIdx.y), taps);
  if (!r.frames) {
    if (blockIdx.x == 0 && a.state_out) tp_copy_state(a, r.cbase);
    return;
  }
  if (blockIdx.x == 0 && a.state_out) {
    tp_write_state(a, r, taps, [&](unsigned ch, unsigned j) {
      return tp_gained(r, ((long long)r.frames - 1 - (long long)j) * (long long)nch + (long long)ch, nch);
    });
  }
  const unsigned long long total = r.evals * nch, stride = (unsigned long long)gridDim.x * kThreads;
  for (unsigned long long i = (unsigned long long)blockIdx.x * kThreads + threadIdx.x; i < total; i += stride) {
    const unsigned long long fr = i / nch;
    const unsigned ch = (unsigned)(i - fr * nch);
    double h[kTpMaxTaps];
#pragma unroll
    for (int k = 0; k < kTpMaxTaps; ++k) h[k] = k < taps ? tp_gained(r, (long long)i - (long long)k * (long long)nch, nch) : 0.0;
    global_max(a.true_peak, r.cbase + ch, true_peak_frame<0, 0>(a.f.c, phases, taps, h));
    if (fr < r.frames) global_max(a.peak, r.cbase + ch, true_peak_bits(fabs(h[0])));
  }
}

template <typename S> hipError_t tp_launch_src(hipStream_t stream, const TruePeakWindowArgs &a)
{
  const unsigned long long nch = (unsigned long long)a.nch, halo = (unsigned long long)(a.f.taps - 1);
  // frames to evaluate in the longest row.  The caller keeps w.stride * nch below 2^60, so nothing here wraps.
  const unsigned long long evals = a.w.frames + halo;
  const bool lds = true_peak_lds_form(a.nch, a.f.taps), bs1770 = a.f.phases == 4 && a.f.taps == 12;
  unsigned fpt = 0, steps = 1;
  unsigned long long gx;
  if (lds) {
    fpt = (unsigned)(((unsigned long long)kTpLdsDoubles - halo * nch) / nch); // >= 1: nch * taps <= kTpLdsDoubles
    const unsigned long long row_tiles = (evals + fpt - 1) / fpt;
    // tiles per workgroup: as in true_peak.hip
    unsigned long long st = row_tiles * (unsigned long long)a.ntracks / 2048;
    st = st < 1 ? 1 : st > 16 ? 16 : st;
    while ((row_tiles + st - 1) / st > 0x7fffffffull) st *= 2;
    steps = (unsigned)st;
    gx = (row_tiles + st - 1) / st;
  } else {
    gx = (evals * nch + kThreads - 1) / kThreads; // (the kernel strides over what a full grid leaves)
    if (gx > 0x7fffffffull) gx = 0x7fffffffull;
  }
  for (int t0 = 0; t0 < a.ntracks; t0 += 32768) { // grid.y is a 16-bit count
    const int nt = a.ntracks - t0 < 32768 ? a.ntracks - t0 : 32768;
    const dim3 grid((unsigned)(gx ? gx : 1), (unsigned)nt), block(kThreads);
    if (!lds) hipLaunchKernelGGL((true_peak_window_direct_kernel<S>), grid, block, 0, stream, a, t0);
    else if (bs1770) hipLaunchKernelGGL((true_peak_window_kernel<S, 4, 12>), grid, block, 0, stream, a, t0, fpt, steps);
    else hipLaunchKernelGGL((true_peak_window_kernel<S, 0, 0>), grid, block, 0, stream, a, t0, fpt, steps);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

template <typename S> void tp_host_src(const TruePeakWindowArgs &a)
{
  const unsigned long long nch = (unsigned long long)a.nch;
  const int taps = a.f.taps;
  auto take = [](double *dst, unsigned long long c, unsigned long long now) {
    unsigned long long have;
    std::memcpy(&have, dst + c, 8);
    if (now > have) std::memcpy(dst + c, &now, 8);
  };
  for (unsigned long long t = 0; t < (unsigned long long)a.ntracks; ++t) {
    const TruePeakWindowCut cut = true_peak_window_cut(a.tracks[t], a.row_frames, a.w);
    const S *src = static_cast<const S *>(a.src) + (t * a.w.stride + cut.w0) * nch;
    const double gain = a.gain ? a.gain[t] : 1.0;
    for (unsigned long long ch = 0; ch < nch; ++ch) {
      const unsigned long long c = t * nch + ch;
      if (!cut.frames) { // the window does not touch the track: its state is handed on
        if (a.state_out)
          for (int j = 0; j < kTpMaxTaps; ++j) a.state_out[c * kTpMaxTaps + j] = a.state_in ? a.state_in[c * kTpMaxTaps + j] : 0.0;
        continue;
      }
      const bool hist = cut.index && a.state_in;
      double h[kTpMaxTaps];
      for (int k = 0; k < kTpMaxTaps; ++k) h[k] = 0.0;
      for (int j = 0; j + 1 < taps; ++j) h[j + 1] = hist ? a.state_in[c * kTpMaxTaps + j] : 0.0; // h[0] is the frame to come
      const unsigned long long evals = cut.frames + (cut.flush ? (unsigned long long)(taps - 1) : 0ull);
      for (unsigned long long i = 0; i < evals; ++i) {
        const bool real = i < cut.frames; // the flushed frames are +0.0 and enter the true peak only
        const double v = real ? (double)src[i * nch + ch] : 0.0;
        h[0] = !real ? 0.0 : a.gain ? v * gain : v;
        if (a.true_peak) take(a.true_peak, c, true_peak_frame<0, 0>(a.f.c, a.f.phases, taps, h));
        if (real && a.peak) take(a.peak, c, true_peak_bits(fabs(h[0])));
        for (int k = kTpMaxTaps - 1; k > 0; --k) h[k] = h[k - 1];
        if (i + 1 == cut.frames && a.state_out) // the history after the last real frame
          for (int j = 0; j < kTpMaxTaps; ++j) a.state_out[c * kTpMaxTaps + j] = j + 1 < taps ? h[j + 1] : 0.0;
      }
    }
  }
}

// =================================================================================================================== loudness

template <typename S> struct LdRow {
  const S *src; // sample 0 of window frame w0 of the track
  LoudnessWindowCut c;
  double gain;
  bool has_gain;
};

template <typename S> __host__ __device__ __forceinline__ LdRow<S> ld_row_of(const LoudnessWindowArgs &a, unsigned long long t)
{
  LdRow<S> r;
  r.c = loudness_window_cut(a.tracks[t], a.row_frames, a.hop, a.energy_stride, a.w);
  r.src = static_cast<const S *>(a.src) + (t * a.w.stride + r.c.w0) * (unsigned long long)a.nch;
  r.has_gain = a.gain != nullptr;
  r.gain = r.has_gain ? a.gain[t] : 1.0;
  return r;
}

template <typename S> __host__ __device__ __forceinline__ double ld_gained(const LdRow<S> &r, S x)
{
  const double v = (double)x;
  return r.has_gain ? v * r.gain : v;
}

__host__ __device__ __forceinline__ unsigned long long ld_work_index(const LoudnessWindowArgs &a, unsigned long long t, unsigned long long j, unsigned ch)
{
  return ((t * a.pieces + j) * (unsigned long long)a.nch + ch) * 4ull;
}

// a first piece that begins mid-hop goes on from the state; the state is read for a track only when index > 0
__host__ __device__ __forceinline__ bool ld_resumes(const LoudnessWindowArgs &a, const LoudnessWindowCut &c, unsigned long long j)
{
  return !j && c.r0 && a.state_in;
}

// kEnergy = false: launch 1; true: launch 3
template <typename S, bool kEnergy>
__global__ __launch_bounds__(kThreads) void loudness_window_pass_kernel(LoudnessWindowArgs a, int t0)
{
  const unsigned nch = (unsigned)a.nch;
  const unsigned long long t = (unsigned long long)(t0 + (int)blockIdx.y);
  const LdRow<S> r = ld_row_of<S>(a, t);
  const unsigned long long lanes = r.c.pieces * nch; // (pieces * nch <= (w.frames + 2) * nch < 2^61)

  for (unsigned long long l = (unsigned long long)blockIdx.x * kThreads + threadIdx.x; l < lanes; l += (unsigned long long)gridDim.x * kThreads) {
    const unsigned long long j = l / nch;
    const unsigned ch = (unsigned)(l - j * nch);
    const LoudnessPiece pc = loudness_piece(r.c, a.hop, j);
    const unsigned long long len = pc.b - pc.a;
    const S *p = r.src + pc.off * nch + ch; // the piece's first frame; frame i of it is p[i * nch], i < len
    double st[4] = {0.0, 0.0, 0.0, 0.0}, energy = 0.0;
    if (ld_resumes(a, r.c, j)) {
      const double *sin = a.state_in + (t * nch + ch) * kLoudnessWinState;
#pragma unroll
      for (int i = 0; i < 4; ++i) st[i] = sin[(kEnergy ? 8 : 4) + i];
      if (kEnergy) energy = sin[12];
    } else if (kEnergy) {
      const double *w = a.work + ld_work_index(a, t, j, ch);
#pragma unroll
      for (int i = 0; i < 4; ++i) st[i] = w[i];
    }

    S cur[kTile], next[kTile];
    auto fetch = [&](unsigned long long i0) {
#pragma unroll
      for (int i = 0; i < kTile; ++i) next[i] = i0 + i < len ? p[(i0 + i) * nch] : S(0);
    };
    fetch(0);
    for (unsigned long long i0 = 0; i0 < len; i0 += kTile) {
#pragma unroll
      for (int i = 0; i < kTile; ++i) cur[i] = next[i];
      if (i0 + kTile < len) fetch(i0 + kTile); // in flight while these frames are computed
#pragma unroll
      for (int i = 0; i < kTile; ++i)
        if (i0 + i < len) {
          const double v = loudness_step(a.c, ld_gained(r, cur[i]), st);
          energy = energy + v * v;
        }
    }
    if (!kEnergy) {
      double *w = a.work + ld_work_index(a, t, j, ch);
#pragma unroll
      for (int i = 0; i < 4; ++i) w[i] = st[i];
    } else if (pc.b == a.hop) {
      a.energy[(t * nch + ch) * a.energy_stride + r.c.k0 + j] = energy; // k0 + j < n <= energy_stride
    } else if (a.state_out) {
      double *so = a.state_out + (t * nch + ch) * kLoudnessWinState;
#pragma unroll
      for (int i = 0; i < 4; ++i) so[8 + i] = st[i];
      so[12] = energy;
    }
  }
}

// Launch 2 of one (track, channel); `so`: the channel's entries of state_out, or null.  Shared with the host twin.
template <typename S>
__host__ __device__ __forceinline__ void ld_carry(const LoudnessWindowArgs &a, const LdRow<S> &r, unsigned long long t, unsigned ch)
{
  const unsigned long long c = t * (unsigned long long)a.nch + ch;
  const double *sin = a.state_in ? a.state_in + c * kLoudnessWinState : nullptr;
  double *so = a.state_out ? a.state_out + c * kLoudnessWinState : nullptr;
  if (ch == 0) a.hops_out[t] = r.c.n;
  if (!r.c.frames) { // nothing of the track is processed: its state is handed on
    if (so)
      for (int i = 0; i < kLoudnessWinState; ++i) so[i] = sin ? sin[i] : 0.0;
    return;
  }
  double st[4] = {0.0, 0.0, 0.0, 0.0}, zl[4] = {0.0, 0.0, 0.0, 0.0};
  if (r.c.index && sin)
    for (int i = 0; i < 4; ++i) st[i] = sin[i];
  for (unsigned long long j = 0; j < r.c.pieces; ++j) {
    double *w = a.work + ld_work_index(a, t, j, ch);
    double z[4];
    for (int i = 0; i < 4; ++i) {
      z[i] = w[i];
      w[i] = st[i];
    }
    if (loudness_piece(r.c, a.hop, j).b == a.hop) loudness_carry(a.m, z, st); // the hop completes in this window
    else
      for (int i = 0; i < 4; ++i) zl[i] = z[i]; // an unfinished last piece
  }
  if (!so) return;
  // on a hop boundary Z = 0, C = S and E = +0.0; launch 3 writes C and E of an unfinished last piece over these
  for (int i = 0; i < 4; ++i) {
    so[i] = st[i];
    so[4 + i] = zl[i];
    so[8 + i] = st[i];
    so[12 + i] = 0.0;
  }
}

template <typename S> __global__ __launch_bounds__(kCarryThreads) void loudness_window_carry_kernel(LoudnessWindowArgs a)
{
  const unsigned long long total = (unsigned long long)a.ntracks * (unsigned long long)a.nch;
  for (unsigned long long c = (unsigned long long)blockIdx.x * kCarryThreads + threadIdx.x; c < total; c += (unsigned long long)gridDim.x * kCarryThreads) {
    const unsigned long long t = c / (unsigned)a.nch;
    const unsigned ch = (unsigned)(c - t * (unsigned)a.nch);
    ld_carry<S>(a, ld_row_of<S>(a, t), t, ch);
  }
}

template <typename S> hipError_t ld_launch_src(hipStream_t stream, const LoudnessWindowArgs &a)
{
  // workgroups of the track with the most pieces (pieces * nch < 2^61); the kernel strides over what a full grid leaves
  const unsigned long long groups = (a.pieces * (unsigned long long)a.nch + kThreads - 1) / kThreads;
  const unsigned gx = groups > 0x7fffffffull ? 0x7fffffffu : (unsigned)groups;
  const unsigned long long chans = (unsigned long long)a.ntracks * (unsigned long long)a.nch;
  const unsigned long long cb = (chans + kCarryThreads - 1) / kCarryThreads;
  for (int pass = 0; pass < 3; ++pass) {
    if (pass == 1) {
      hipLaunchKernelGGL((loudness_window_carry_kernel<S>), dim3(cb > 0x7fffffffull ? 0x7fffffffu : (unsigned)cb), dim3(kCarryThreads), 0, stream, a);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
      continue;
    }
    for (int t0 = 0; t0 < a.ntracks; t0 += 32768) { // grid.y is a 16-bit count
      const int nt = a.ntracks - t0 < 32768 ? a.ntracks - t0 : 32768;
      const dim3 grid(gx, (unsigned)nt), block(kThreads);
      if (pass == 0) hipLaunchKernelGGL((loudness_window_pass_kernel<S, false>), grid, block, 0, stream, a, t0);
      else hipLaunchKernelGGL((loudness_window_pass_kernel<S, true>), grid, block, 0, stream, a, t0);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
    }
  }
  return hipSuccess;
}

template <typename S> void ld_host_src(const LoudnessWindowArgs &a)
{
  const unsigned nch = (unsigned)a.nch;
  for (unsigned long long t = 0; t < (unsigned long long)a.ntracks; ++t) {
    const LdRow<S> r = ld_row_of<S>(a, t);
    for (unsigned ch = 0; ch < nch; ++ch) {
      const unsigned long long c = t * nch + ch;
      const double *sin = a.state_in ? a.state_in + c * kLoudnessWinState : nullptr;
      for (int pass = 0; pass < 3; ++pass) {
        if (pass == 1) {
          ld_carry<S>(a, r, t, ch);
          continue;
        }
        for (unsigned long long j = 0; j < r.c.pieces; ++j) {
          const LoudnessPiece pc = loudness_piece(r.c, a.hop, j);
          double *w = a.work + ld_work_index(a, t, j, ch);
          double st[4] = {0.0, 0.0, 0.0, 0.0}, energy = 0.0;
          if (ld_resumes(a, r.c, j)) {
            for (int i = 0; i < 4; ++i) st[i] = sin[(pass ? 8 : 4) + i];
            if (pass) energy = sin[12];
          } else if (pass) {
            for (int i = 0; i < 4; ++i) st[i] = w[i];
          }
          for (unsigned long long i = 0; i < pc.b - pc.a; ++i) {
            const double v = loudness_step(a.c, ld_gained(r, r.src[(pc.off + i) * nch + ch]), st);
            energy = energy + v * v;
          }
          if (!pass) {
            for (int i = 0; i < 4; ++i) w[i] = st[i];
          } else if (pc.b == a.hop) {
            a.energy[c * a.energy_stride + r.c.k0 + j] = energy;
          } else if (a.state_out) {
            double *so = a.state_out + c * kLoudnessWinState;
            for (int i = 0; i < 4; ++i) so[8 + i] = st[i];
            so[12] = energy;
          }
        }
      }
    }
  }
}

} // namespace

hipError_t launch_true_peak_window(hipStream_t stream, const TruePeakWindowArgs &a)
{
  return a.src_double ? tp_launch_src<double>(stream, a) : tp_launch_src<float>(stream, a);
}

void true_peak_window_host(const TruePeakWindowArgs &a)
{
  if (a.src_double) tp_host_src<double>(a);
  else tp_host_src<float>(a);
}

hipError_t launch_loudness_window(hipStream_t stream, const LoudnessWindowArgs &a)
{
  return a.src_double ? ld_launch_src<double>(stream, a) : ld_launch_src<float>(stream, a);
}

void loudness_window_host(const LoudnessWindowArgs &a)
{
  if (a.src_double) ld_host_src<double>(a);
  else ld_host_src<float>(a);
}

} // namespace rsmp
