// Hop energies and gate of the loudness measurement ("Loudness").  The arithmetic is loudness.hpp's; this file is
// the lane layout around it.
//
// A channel's K-weighting is one serial recursion, so RRX_loudness_device cuts it into hops (include/ratelib_amd.h):
//   pass 1   one lane per (stream, channel, hop) runs the hop from an all-zero state and leaves its end state z_k in `work`
//   carry    one lane per (stream, channel) walks the hops ascending, S_{k+1} = M S_k + z_k, and leaves S_k where z_k was
//   pass 3   the lanes of pass 1 run their hop again from S_k and write its energy
// Passes 1 and 3 are one kernel: lane L of a stream takes (hop, channel) = (L / nch, L % nch) and streams its own hop from global
// memory, kTile frames at a time into registers, with the loads of the next kTile frames issued before these are computed: at
// the sizes of a music library (108 hops of 256 x 2 channels) there is about one wave per SIMD, and nothing else would hide the
// latency of the loads.  The frames of a hop lie hop * nch samples from those of the next, so a load instruction of a stereo wave
// touches 32 cache lines; each of them is used up by the lane's next kTile loads (16 stereo float frames are one 128-byte line),
// and a form that stages the tiles through LDS with loads along the rows measured 17-18 % slower ("Loudness").
// A row can also be a track at rest in a packed source of float32, S16, packed S24 or S32 (RRX_tracks_loudness_packed_device):
// the same kernels instantiated on TracksPacked<R>, whose row is tracks_packed_cut's clamp of the table entry.  The lanes keep the
// samples in flight as they are stored (R; three bytes for S24) and convert them by tracks_value where they are used.  Mono and
// stereo S24 take loudness_pass_s24_kernel, which loads the aligned dwords that cover a lane's tile instead of three bytes a sample.
// Nothing outside the whole hops of the rows is read; nothing but energy, work, state_out and hops_out is written.
#include "loudness.hpp"

namespace rsmp {
namespace {

constexpr int kThreads = 256, kTile = 16;
constexpr int kCarryThreads = 64, kAhead = 8;

// one row of work: S = float / double, a stream or a track's slice of its row; S = TracksPacked<R>, a track at rest in a packed
// source of samples stored as R (tracks.hpp)
template <typename S> struct Row {
  const typename TracksSrcOf<S>::raw *src; // sample 0 of the row's frame 0
  unsigned long long n; // whole hops
  double gain;
  bool has_gain;
};

template <typename S> __host__ __device__ __forceinline__ Row<S> row_of(const LoudnessArgs &a, unsigned long long s)
{
  using R = typename TracksSrcOf<S>::raw;
  Row<S> r;
  const unsigned long long nch = (unsigned long long)a.nch;
  if (TracksSrcOf<S>::packed) { // src_stride: the source's frames, frames: max_frames
    const TracksPackedCut pc = tracks_packed_cut(a.tracks[s], a.src_stride, a.frames);
    r.src = static_cast<const R *>(a.src) + pc.first * nch;
    r.n = pc.frames / a.hop; // <= max_hops: pc.frames <= max_frames
    if (r.n > a.energy_stride) r.n = a.energy_stride;
  } else if (a.tracks) {
    const TracksSlice sl = tracks_slice(a.tracks[s], a.frames, 0, false);
    r.src = static_cast<const R *>(a.src) + (s * a.frames + sl.of) * nch;
    r.n = sl.frames / a.hop; // <= max_hops: sl.frames <= row_frames
    if (r.n > a.energy_stride) r.n = a.energy_stride;
  } else {
    r.src = static_cast<const R *>(a.src) + s * a.src_stride;
    r.n = a.max_hops;
  }
  r.has_gain = a.gain != nullptr;
  r.gain = r.has_gain ? a.gain[s] : 1.0;
  return r;
}

// x: one sample as it is stored
template <typename S> __host__ __device__ __forceinline__ double gained(const Row<S> &r, typename TracksSrcOf<S>::raw x)
{
  const double v = tracks_value(x);
  return r.has_gain ? v * r.gain : v;
}

// gained sample i of the row, for the host loops: a packed source through the load function of the measuring path
template <typename S> double gained_at(const Row<S> &r, unsigned long long i)
{
  if constexpr (TracksSrcOf<S>::packed) {
    const double v = tracks_load_value(tracks_kind_of<typename TracksSrcOf<S>::raw>(), r.src, i);
    return r.has_gain ? v * r.gain : v;
  } else {
    return gained(r, r.src[i]);
  }
}

__host__ __device__ __forceinline__ unsigned long long work_index(const LoudnessArgs &a, unsigned long long s, unsigned long long k, unsigned ch)
{
  return ((s * a.max_hops + k) * (unsigned long long)a.nch + ch) * 4ull;
}

// kEnergy = false: pass 1; true: pass 3
template <typename S, bool kEnergy>
__global__ __launch_bounds__(kThreads) void loudness_pass_kernel(LoudnessArgs a, int s0)
{
  using R = typename TracksSrcOf<S>::raw;
  const unsigned nch = (unsigned)a.nch;
  const unsigned long long s = (unsigned long long)(s0 + (int)blockIdx.y);
  const Row<S> r = row_of<S>(a, s);
  const unsigned long long hop = a.hop, lanes = r.n * nch; // (n * nch <= frames * nch < 2^60)

  for (unsigned long long l = (unsigned long long)blockIdx.x * kThreads + threadIdx.x; l < lanes; l += (unsigned long long)gridDim.x * kThreads) {
    const unsigned long long k = l / nch;
    const unsigned ch = (unsigned)(l - k * nch);
    const R *p = r.src + k * hop * nch + ch; // the hop's first frame; frame i of it is p[i * nch], i < hop
    double st[4] = {0.0, 0.0, 0.0, 0.0}, energy = 0.0;
    if (kEnergy) {
      const double *w = a.work + work_index(a, s, k, ch);
#pragma unroll
      for (int i = 0; i < 4; ++i) st[i] = w[i];
    }

    R cur[kTile], next[kTile];
    auto fetch = [&](unsigned long long i0) {
#pragma unroll
      for (int i = 0; i < kTile; ++i) next[i] = i0 + i < hop ? p[(i0 + i) * nch] : R();
    };
    fetch(0);
    for (unsigned long long i0 = 0; i0 < hop; i0 += kTile) {
#pragma unroll
      for (int i = 0; i < kTile; ++i) cur[i] = next[i];
      if (i0 + kTile < hop) fetch(i0 + kTile); // in flight while these frames are computed
#pragma unroll
      for (int i = 0; i < kTile; ++i)
        if (i0 + i < hop) {
          const double v = loudness_step(a.c, gained(r, cur[i]), st);
          energy = energy + v * v;
        }
    }
    if (kEnergy) {
      a.energy[(s * nch + ch) * a.energy_stride + a.first_hop + k] = energy;
    } else {
      double *w = a.work + work_index(a, s, k, ch);
#pragma unroll
      for (int i = 0; i < 4; ++i) w[i] = st[i];
    }
  }
}

// The pass kernel for a packed S24 source of kN = 1 or 2 channels, the layouts of a music library.  Three byte loads a sample
// from a lane's own strided frames make the pass 2.4 times slower than the float rows' ("Packed sources"), so a lane
// loads the aligned dwords that cover its tile instead, as the stage copy kernel does for its groups (tracks.hip, unpack4): the
// kTile samples of a lane span ((kTile - 1) * kN + 1) * 3 = 48 or 93 bytes from p, its first sample; with mis = p & 3 -- the
// same for every tile of the lane, tiles being 48 * kN bytes apart -- they lie in the kD = 12 * kN dwords from p - mis, and for
// kN = 1 and mis != 0 in one more.  The dwords stay in registers as loaded while the tile before is computed; then they are
// realigned by mis (v_alignbit) and the sample at byte 3 * i * kN, a compile-time position, is cut out and sign-extended.  The
// value and everything behind it are the generic kernel's: tracks_value_s24, the gain, loudness_step.
// Reads: only dwords that hold a byte of the lane's tile, which lies inside a whole hop of the clamped track; so the whole aligned
// dword that holds the first or the last byte of the source may be read, and nothing further out.  The hop's last, partial tile
// loads dword by dword, only those that hold a byte of its frames.
template <int kN, bool kEnergy>
__global__ __launch_bounds__(kThreads) void loudness_pass_s24_kernel(LoudnessArgs a, int s0)
{
  using S = TracksPacked<TracksS24>;
  constexpr int kD = 12 * kN;
  const unsigned long long s = (unsigned long long)(s0 + (int)blockIdx.y);
  const Row<S> r = row_of<S>(a, s);
  const unsigned long long hop = a.hop, lanes = r.n * kN;

  for (unsigned long long l = (unsigned long long)blockIdx.x * kThreads + threadIdx.x; l < lanes; l += (unsigned long long)gridDim.x * kThreads) {
    const unsigned long long k = l / kN;
    const unsigned ch = (unsigned)(l - k * kN);
    const unsigned char *p = reinterpret_cast<const unsigned char *>(r.src + k * hop * kN + ch); // the lane's first sample
    const unsigned mis = (unsigned)(reinterpret_cast<unsigned long long>(p) & 3u), sh = mis * 8;
    const unsigned *w = reinterpret_cast<const unsigned *>(p - mis); // dword aligned; tile i0 begins (i0 / 4) * 3 * kN dwords on
    double st[4] = {0.0, 0.0, 0.0, 0.0}, energy = 0.0;
    if (kEnergy) {
      const double *z = a.work + work_index(a, s, k, ch);
#pragma unroll
      for (int i = 0; i < 4; ++i) st[i] = z[i];
    }

    unsigned cur[kD + 1], next[kD + 1];
    auto fetch = [&](unsigned long long i0) {
      const unsigned *q = w + (i0 >> 2) * (3 * kN);
      if (i0 + kTile <= hop) { // a whole tile: kD dwords, and the one behind them where the last sample reaches into it
        __builtin_memcpy(next, q, kD * sizeof(unsigned));
        next[kD] = kN == 1 && mis ? q[kD] : 0u;
      } else { // the hop's last frames: the dwords that hold a byte of them, one by one
        const unsigned m = (unsigned)(hop - i0), ndw = (mis + ((m - 1) * kN + 1) * 3 + 3) >> 2; // <= kD + 1
#pragma unroll
        for (int j = 0; j <= kD; ++j) next[j] = (unsigned)j < ndw ? q[j] : 0u;
      }
    };
    fetch(0);
    for (unsigned long long i0 = 0; i0 < hop; i0 += kTile) {
#pragma unroll
      for (int j = 0; j <= kD; ++j) cur[j] = next[j];
      if (i0 + kTile < hop) fetch(i0 + kTile); // in flight while these frames are computed
      unsigned d[kD];
#pragma unroll
      for (int j = 0; j < kD; ++j) d[j] = __builtin_amdgcn_alignbit(cur[j + 1], cur[j], sh); // byte 0 of d[0] is byte 0 of the lane's first sample
#pragma unroll
      for (int i = 0; i < kTile; ++i)
        if (i0 + i < hop) {
          const int o = 3 * i * kN, c = o >> 2, b = (o & 3) * 8; // where sample i begins in d
          // (b >= 16 only where c + 1 < kD: the last sample ends inside d[kD - 1])
          const int q = b == 0 ? (int)(d[c] << 8) >> 8 : b == 8 ? (int)d[c] >> 8 : (int)(__builtin_amdgcn_alignbit(d[c + 1 < kD ? c + 1 : c], d[c], b) << 8) >> 8;
          const double x = tracks_value_s24(q);
          const double v = loudness_step(a.c, r.has_gain ? x * r.gain : x, st);
          energy = energy + v * v;
        }
    }
    if (kEnergy) {
      a.energy[(s * kN + ch) * a.energy_stride + a.first_hop + k] = energy;
    } else {
      double *z = a.work + work_index(a, s, k, ch);
#pragma unroll
      for (int i = 0; i < 4; ++i) z[i] = st[i];
    }
  }
}

// one lane per (stream, channel): z_k -> S_k in place, hops ascending; S after the last hop goes to state_out
template <typename S> __global__ __launch_bounds__(kCarryThreads) void loudness_carry_kernel(LoudnessArgs a)
{
  const unsigned long long total = (unsigned long long)a.nstreams * (unsigned long long)a.nch;
  for (unsigned long long c = (unsigned long long)blockIdx.x * kCarryThreads + threadIdx.x; c < total; c += (unsigned long long)gridDim.x * kCarryThreads) {
    const unsigned long long s = c / (unsigned)a.nch;
    const unsigned ch = (unsigned)(c - s * (unsigned)a.nch);
    const Row<S> r = row_of<S>(a, s);
    double st[4] = {0.0, 0.0, 0.0, 0.0};
    if (a.state_in) {
#pragma unroll
      for (int i = 0; i < 4; ++i) st[i] = a.state_in[c * 4 + i];
    }
    for (unsigned long long k = 0; k < r.n; k += kAhead) {
      double z[kAhead][4];
#pragma unroll
      for (int u = 0; u < kAhead; ++u)
        if (k + u < r.n) {
          const double *w = a.work + work_index(a, s, k + u, ch);
#pragma unroll
          for (int i = 0; i < 4; ++i) z[u][i] = w[i];
        }
#pragma unroll
      for (int u = 0; u < kAhead; ++u)
        if (k + u < r.n) {
          double *w = a.work + work_index(a, s, k + u, ch);
#pragma unroll
          for (int i = 0; i < 4; ++i) w[i] = st[i];
          loudness_carry(a.m, z[u], st);
        }
    }
    if (a.state_out) {
#pragma unroll
      for (int i = 0; i < 4; ++i) a.state_out[c * 4 + i] = st[i];
    }
    if (a.hops_out && ch == 0) a.hops_out[s] = r.n;
  }
}

typedef void (*PassKernel)(LoudnessArgs, int);

// pass1 / pass3: the pass kernels, where they are not the generic ones
template <typename S>
hipError_t launch_src(hipStream_t stream, const LoudnessArgs &a, PassKernel pass1 = loudness_pass_kernel<S, false>,
                      PassKernel pass3 = loudness_pass_kernel<S, true>)
{
  // workgroups of the longest row (max_hops * nch < 2^60); the kernel strides over what a full grid leaves
  const unsigned long long groups = (a.max_hops * (unsigned long long)a.nch + kThreads - 1) / kThreads;
  const unsigned gx = groups > 0x7fffffffull ? 0x7fffffffu : (unsigned)groups;
  const unsigned long long chans = (unsigned long long)a.nstreams * (unsigned long long)a.nch;
  const unsigned long long cb = (chans + kCarryThreads - 1) / kCarryThreads;
  for (int pass = 0; pass < 3; ++pass) {
    if (pass == 1) {
      hipLaunchKernelGGL((loudness_carry_kernel<S>), dim3(cb > 0x7fffffffull ? 0x7fffffffu : (unsigned)cb), dim3(kCarryThreads), 0, stream, a);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
      continue;
    }
    if (!gx) continue; // no whole hop: the carry alone hands the state on
    for (int s0 = 0; s0 < a.nstreams; s0 += 32768) { // grid.y is a 16-bit count
      const int ns = a.nstreams - s0 < 32768 ? a.nstreams - s0 : 32768;
      const dim3 grid(gx, (unsigned)ns), block(kThreads);
      hipLaunchKernelGGL(pass == 0 ? pass1 : pass3, grid, block, 0, stream, a, s0);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
    }
  }
  return hipSuccess;
}

template <typename S> void host_src(const LoudnessArgs &a)
{
  const unsigned nch = (unsigned)a.nch;
  for (unsigned long long s = 0; s < (unsigned long long)a.nstreams; ++s) {
    const Row<S> r = row_of<S>(a, s);
    for (unsigned ch = 0; ch < nch; ++ch) {
      const unsigned long long c = s * nch + ch;
      for (int pass = 0; pass < 3; ++pass) {
        double st[4] = {0.0, 0.0, 0.0, 0.0};
        if (pass == 1 && a.state_in)
          for (int i = 0; i < 4; ++i) st[i] = a.state_in[c * 4 + i];
        for (unsigned long long k = 0; k < r.n; ++k) {
          double *w = a.work + work_index(a, s, k, ch);
          if (pass == 1) {
            double z[4];
            for (int i = 0; i < 4; ++i) {
              z[i] = w[i];
              w[i] = st[i];
            }
            loudness_carry(a.m, z, st);
            continue;
          }
          double energy = 0.0;
          for (int i = 0; i < 4; ++i) st[i] = pass ? w[i] : 0.0;
          for (unsigned long long i = 0; i < a.hop; ++i) {
            const double v = loudness_step(a.c, gained_at(r, (k * a.hop + i) * nch + ch), st);
            energy = energy + v * v;
          }
          if (pass) a.energy[c * a.energy_stride + a.first_hop + k] = energy;
          else
            for (int i = 0; i < 4; ++i) w[i] = st[i];
        }
        if (pass == 1 && a.state_out)
          for (int i = 0; i < 4; ++i) a.state_out[c * 4 + i] = st[i];
      }
    }
    if (a.hops_out) a.hops_out[s] = r.n;
  }
}

// The gate: one workgroup per stream.  The blocks z_j are computed kThreads at a time into LDS; lane 0 adds up the ones that
// pass, ascending, once for the absolute gate and -- the z_j computed again, to the same bits -- once for both gates.
__global__ __launch_bounds__(kThreads) void loudness_gate_kernel(LoudnessGateArgs a)
{
  __shared__ double z[kThreads];
  __shared__ double sh_t;
  const unsigned tid = threadIdx.x;
  const unsigned long long s = blockIdx.x;
  unsigned long long n = a.nhops;
  if (a.hops && a.hops[s] < n) n = a.hops[s];
  const unsigned long long nb = n < 4 ? 0 : n - 3;
  const double *e = a.energy + s * (unsigned long long)a.nch * a.energy_stride;
  double sum[2] = {0.0, 0.0}, cnt[2] = {0.0, 0.0};
  for (int pass = 0; pass < 2; ++pass) {
    unsigned long long count = 0;
    const double t = pass ? sh_t : 0.0;
    for (unsigned long long j0 = 0; j0 < nb; j0 += kThreads) {
      const unsigned m = nb - j0 < (unsigned long long)kThreads ? (unsigned)(nb - j0) : (unsigned)kThreads;
      __syncthreads(); // lane 0 is done with the tile before
      if (tid < m) z[tid] = loudness_block(a, e, j0 + tid);
      __syncthreads();
      if (tid == 0)
        for (unsigned j = 0; j < m; ++j) {
          const double v = z[j];
          if (v > a.abs_threshold && (!pass || v > t)) {
            sum[pass] = sum[pass] + v;
            ++count;
          }
        }
    }
    cnt[pass] = (double)count;
    if (!pass) {
      if (tid == 0) sh_t = a.rel_factor * (sum[0] / cnt[0]);
      __syncthreads();
    }
  }
  if (tid == 0) {
    double *out = a.result + s * 4;
    out[0] = sum[1];
    out[1] = cnt[1];
    out[2] = sum[0];
    out[3] = cnt[0];
  }
}

} // namespace

hipError_t launch_loudness(hipStream_t stream, const LoudnessArgs &a)
{
  return a.src_double ? launch_src<double>(stream, a) : launch_src<float>(stream, a);
}

void loudness_host(const LoudnessArgs &a)
{
  if (a.src_double) host_src<double>(a);
  else host_src<float>(a);
}

hipError_t launch_loudness_packed(hipStream_t stream, const LoudnessArgs &a, int kind)
{
  switch (kind) {
  case kTracksSrcS16: return launch_src<TracksPacked<short>>(stream, a);
  case kTracksSrcS24: // mono and stereo: the dword form
    if (a.nch == 1) return launch_src<TracksPacked<TracksS24>>(stream, a, loudness_pass_s24_kernel<1, false>, loudness_pass_s24_kernel<1, true>);
    if (a.nch == 2) return launch_src<TracksPacked<TracksS24>>(stream, a, loudness_pass_s24_kernel<2, false>, loudness_pass_s24_kernel<2, true>);
    return launch_src<TracksPacked<TracksS24>>(stream, a);
  case kTracksSrcS32: return launch_src<TracksPacked<int>>(stream, a);
  default: return launch_src<TracksPacked<float>>(stream, a);
  }
}

void loudness_packed_host(const LoudnessArgs &a, int kind)
{
  switch (kind) {
  case kTracksSrcS16: return host_src<TracksPacked<short>>(a);
  case kTracksSrcS24: return host_src<TracksPacked<TracksS24>>(a);
  case kTracksSrcS32: return host_src<TracksPacked<int>>(a);
  default: return host_src<TracksPacked<float>>(a);
  }
}

hipError_t launch_loudness_gate(hipStream_t stream, const LoudnessGateArgs &a)
{
  hipLaunchKernelGGL(loudness_gate_kernel, dim3((unsigned)a.nstreams), dim3(kThreads), 0, stream, a);
  return hipGetLastError();
}

void loudness_gate_host(const LoudnessGateArgs &a)
{
  for (unsigned long long s = 0; s < (unsigned long long)a.nstreams; ++s) {
    unsigned long long n = a.nhops;
    if (a.hops && a.hops[s] < n) n = a.hops[s];
    const unsigned long long nb = n < 4 ? 0 : n - 3;
    const double *e = a.energy + s * (unsigned long long)a.nch * a.energy_stride;
    double sum[2] = {0.0, 0.0}, cnt[2] = {0.0, 0.0}, t = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
      unsigned long long count = 0;
      for (unsigned long long j = 0; j < nb; ++j) {
        const double v = loudness_block(a, e, j);
        if (v > a.abs_threshold && (!pass || v > t)) {
          sum[pass] = sum[pass] + v;
          ++count;
        }
      }
      cnt[pass] = (double)count;
      if (!pass) t = a.rel_factor * (sum[0] / cnt[0]);
    }
    double *out = a.result + s * 4;
    out[0] = sum[1];
    out[1] = cnt[1];
    out[2] = sum[0];
    out[3] = cnt[0];
  }
}

} // namespace rsmp
