// Output stage for device-resident frames: one streaming pass over the float32 / float64 frames a handle produced
// that applies a per-stream gain, adds deterministic TPDF dither, quantises to S16, packed S24 or S32 and takes, per (stream,
// channel), the peak and the number of clipped samples.  The arithmetic is finish_sample (finish.hpp), shared with the host twin
// at the end of this file.
//
// Shape: grid = (chunk of a stream's row, stream); a row is the frames * nch interleaved samples of one stream.  A row is cut into
//   head    0..3 samples, as many as it takes to bring the DESTINATION to a dword boundary (decided per row: the row pitch need
//           not keep row 0's alignment), written byte by byte by workgroup 0;
//   groups  of 4 consecutive samples, one lane each: 16 (float) or 2 x 16 (double) bytes loaded, 2 / 3 / 4 whole dwords stored.
//           Multi-dword accesses need dword alignment only, which the sample type (source) and the head (destination) give;
//   tail    the 0..3 samples left over, byte by byte by workgroup 0.
// A workgroup takes `span` samples per step and `steps` consecutive steps.  Where lcm(4, nch) <= 1024 (every channel count up to
// 256, and those multiples of 4 or 2 up to 1024 / 512), span is the largest multiple of it within 1024: the 4 samples of a lane
// then have the same 4 channels in every step, so peak and clip count stay in registers, are merged per channel in LDS when the
// workgroup is done and leave as at most one global atomic per (workgroup, channel, statistic).  Any other channel count takes
// the direct form: span = 1024, channel and frame by division per group, atomics straight to global memory (a peak only when it
// beats the value already there).
// No byte outside the frames * nch samples of a destination row is touched.
#include "finish.hpp"

#include <cstring>

namespace rsmp {
namespace {

constexpr int kThreads = 256, kSpanMax = kThreads * 4;

__device__ __forceinline__ unsigned long long peak_bits(double a) { return (unsigned long long)__double_as_longlong(a); }

// bits of a non-negative double order as unsigned integers (a NaN, sign cleared by fabs, lies above +inf and stays)
__device__ __forceinline__ void global_stats(const FinishArgs &a, unsigned long long c, unsigned long long pk, unsigned long long cl)
{
  if (a.peak && pk) {
    unsigned long long *p = reinterpret_cast<unsigned long long *>(a.peak) + c;
    if (pk > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, pk); // the value only ever grows
  }
  if (a.clipped && cl) atomicAdd(a.clipped + c, cl);
}

template <int kBits> struct Pack;
template <> struct Pack<15> {
  static constexpr int kBytes = 2, kWords = 2;
  static __device__ __forceinline__ void words(const int *q, unsigned *w)
  {
    w[0] = ((unsigned)q[0] & 0xffffu) | ((unsigned)q[1] << 16);
    w[1] = ((unsigned)q[2] & 0xffffu) | ((unsigned)q[3] << 16);
  }
};
template <> struct Pack<23> { // four 3-byte samples are three dwords
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

// S: float or double source.  kWrite = false: measure only.  kReg: statistics in registers and LDS (see the head of the file).
template <typename S, int kBits, bool kWrite, bool kReg>
__global__ __launch_bounds__(kThreads) void finish_kernel(FinishArgs a, int s0, int span, unsigned fps, int steps)
{
  __shared__ unsigned long long sh_peak[kReg ? kFinishLdsChannels : 1];
  __shared__ unsigned sh_clip[kReg ? kFinishLdsChannels : 1];
  using P = Pack<kBits>;
  const unsigned tid = threadIdx.x;
  const unsigned nch = (unsigned)a.nch;
  const unsigned long long s = (unsigned long long)(s0 + (int)blockIdx.y), n = a.n, cbase = s * nch;
  const S *src = static_cast<const S *>(a.src) + s * a.src_stride;
  unsigned char *dst = kWrite ? static_cast<unsigned char *>(a.dst) + s * a.dst_stride * P::kBytes : nullptr;
  const bool has_gain = a.gain != nullptr, dither = a.dither != 0;
  const double gain = has_gain ? a.gain[s] : 1.0;

  // the row's head: samples in front of the first dword boundary of the destination
  const unsigned long long addr = reinterpret_cast<unsigned long long>(dst);
  unsigned head = !kWrite ? 0u : kBits == 15 ? (unsigned)(addr >> 1) & 1u : kBits == 23 ? (unsigned)addr & 3u : 0u;
  if (head > n) head = (unsigned)n;
  const unsigned long long ngroups = (n - head) >> 2;
  const unsigned gps = (unsigned)span >> 2; // groups (= lanes at work) per step
  const unsigned long long step0 = (unsigned long long)blockIdx.x * (unsigned)steps;
  if (blockIdx.x != 0 && step0 * gps >= ngroups) return; // (the grid is sized from n / 4: the head can leave a workgroup without groups)

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
      const unsigned long long k = is_head ? tid : head + (ngroups << 2) + (tid - 64);
      const unsigned long long fr = k / nch;
      const unsigned ch = (unsigned)(k - fr * nch);
      const FinishSample r = finish_sample<kBits>((double)src[k], has_gain, gain, dither, a.seed, a.first_frame + fr, cbase + ch);
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
    unsigned long long frj[4], pk[4] = {0, 0, 0, 0};
    unsigned cl[4] = {0, 0, 0, 0};
    if (kReg) {
      const unsigned k0 = head + 4 * tid, f0 = k0 / nch;
      unsigned ch = k0 - f0 * nch;
      unsigned long long fr = a.first_frame + f0 + step0 * fps;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        chj[j] = ch;
        frj[j] = fr;
        if (++ch == nch) ch = 0, ++fr;
      }
    }
    for (int u = 0; u < steps; ++u) {
      const unsigned long long gi = (step0 + u) * gps + tid;
      if (gi >= ngroups) break;
      const unsigned long long k = head + (gi << 2);
      S x[4];
      __builtin_memcpy(x, src + k, sizeof(x)); // 16-byte loads: one for float, two for double
      if (!kReg) {
        const unsigned long long f0 = k / nch;
        unsigned ch = (unsigned)(k - f0 * nch);
        unsigned long long fr = a.first_frame + f0;
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
          const unsigned long long b = peak_bits(r.a);
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

unsigned long long gcd_u(unsigned long long x, unsigned long long y)
{
  while (y) {
    const unsigned long long r = x % y;
    x = y;
    y = r;
  }
  return x;
}

template <typename S, int kBits, bool kWrite>
hipError_t launch_typed(hipStream_t stream, const FinishArgs &a)
{
  const unsigned long long nch = (unsigned long long)a.nch, lcm4 = nch / gcd_u(nch, 4) * 4;
  static_assert(kFinishLdsChannels >= kSpanMax, "nch <= lcm(4, nch) <= kSpanMax has to fit the LDS table");
  const bool reg = lcm4 <= (unsigned long long)kSpanMax;
  const int span = reg ? int(kSpanMax / lcm4 * lcm4) : kSpanMax;
  const unsigned fps = reg ? unsigned(span / a.nch) : 0u;
  const unsigned long long row_steps = ((a.n + 3) / 4 + span / 4 - 1) / (span / 4);
  // steps per workgroup: as many as leave about 16 workgroups per CU on the chip, at most 32; more only to stay inside the grid
  // limit.  The caller keeps n below 2^60 (RRX_finish_device refuses more), so row_steps < 2^51 and the doubling ends at 2^20
  // steps or fewer: a workgroup sees fewer than 2^31 samples, which its 32-bit clip counts (cl[], sh_clip) hold.
  unsigned long long steps = row_steps * (unsigned long long)a.nstreams / 4096;
  steps = steps < 1 ? 1 : steps > 32 ? 32 : steps;
  while ((row_steps + steps - 1) / steps > 0x7fffffffull) steps *= 2;
  const unsigned gx = (unsigned)((row_steps + steps - 1) / steps);
  for (int s0 = 0; s0 < a.nstreams; s0 += 32768) { // grid.y is a 16-bit count
    const int ns = a.nstreams - s0 < 32768 ? a.nstreams - s0 : 32768;
    const dim3 grid(gx ? gx : 1, (unsigned)ns), block(kThreads);
    if (reg) hipLaunchKernelGGL((finish_kernel<S, kBits, kWrite, true>), grid, block, 0, stream, a, s0, span, fps, (int)steps);
    else hipLaunchKernelGGL((finish_kernel<S, kBits, kWrite, false>), grid, block, 0, stream, a, s0, span, fps, (int)steps);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

template <typename S> hipError_t launch_src(hipStream_t stream, const FinishArgs &a)
{
  if (!a.dst) return launch_typed<S, 31, false>(stream, a);
  switch (a.bits) {
  case 15: return launch_typed<S, 15, true>(stream, a);
  case 23: return launch_typed<S, 23, true>(stream, a);
  default: return launch_typed<S, 31, true>(stream, a);
  }
}

template <typename S, int kBits> void host_typed(const FinishArgs &a)
{
  constexpr int kBytes = kBits == 15 ? 2 : kBits == 23 ? 3 : 4;
  const unsigned long long nch = (unsigned long long)a.nch;
  for (unsigned long long s = 0; s < (unsigned long long)a.nstreams; ++s) {
    const S *src = static_cast<const S *>(a.src) + s * a.src_stride;
    unsigned char *dst = a.dst ? static_cast<unsigned char *>(a.dst) + s * a.dst_stride * kBytes : nullptr;
    const double gain = a.gain ? a.gain[s] : 1.0;
    for (unsigned long long k = 0; k < a.n; ++k) {
      const unsigned long long fr = k / nch, c = s * nch + (k - fr * nch);
      const FinishSample r = finish_sample<kBits>((double)src[k], a.gain != nullptr, gain, a.dither != 0, a.seed, a.first_frame + fr, c);
      if (dst) finish_store_bytes<kBits>(dst + k * kBytes, r.q);
      if (a.peak) {
        unsigned long long have, now;
        std::memcpy(&have, a.peak + c, 8);
        std::memcpy(&now, &r.a, 8);
        if (now > have) std::memcpy(a.peak + c, &now, 8);
      }
      if (a.clipped && r.clip) ++a.clipped[c];
    }
  }
}

template <typename S> void host_src(const FinishArgs &a)
{
  if (!a.dst || a.bits == 31) host_typed<S, 31>(a);
  else if (a.bits == 15) host_typed<S, 15>(a);
  else host_typed<S, 23>(a);
}

} // namespace

hipError_t launch_finish(hipStream_t stream, const FinishArgs &a)
{
  return a.src_double ? launch_src<double>(stream, a) : launch_src<float>(stream, a);
}

void finish_host(const FinishArgs &a)
{
  if (a.src_double) host_src<double>(a);
  else host_src<float>(a);
}

} // namespace rsmp
