// LPC edge extrapolation for device-resident frames: lpc_extrapolate2 of the reference (lpc/lpc.cpp:25-191) for every
// (stream, channel) of an interleaved float32 buffer, bit for bit.
//
// The arithmetic is tiny; what fixes the bits is its ORDER, so the order is the reference's everywhere:
//   window      float, every operation rounded on its own (this file is compiled with -ffp-contract=off)          :80-88
//   autocorr    fp64, one lane per lag, each lag ONE serial ascending sum of exact products                       :91-105
//   Levinson    fp64, one lane, the reference's loops as they stand (early stop, in-place update, damping)       :107-160
//   recursion   float, one lane per direction, taps in ascending order, the +-10 clamp in the reference's form    :162-191
// One 64-lane workgroup per (stream, channel): parallel over lags, directions, channels and streams, never inside a sum.
// The per-channel body is lpc_channel (lpc_body.hpp), shared with the stage kernel of tracks.hip.
#include "lpc_body.hpp"

#include "kernels.hpp"

namespace rsmp {
namespace {

// kLds: the windowed copy of the channel lives in LDS (data_len <= kLpcLdsFrames); otherwise every use recomputes the window
// from global memory (the same float operations, so the same bits).
template <bool kLds>
__global__ __launch_bounds__(64) void lpc_extrapolate_kernel(float *data, long long stream_stride, int nch, long long n, float n2,
                                                              int order, long long bk, long long fw)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char lpc_lds[];
  float *x = data + (long long)(blockIdx.x / nch) * stream_stride + blockIdx.x % nch; // frame i of this channel: x[i * nch]
  lpc_channel<kLds>(lpc_lds, threadIdx.x, n, n2, order, bk, fw, [=](long long i) { return x[i * nch]; },
                    [=](long long i, float v) { x[i * nch] = v; });
}

} // namespace

hipError_t launch_lpc_extrapolate(hipStream_t stream, float *data, size_t stream_stride, int nstreams, size_t data_len, int nch,
                                  int order, size_t extra_bkwd, size_t extra_fwd)
{
  const bool lds = data_len <= size_t(kLpcLdsFrames);
  const size_t bytes = sizeof(LpcShared) + (lds ? data_len * sizeof(float) : 0);
  const float n2 = (data_len + 1) / 2.0f; // :82, as written
  const dim3 grid((unsigned)((long long)nstreams * nch)), block(64);
  const long long stride = (long long)stream_stride * nch;
  if (lds) {
    static DynLdsOnce once;
    hipError_t e = once.set(reinterpret_cast<const void *>(&lpc_extrapolate_kernel<true>),
                            int(sizeof(LpcShared) + kLpcLdsFrames * sizeof(float)));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lpc_extrapolate_kernel<true>, grid, block, bytes, stream, data, stride, nch, (long long)data_len, n2, order,
                       (long long)extra_bkwd, (long long)extra_fwd);
  } else {
    hipLaunchKernelGGL(lpc_extrapolate_kernel<false>, grid, block, bytes, stream, data, stride, nch, (long long)data_len, n2, order,
                       (long long)extra_bkwd, (long long)extra_fwd);
  }
  return hipGetLastError();
}

} // namespace rsmp
