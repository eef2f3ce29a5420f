// Launch entry point of the LPC edge extrapolator for device-resident frames (implemented in lpc.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

namespace rsmp {

constexpr int kLpcMaxOrder = 32;      // the plugin's LPC_ORDER (lpc/lpc.h:25); the kernel keeps this many taps in registers
constexpr int kLpcLdsFrames = 16384;  // the plugin's largest PRIME_LEN_ (foo_dsp_rate.cpp:101): windowed copy held in LDS up to here

// lpc_extrapolate2 (lpc/lpc.h:27) for every (stream, channel) of a [stream][frame][channel] float32 buffer: data = frame 0 of
// stream 0's base frames, stream_stride in frames.  Only enqueues on `stream`; the arguments are the caller's to validate
// (1 <= order <= kLpcMaxOrder < data_len, nstreams * nch fits a grid).
hipError_t launch_lpc_extrapolate(hipStream_t stream, float *data, size_t stream_stride, int nstreams, size_t data_len, int nch,
                                  int order, size_t extra_bkwd, size_t extra_fwd);

} // namespace rsmp
