// Ragged track batches: tracks of unequal length around one batch handle.  The stage kernels turn the packed
// tracks into the rows the handle is pushed from (copy, LPC extension at each track's own ends, zeros behind it); the ragged
// output stage is finish_sample (finish.hpp) per track, from the handle's output rows into one packed destination.  Both read a
// table of Track entries that lives on the device (implemented in tracks.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

namespace rsmp {

// RRX_track of include/ratelib_amd.h, field for field; all in frames
struct Track {
  unsigned long long src_first, frames, lead, out_first, out_frames, dst_first;
};

// What the packed source of the stage pass holds (RRX_tracks_stage_device_samples): float32, or integer PCM at rest.  The rows
// are float32 whatever the source is, because the LPC arithmetic is; RRX_FMT_DOUBLE sources are not offered for that reason.
enum TracksSrc : int { kTracksSrcF32 = 0, kTracksSrcS16 = 1, kTracksSrcS24 = 2, kTracksSrcS32 = 3 };

constexpr int tracks_src_bytes(int kind) { return kind == kTracksSrcS16 ? 2 : kind == kTracksSrcS24 ? 3 : 4; }

// Sample i of a packed source at `base`, as the float32 the rows hold.  This conversion is part of the ABI of
// RRX_tracks_stage_device_samples (include/ratelib_amd.h): x = (float)((double)s * 2^-bits), bits = 15 / 23 / 31, one rounding to
// nearest even.  S16 and S24 (three bytes, little endian, two's complement, sign-extended) are exact; S32 is rounded to float32's
// 24 bits by the int -> float conversion, the scaling by a power of two is exact, and INT32_MAX becomes 1.0f.  The stage kernels'
// sample-by-sample paths, the LPC base-frame loads (tracks.hip) and the host loop behind RRX_debug_tracks_load_host (capi.cpp) all
// call this function, so they cannot drift apart; the copy kernel's group path unpacks whole dwords to the same integers.
// `base` needs the alignment of one sample (1 byte for S24); exactly the sample's own bytes are read.
__host__ __device__ __forceinline__ float tracks_load_sample(int kind, const void *base, unsigned long long i)
{
  switch (kind) {
  case kTracksSrcS16: return (float)static_cast<const short *>(base)[i] * 0x1p-15f;
  case kTracksSrcS24: {
    const unsigned char *p = static_cast<const unsigned char *>(base) + i * 3;
    const int s = (int)p[0] | ((int)p[1] << 8) | (int)(signed char)p[2] * 65536;
    return (float)s * 0x1p-23f;
  }
  case kTracksSrcS32: return (float)static_cast<const int *>(base)[i] * 0x1p-31f;
  default: return static_cast<const float *>(base)[i];
  }
}

// what RRX_tracks_stage_device_samples was given, after validation
struct TracksStageArgs {
  const Track *tracks;                     // [ntracks], on the device
  const void *src;                         // packed tracks: [src_total][nch] samples of src_kind
  float *rows;                             // [ntracks][row_frames][nch]
  unsigned long long src_total, row_frames; // frames
  int ntracks, nch;
  int prime_len;                           // base frames the extrapolator looks at (RRX_edge_geometry), at most kLpcLdsFrames
  int src_kind;                            // TracksSrc
};

// what RRX_tracks_finish_device was given, after validation
struct TracksFinishArgs {
  const Track *tracks;                     // [ntracks], on the device
  const void *src;                         // output rows [ntracks][row_frames][nch]: float (src_double = 0) or double
  void *dst;                               // packed destination [dst_total][nch]; null: measure only
  const double *gain;                      // [ntracks], null = unity
  double *peak;                            // [ntracks * nch], null = not taken
  unsigned long long *clipped;             // [ntracks * nch], null = not taken
  unsigned long long row_frames, dst_total; // frames
  unsigned long long seed;
  int ntracks, nch;
  int src_double;
  int bits;                                // 15 / 23 / 31: S16, packed S24, S32 (measure only: 31)
  int dither;
};

// Both only enqueue on `stream` (two kernels for the stage, picked by src_kind, one for the output stage, each split into as many
// launches as the grid limits ask for); the arguments are the caller's to validate.  The table cannot be: the kernels clamp what they take from
// it, so a wrong entry gives wrong samples and never an access outside src, the track's own row, or dst.
// Reads of an integer source: the copy kernel's group path loads the aligned dwords that cover a group of 4 samples, so it may read
// the whole aligned dword that holds the first or the last byte of the source (the same page: it cannot fault) and nothing further
// out; every other path reads exactly the bytes of the samples it uses.
hipError_t launch_tracks_stage(hipStream_t stream, const TracksStageArgs &a);
hipError_t launch_tracks_finish(hipStream_t stream, const TracksFinishArgs &a);

} // namespace rsmp
