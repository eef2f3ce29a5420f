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

// what RRX_tracks_stage_device was given, after validation
struct TracksStageArgs {
  const Track *tracks;                     // [ntracks], on the device
  const float *src;                        // packed tracks: [src_total][nch]
  float *rows;                             // [ntracks][row_frames][nch]
  unsigned long long src_total, row_frames; // frames
  int ntracks, nch;
  int prime_len;                           // base frames the extrapolator looks at (RRX_edge_geometry), at most kLpcLdsFrames
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

// Both only enqueue on `stream` (two kernels for the stage, one for the output stage, each split into as many launches as the
// grid limits ask for); the arguments are the caller's to validate.  The table cannot be: the kernels clamp what they take from
// it, so a wrong entry gives wrong samples and never an access outside src, the track's own row, or dst.
hipError_t launch_tracks_stage(hipStream_t stream, const TracksStageArgs &a);
hipError_t launch_tracks_finish(hipStream_t stream, const TracksFinishArgs &a);

} // namespace rsmp
