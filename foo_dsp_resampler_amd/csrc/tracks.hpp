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
// sample-by-sample paths, the LPC base-frame loads (tracks.hip) and the host loop behind RRX_debug_tracks_load_host (capi_stage.cpp) all
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

// The measuring path (RRX_tracks_true_peak_packed_device / RRX_tracks_loudness_packed_device, include/ratelib_amd.h) reads a
// packed source as the meters' fp64: v = (double)s * 2^-bits, bits = 15 / 23 / 31, or (double)x for float32.  This is exact for
// all four kinds, and for S32 deliberately NOT the stage pass's value above, which is rounded to float32: a meter measures what the
// file holds, so INT32_MAX is 1 - 2^-31 and not 1.0.  One sample as it is stored is a float, short, TracksS24 or int; the
// kernels keep samples in flight in that form and convert where they use them.
struct TracksS24 {
  unsigned char b[3]; // little endian, two's complement
};

__host__ __device__ __forceinline__ double tracks_value(float x) { return (double)x; }
__host__ __device__ __forceinline__ double tracks_value(double x) { return x; } // (the rows of the row forms)
__host__ __device__ __forceinline__ double tracks_value(short s) { return (double)s * 0x1p-15; }
__host__ __device__ __forceinline__ double tracks_value(int s) { return (double)s * 0x1p-31; }
__host__ __device__ __forceinline__ double tracks_value_s24(int s) { return (double)s * 0x1p-23; } // s: the sign-extended sample
__host__ __device__ __forceinline__ double tracks_value(TracksS24 r)
{
  return tracks_value_s24((int)r.b[0] | ((int)r.b[1] << 8) | (int)(signed char)r.b[2] * 65536);
}

// Sample i of a packed source at `base` as that double: tracks_load_sample's switch for the measuring path.  The kernels
// (true_peak.hip, loudness.hip: instantiated per kind, through the same tracks_value) and the host twins behind
// RRX_debug_tracks_true_peak_packed_host / RRX_debug_tracks_loudness_packed_host share it.  `base` needs the alignment of one
// sample (1 byte for S24); exactly the sample's own bytes are read.
__host__ __device__ __forceinline__ double tracks_load_value(int kind, const void *base, unsigned long long i)
{
  switch (kind) {
  case kTracksSrcS16: return tracks_value(static_cast<const short *>(base)[i]);
  case kTracksSrcS24: return tracks_value(static_cast<const TracksS24 *>(base)[i]);
  case kTracksSrcS32: return tracks_value(static_cast<const int *>(base)[i]);
  default: return tracks_value(static_cast<const float *>(base)[i]);
  }
}

// What the measuring kernels are instantiated on: S = float / double are rows of the row forms, Packed<R> a packed source whose
// samples are stored as R.  (A tag and not a flag, so that the row forms' instantiations keep their names.)
template <typename R> struct TracksPacked {};
template <typename S> struct TracksSrcOf {
  using raw = S;
  static constexpr bool packed = false;
};
template <typename R> struct TracksSrcOf<TracksPacked<R>> {
  using raw = R;
  static constexpr bool packed = true;
};
template <typename R> constexpr int tracks_kind_of();
template <> constexpr int tracks_kind_of<float>() { return kTracksSrcF32; }
template <> constexpr int tracks_kind_of<short>() { return kTracksSrcS16; }
template <> constexpr int tracks_kind_of<TracksS24>() { return kTracksSrcS24; }
template <> constexpr int tracks_kind_of<int>() { return kTracksSrcS32; }

// ------------------------------------------------------------------------------------------------------ interval arithmetic
// Everything the kernels take from a table entry goes through the four functions below, which hold all the u64 clamps against
// wrap-around: the whole-row kernels call tracks_entry / tracks_slice, the window kernels tracks_stage_cut / tracks_finish_cut,
// which are built on them, and RRX_debug_tracks_window_cut (capi_stage.cpp) runs the same functions on the host.

// Track t's input side, clamped: lead + frames + fwd <= row_frames and first + have <= src_total whatever the table says
struct TracksEntry {
  unsigned long long first, have; // the track's frames in the packed source: [first, first + have), have <= frames
  unsigned long long lead, frames, fwd;
};

__host__ __device__ __forceinline__ TracksEntry tracks_entry(const Track &tr, unsigned long long row_frames, unsigned long long src_total)
{
  TracksEntry e;
  e.lead = tr.lead < row_frames ? tr.lead : row_frames;
  e.frames = tr.frames < row_frames - e.lead ? tr.frames : row_frames - e.lead;
  e.fwd = e.lead < row_frames - e.lead - e.frames ? e.lead : row_frames - e.lead - e.frames;
  e.first = tr.src_first < src_total ? tr.src_first : src_total;
  e.have = e.frames < src_total - e.first ? e.frames : src_total - e.first;
  return e;
}

// Frames [first, first + frames) of rows of row_frames frames: what the window calls work on.  first + frames <= row_frames
// (the callers of the kernels refuse anything else), so no sum below can wrap.
struct TracksWindow {
  unsigned long long first, frames;
  unsigned long long stride;      // pitch of the window rows in frames, >= frames (the cut functions do not look at it)
};

// [lo, hi) of a row, lo <= hi <= row_frames, cut to the window and counted from the window's first frame
__host__ __device__ __forceinline__ void tracks_window_range(const TracksWindow &w, unsigned long long lo, unsigned long long hi,
                                                             unsigned long long *out)
{
  const unsigned long long end = w.first + w.frames;
  out[0] = (lo < w.first ? w.first : lo < end ? lo : end) - w.first;
  out[1] = (hi < w.first ? w.first : hi < end ? hi : end) - w.first;
}

// The stage pass of one track inside a window: the four regions of its row (tracks.hip), each cut to the window, as half-open
// ranges of WINDOW frames.  They are adjacent, in this order, and cover [0, w.frames) exactly: bk[0] == 0, bk[1] == cp[0],
// cp[1] == fw[0], fw[1] == z[0], z[1] == w.frames.
struct TracksStageCut {
  TracksEntry e;
  unsigned long long bk[2], cp[2], fw[2], z[2]; // backward extension, the track, forward extension, zeros
  unsigned long long src_frame;                  // frame of the packed source that window frame cp[0] is a copy of (cp empty: e.first)
  unsigned long long readable;                   // of the frames [cp[0], cp[1]), the first `readable` lie inside the source; the rest read as zeros
};

__host__ __device__ __forceinline__ TracksStageCut tracks_stage_cut(const Track &tr, unsigned long long row_frames, unsigned long long src_total,
                                                                    const TracksWindow &w)
{
  TracksStageCut c;
  c.e = tracks_entry(tr, row_frames, src_total);
  const unsigned long long c0 = c.e.lead, c1 = c0 + c.e.frames, z0 = c1 + c.e.fwd; // <= row_frames by the clamps
  tracks_window_range(w, 0, c0, c.bk);
  tracks_window_range(w, c0, c1, c.cp);
  tracks_window_range(w, c1, z0, c.fw);
  tracks_window_range(w, z0, row_frames, c.z);
  const unsigned long long n = c.cp[1] - c.cp[0], off = n ? w.first + c.cp[0] - c0 : 0; // frame of the track that comes first
  c.src_frame = c.e.first + off;                                                        // (<= src_total + row_frames)
  c.readable = c.e.have > off ? (c.e.have - off < n ? c.e.have - off : n) : 0;
  return c;
}

// Track t's output side, clamped: its slice [of, of + frames) lies inside its row and (when written) [df, df + frames) inside the
// destination
struct TracksSlice {
  unsigned long long of, df, frames;
};

__host__ __device__ __forceinline__ TracksSlice tracks_slice(const Track &tr, unsigned long long row_frames, unsigned long long dst_total, bool write)
{
  TracksSlice s;
  s.of = tr.out_first < row_frames ? tr.out_first : row_frames;
  s.df = !write ? 0 : tr.dst_first < dst_total ? tr.dst_first : dst_total;
  s.frames = tr.out_frames < row_frames - s.of ? tr.out_frames : row_frames - s.of;
  if (write && s.frames > dst_total - s.df) s.frames = dst_total - s.df;
  return s;
}

// Track t measured at rest in the packed source (the packed meter calls): only the input side of its entry counts.  first +
// frames <= src_total and frames <= max_frames whatever the table says, so a wrong table gives wrong numbers, never a read outside
// the source.  The kernels and the host twins both call this.
struct TracksPackedCut {
  unsigned long long first, frames;
};

__host__ __device__ __forceinline__ TracksPackedCut tracks_packed_cut(const Track &tr, unsigned long long src_total, unsigned long long max_frames)
{
  TracksPackedCut c;
  c.first = tr.src_first < src_total ? tr.src_first : src_total;
  c.frames = tr.frames < src_total - c.first ? tr.frames : src_total - c.first;
  if (c.frames > max_frames) c.frames = max_frames;
  return c;
}

// The output stage of one track inside a window: window frames [w0, w1) are frames index, index + 1, ... of the track's slice
// (the frame number its dither is keyed by) and go to frames dst_frame, dst_frame + 1, ... of the packed destination.  A slice
// that does not meet the window gives all zeros.
struct TracksFinishCut {
  unsigned long long w0, w1, index, dst_frame;
};

__host__ __device__ __forceinline__ TracksFinishCut tracks_finish_cut(const Track &tr, unsigned long long row_frames, unsigned long long dst_total,
                                                                      bool write, const TracksWindow &w)
{
  const TracksSlice s = tracks_slice(tr, row_frames, dst_total, write);
  const unsigned long long end = w.first + w.frames, lo = s.of > w.first ? s.of : w.first, hi = s.of + s.frames < end ? s.of + s.frames : end;
  TracksFinishCut c = {0, 0, 0, 0};
  if (hi > lo) {
    c.w0 = lo - w.first;
    c.w1 = hi - w.first;
    c.index = lo - s.of;
    c.dst_frame = s.df + c.index;
  }
  return c;
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
// The window forms (RRX_tracks_stage_window_device / RRX_tracks_finish_window_device): a.rows / a.src is the window buffer
// [ntracks][w.stride][nch], a.row_frames the length of the virtual rows, of which no buffer exists; frames [w.first, w.first +
// w.frames) of every row are written / read, and nothing else of the window buffer.  w.frames > 0.
hipError_t launch_tracks_stage_window(hipStream_t stream, const TracksStageArgs &a, const TracksWindow &w);
hipError_t launch_tracks_finish_window(hipStream_t stream, const TracksFinishArgs &a, const TracksWindow &w);

} // namespace rsmp
