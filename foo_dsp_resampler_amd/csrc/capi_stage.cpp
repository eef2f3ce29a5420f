// C ABI: the handle-free calls of include/ratelib_amd.h -- LPC edge extrapolation, the output stage and its shaped form, ragged
// track batches, true peak, the limiter and its release, loudness and its statistics, the window families of the track path, and
// channel mixing.
// A device entry validates its arguments (the family's *_args function) and ends in on_device; its host twin, a test hook, hands
// the same *_args function to on_host.  Everything that can be refused from the arguments alone is refused before any device is
// touched.
#include "../../include/ratelib_amd.h"
#include "../../include/ratelib_amd_album.h"

#include "capi_common.hpp"
#include "engine.hpp"
#include "finish.hpp"
#include "finish_shaped.hpp"
#include "loudness.hpp"
#include "loudness_stats.hpp"
#include "lpc.hpp"
#include "measure_window.hpp"
#include "tracks.hpp"
#include "tracks_album.hpp"
#include "tracks_mix.hpp"
#include "true_peak.hpp"
#include "limit.hpp"
#include "limit_release.hpp"
#include "limit_release_window.hpp"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

// The library's dynamic symbol table lists the C names of the helpers that came here from capi.cpp (an unnamed namespace inside
// extern "C" does not keep them out of it), and it stays as it was: those helpers keep their names and their linkage.  What is
// new in this file adds nothing to the table: it is outside extern "C", a template, or static.
extern "C" {
namespace {

// the device argument of a handle-free device call: RR_OK, or what the call returns
int check_device(int device)
{
  if (device >= 0) { // as RRX_open_batch_on
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) return RR_EXTUNINIT;
    if (device >= n) return RR_INVPARAM;
  }
  return rsmp::device_is_gfx950(device) ? RR_OK : RR_EXTUNINIT;
}

bool pcm_format(int f) { return f == RRX_FMT_S16 || f == RRX_FMT_S24_3 || f == RRX_FMT_S32; }
int pcm_bits(int f) { return f == RRX_FMT_S16 ? 15 : f == RRX_FMT_S24_3 ? 23 : 31; }

} // namespace
} // extern "C"

namespace {

// How every device entry ends once its own arguments are accepted.  The order is public behaviour (tests/test_*_api.py count it
// per family): RR_INVPARAM before RR_EXTUNINIT before the RR_OK of an empty call before anything asks for a device.  `launch`
// returns a hipError_t.
template <class Launch> int on_device(int device, bool nothing_to_do, Launch launch)
{
  if (device < -1) return RR_INVPARAM;
  if (!rsmp::ratelib_initialized()) return RR_EXTUNINIT;
  if (nothing_to_do) return RR_OK;
  const int dev = check_device(device);
  if (dev != RR_OK) return dev;
  rsmp::DeviceScope on(device); // restores the caller's device on return
  if (!on.ok()) return RR_INTERNAL;
  return launch() == hipSuccess ? RR_OK : RR_INTERNAL;
}

// How every host twin of a device entry goes: refused unless the test hooks are on, then the entry's own `args` (its *_args call,
// which returns an RR_* code), then the host function unless there is nothing to do.
template <class Args, class Host> int on_host(Args args, bool nothing_to_do, Host host)
{
  if (!rsmp::knobs().test_hooks) return -1;
  const int rc = args();
  if (rc != RR_OK) return rc;
  if (!nothing_to_do) host();
  return RR_OK;
}

// No buffer has 2^60 samples, so none has more than this many frames of nch channels.  With that bound frames * nch, stride * nch
// and the row offsets stream * stride * nch of the callers and the kernels (times up to 8 bytes a sample) cannot wrap, and a
// workgroup's 32-bit clip count cannot either (finish.hip, launch_typed).  Rows of a batch divide it by their number.
size_t most_frames(int nch) { return (~size_t(0) >> 4) / size_t(nch); }

bool float_format(int f) { return f == RRX_FMT_FLOAT || f == RRX_FMT_DOUBLE; }

// two state buffers of `doubles` doubles each share no byte (equal pointers overlap); a missing one overlaps nothing.  The counts
// are [streams * channels][a few] with streams * channels < 2^60: no wrap for a buffer that exists.
bool states_apart(const double *state_in, const double *state_out, uintptr_t doubles)
{
  if (!state_in || !state_out) return true;
  const uintptr_t x = reinterpret_cast<uintptr_t>(state_in), y = reinterpret_cast<uintptr_t>(state_out);
  const uintptr_t bytes = doubles * sizeof(double);
  return x < y ? y - x >= bytes : x - y >= bytes;
}

} // namespace

extern "C" {

// lpc/lpc.h:27 on device-resident frames.
int RRX_lpc_extrapolate_device(int device, void *hip_stream, fb_sample_t *d_data, size_t stream_stride, int nstreams, size_t data_len,
                               int nch, int lpc_order, size_t extra_bkwd, size_t extra_fwd)
{
  if (!d_data || nstreams < 1 || nch < 1 || lpc_order < 1 || lpc_order > rsmp::kLpcMaxOrder || data_len <= size_t(lpc_order)) return RR_INVPARAM;
  if (nstreams > 1 && stream_stride < extra_bkwd + data_len + extra_fwd) return RR_INVPARAM;
  if ((long long)nstreams * nch > 0x7fffffffLL) return RR_INVPARAM; // (one workgroup per channel of every stream)
  return on_device(device, !extra_bkwd && !extra_fwd, [&] {
    return rsmp::launch_lpc_extrapolate(static_cast<hipStream_t>(hip_stream), d_data, stream_stride, nstreams, data_len, nch, lpc_order,
                                        extra_bkwd, extra_fwd);
  });
}

namespace {

// RRX_finish_device / RRX_debug_finish_host: everything that can be refused from the arguments alone; fills `a` when it is RR_OK
int finish_args(int src_format, const void *src, size_t src_stride, int dst_format, void *dst, size_t dst_stride, int nstreams,
                size_t frames, int nch, const double *gain, int dither, unsigned long long seed, unsigned long long first_frame,
                double *peak, unsigned long long *clipped, rsmp::FinishArgs &a)
{
  if (!src || nstreams < 1 || nch < 1) return RR_INVPARAM;
  if (!float_format(src_format)) return RR_INVPARAM;
  if (dst && !pcm_format(dst_format)) return RR_INVPARAM;
  if (nstreams > 1 && (src_stride < frames || (dst && dst_stride < frames))) return RR_INVPARAM;
  if (!dst && !peak && !clipped) return RR_INVPARAM;
  if (first_frame + frames < first_frame) return RR_INVPARAM;               // the frame counter of the dither would wrap
  const size_t most = most_frames(nch);
  if (frames > most) return RR_INVPARAM;
  if (nstreams > 1 && (src_stride > most / size_t(nstreams) || (dst && dst_stride > most / size_t(nstreams)))) return RR_INVPARAM;
  a.src = src;
  a.dst = dst;
  a.gain = gain;
  a.peak = peak;
  a.clipped = clipped;
  a.src_stride = nstreams > 1 ? (unsigned long long)src_stride * nch : 0;
  a.dst_stride = nstreams > 1 ? (unsigned long long)dst_stride * nch : 0;
  a.n = (unsigned long long)frames * nch;
  a.seed = seed;
  a.first_frame = first_frame;
  a.nstreams = nstreams;
  a.nch = nch;
  a.src_double = src_format == RRX_FMT_DOUBLE;
  a.bits = dst ? pcm_bits(dst_format) : 31; // measure only: the S32 grid
  a.dither = dither != 0;
  return RR_OK;
}

} // namespace

// The output stage on device-resident frames (finish.hip).
int RRX_finish_device(int device, void *hip_stream, int src_format, const void *d_src, size_t src_stride, int dst_format, void *d_dst,
                      size_t dst_stride, int nstreams, size_t frames, int nch, const double *d_gain, int dither, unsigned long long seed,
                      unsigned long long first_frame, double *d_peak, unsigned long long *d_clipped)
{
  rsmp::FinishArgs a;
  const int rc = finish_args(src_format, d_src, src_stride, dst_format, d_dst, dst_stride, nstreams, frames, nch, d_gain, dither, seed,
                             first_frame, d_peak, d_clipped, a);
  if (rc != RR_OK) return rc;
  return on_device(device, !frames, [&] { return rsmp::launch_finish(static_cast<hipStream_t>(hip_stream), a); });
}

int RRX_debug_finish_host(int src_format, const void *src, size_t src_stride, int dst_format, void *dst, size_t dst_stride, int nstreams,
                          size_t frames, int nch, const double *gain, int dither, unsigned long long seed, unsigned long long first_frame,
                          double *peak, unsigned long long *clipped)
{
  rsmp::FinishArgs a;
  return on_host(
      [&] {
        return finish_args(src_format, src, src_stride, dst_format, dst, dst_stride, nstreams, frames, nch, gain, dither, seed, first_frame,
                           peak, clipped, a);
      },
      !frames, [&] { rsmp::finish_host(a); });
}

namespace {

// RRX_FMT_* of a packed source -> rsmp::TracksSrc, or -1: RRX_FMT_DOUBLE is no source of the stage pass (the rows are float32)
int tracks_src_kind(int src_format)
{
  switch (src_format) {
  case RRX_FMT_FLOAT: return rsmp::kTracksSrcF32;
  case RRX_FMT_S16: return rsmp::kTracksSrcS16;
  case RRX_FMT_S24_3: return rsmp::kTracksSrcS24;
  case RRX_FMT_S32: return rsmp::kTracksSrcS32;
  default: return -1;
  }
}

// RRX_tracks_stage_device_samples / RRX_tracks_stage_window_device: everything that can be refused from the arguments alone but
// the window; `rows` is the rows, or the window's buffer
static int tracks_stage_args(size_t in_rate, size_t out_rate, const RRX_track *tracks, int ntracks, int nch, int src_format, const void *packed,
                      size_t src_total, fb_sample_t *rows, size_t row_frames, rsmp::TracksStageArgs &a)
{
  static_assert(sizeof(RRX_track) == sizeof(rsmp::Track) && sizeof(RRX_track) == 6 * sizeof(unsigned long long), "RRX_track mirrors rsmp::Track");
  const int kind = tracks_src_kind(src_format);
  if (kind < 0) return RR_INVPARAM;
  if (!tracks || !packed || !rows || ntracks < 1 || nch < 1 || !in_rate || !out_rate || !row_frames) return RR_INVPARAM;
  if ((long long)ntracks * nch > 0x3fffffffLL) return RR_INVPARAM; // (two workgroups per channel of every track)
  if (src_total > most_frames(nch) || row_frames > most_frames(nch) / size_t(ntracks)) return RR_INVPARAM; // (nor has a virtual row, of which a window call holds a part)
  size_t n_add = 0, n_drop = 0, prime = 0, inbuf = 0;
  if (RRX_edge_geometry(in_rate, out_rate, &n_add, &n_drop, &prime, &inbuf) != RR_OK || prime > size_t(rsmp::kLpcLdsFrames)) return RR_INVPARAM;
  a.tracks = reinterpret_cast<const rsmp::Track *>(tracks);
  a.src = packed;
  a.rows = rows;
  a.src_total = src_total;
  a.row_frames = row_frames;
  a.ntracks = ntracks;
  a.nch = nch;
  a.prime_len = int(prime);
  a.src_kind = kind;
  return RR_OK;
}

} // namespace

// The stage pass of a ragged batch (tracks.hip).
int RRX_tracks_stage_device_samples(int device, void *hip_stream, size_t in_rate, size_t out_rate, const RRX_track *d_tracks, int ntracks,
                                    int nch, int src_format, const void *d_packed, size_t src_total, fb_sample_t *d_rows, size_t row_frames)
{
  rsmp::TracksStageArgs a;
  const int rc = tracks_stage_args(in_rate, out_rate, d_tracks, ntracks, nch, src_format, d_packed, src_total, d_rows, row_frames, a);
  if (rc != RR_OK) return rc;
  return on_device(device, false, [&] { return rsmp::launch_tracks_stage(static_cast<hipStream_t>(hip_stream), a); });
}

int RRX_tracks_stage_device(int device, void *hip_stream, size_t in_rate, size_t out_rate, const RRX_track *d_tracks, int ntracks, int nch,
                            const fb_sample_t *d_packed, size_t src_total, fb_sample_t *d_rows, size_t row_frames)
{
  return RRX_tracks_stage_device_samples(device, hip_stream, in_rate, out_rate, d_tracks, ntracks, nch, RRX_FMT_FLOAT, d_packed, src_total,
                                         d_rows, row_frames);
}

// Test hook: the conversion of RRX_tracks_stage_device_samples on host memory, a serial loop over the function the kernels call
int RRX_debug_tracks_load_host(int src_format, const void *src, size_t first_sample, size_t count, float *out)
{
  if (!rsmp::knobs().test_hooks) return -1;
  const int kind = tracks_src_kind(src_format);
  if (kind < 0 || !src || !out) return RR_INVPARAM;
  for (size_t i = 0; i < count; ++i) out[i] = rsmp::tracks_load_sample(kind, src, first_sample + i);
  return RR_OK;
}

namespace {

// The four output-stage calls of a ragged batch, plain and shaped, whole rows and windows: the refusals they share and
// rsmp::TracksFinishArgs.  `rows` is the rows, or the window's buffer; the shaped calls put their own fields on top.
static int tracks_finish_args(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *rows, size_t row_frames, int dst_format,
                       void *dst, size_t dst_total, const double *gain, int dither, unsigned long long seed, double *peak,
                       unsigned long long *clipped, rsmp::TracksFinishArgs &a)
{
  if (!tracks || !rows || ntracks < 1 || nch < 1) return RR_INVPARAM;
  if (!float_format(src_format)) return RR_INVPARAM;
  if (dst && !pcm_format(dst_format)) return RR_INVPARAM;
  if (!dst && !peak && !clipped) return RR_INVPARAM;
  if (row_frames > most_frames(nch) / size_t(ntracks) || (dst && dst_total > most_frames(nch))) return RR_INVPARAM;
  a.tracks = reinterpret_cast<const rsmp::Track *>(tracks);
  a.src = rows;
  a.dst = dst;
  a.gain = gain;
  a.peak = peak;
  a.clipped = clipped;
  a.row_frames = row_frames;
  a.dst_total = dst_total;
  a.seed = seed;
  a.ntracks = ntracks;
  a.nch = nch;
  a.src_double = src_format == RRX_FMT_DOUBLE;
  a.bits = dst ? pcm_bits(dst_format) : 31; // measure only: the S32 grid
  a.dither = dither != 0;
  return RR_OK;
}

} // namespace

// The output stage of a ragged batch (tracks.hip).
int RRX_tracks_finish_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch, int src_format,
                             const void *d_rows, size_t row_frames, int dst_format, void *d_dst, size_t dst_total, const double *d_gain,
                             int dither, unsigned long long seed, double *d_peak, unsigned long long *d_clipped)
{
  rsmp::TracksFinishArgs a;
  const int rc = tracks_finish_args(d_tracks, ntracks, nch, src_format, d_rows, row_frames, dst_format, d_dst, dst_total, d_gain, dither, seed,
                                    d_peak, d_clipped, a);
  if (rc != RR_OK) return rc;
  return on_device(device, !row_frames, [&] { return rsmp::launch_tracks_finish(static_cast<hipStream_t>(hip_stream), a); });
}

namespace {

// the filter of the shaped calls: RR_INVPARAM for a NULL pointer, an order outside 1..RRX_SHAPE_MAX_ORDER or a non-finite
// coefficient; `out` gets the coefficients, padded with zeros
int shaped_filter(const double *coefs, int order, double (&out)[rsmp::kShapeMaxOrder])
{
  static_assert(RRX_SHAPE_MAX_ORDER == rsmp::kShapeMaxOrder, "the header's constant is the kernels'");
  if (!coefs || order < 1 || order > RRX_SHAPE_MAX_ORDER) return RR_INVPARAM;
  for (int k = 0; k < rsmp::kShapeMaxOrder; ++k) {
    out[k] = k < order ? coefs[k] : 0.0;
    if (!std::isfinite(out[k])) return RR_INVPARAM;
  }
  return RR_OK;
}

// RRX_finish_shaped_device / RRX_debug_finish_shaped_host: everything that can be refused from the arguments alone
int finish_shaped_args(int src_format, const void *src, size_t src_stride, int dst_format, void *dst, size_t dst_stride, int nstreams,
                       size_t frames, int nch, const double *gain, int dither, unsigned long long seed, unsigned long long first_frame,
                       const double *coefs, int order, size_t segment, const double *state_in, double *state_out, double *peak,
                       unsigned long long *clipped, rsmp::ShapedArgs &a)
{
  if (!pcm_format(dst_format)) return RR_INVPARAM; // measure only included: the statistics are those of the write
  int rc = shaped_filter(coefs, order, a.coefs);
  if (rc != RR_OK) return rc;
  rsmp::FinishArgs f;
  rc = finish_args(src_format, src, src_stride, dst_format, dst, dst_stride, nstreams, frames, nch, gain, dither, seed, first_frame, peak,
                   clipped, f);
  if (rc != RR_OK) return rc;
  if (!state_in && !rsmp::shaped_restarts(first_frame, segment)) return RR_INVPARAM; // a call without a state begins a segment
  if (!states_apart(state_in, state_out, uintptr_t(nstreams) * uintptr_t(nch) * rsmp::kShapeMaxOrder)) return RR_INVPARAM;
  a.src = f.src;
  a.dst = f.dst;
  a.gain = f.gain;
  a.peak = f.peak;
  a.clipped = f.clipped;
  a.state_in = state_in;
  a.state_out = state_out;
  a.src_stride = f.src_stride;
  a.dst_stride = f.dst_stride;
  a.frames = frames;
  a.seed = seed;
  a.first_frame = first_frame;
  a.segment = segment;
  a.nstreams = nstreams;
  a.nch = nch;
  a.src_double = f.src_double;
  a.bits = pcm_bits(dst_format);
  a.dither = f.dither;
  a.order = order;
  return RR_OK;
}

} // namespace

// The output stage with noise-shaped dither (finish_shaped.hip).
int RRX_finish_shaped_device(int device, void *hip_stream, int src_format, const void *d_src, size_t src_stride, int dst_format, void *d_dst,
                             size_t dst_stride, int nstreams, size_t frames, int nch, const double *d_gain, int dither, unsigned long long seed,
                             unsigned long long first_frame, const double *coefs, int order, size_t segment, const double *d_state_in,
                             double *d_state_out, double *d_peak, unsigned long long *d_clipped)
{
  rsmp::ShapedArgs a;
  const int rc = finish_shaped_args(src_format, d_src, src_stride, dst_format, d_dst, dst_stride, nstreams, frames, nch, d_gain, dither, seed,
                                    first_frame, coefs, order, segment, d_state_in, d_state_out, d_peak, d_clipped, a);
  if (rc != RR_OK) return rc;
  return on_device(device, !frames, [&] { return rsmp::launch_finish_shaped(static_cast<hipStream_t>(hip_stream), a); });
}

int RRX_debug_finish_shaped_host(int src_format, const void *src, size_t src_stride, int dst_format, void *dst, size_t dst_stride, int nstreams,
                                 size_t frames, int nch, const double *gain, int dither, unsigned long long seed,
                                 unsigned long long first_frame, const double *coefs, int order, size_t segment, const double *state_in,
                                 double *state_out, double *peak, unsigned long long *clipped)
{
  rsmp::ShapedArgs a;
  return on_host(
      [&] {
        return finish_shaped_args(src_format, src, src_stride, dst_format, dst, dst_stride, nstreams, frames, nch, gain, dither, seed,
                                  first_frame, coefs, order, segment, state_in, state_out, peak, clipped, a);
      },
      !frames, [&] { rsmp::finish_shaped_host(a); });
}

namespace {

// the filter of the true-peak calls: RR_INVPARAM for a NULL pointer, a shape outside 1..RRX_TP_MAX_PHASES x 1..RRX_TP_MAX_TAPS or a
// non-finite coefficient; `out` gets the phases * taps coefficients as they are, without padding
int true_peak_filter(const double *coefs, int phases, int taps, rsmp::TruePeakFilter &out)
{
  static_assert(RRX_TP_MAX_PHASES == rsmp::kTpMaxPhases && RRX_TP_MAX_TAPS == rsmp::kTpMaxTaps, "the header's constants are the kernels'");
  if (!coefs || phases < 1 || phases > RRX_TP_MAX_PHASES || taps < 1 || taps > RRX_TP_MAX_TAPS) return RR_INVPARAM;
  for (int k = 0; k < rsmp::kTpMaxPhases * rsmp::kTpMaxTaps; ++k) {
    out.c[k] = k < phases * taps ? coefs[k] : 0.0; // (never read beyond phases * taps)
    if (!std::isfinite(out.c[k])) return RR_INVPARAM;
  }
  out.phases = phases;
  out.taps = taps;
  return RR_OK;
}

// RRX_true_peak_device / RRX_debug_true_peak_host: everything that can be refused from the arguments alone
int true_peak_args(int src_format, const void *src, size_t src_stride, int nstreams, size_t frames, int nch, const double *gain,
                   unsigned long long first_frame, const double *coefs, int phases, int taps, int flush, const double *state_in,
                   double *state_out, double *true_peak, double *peak, rsmp::TruePeakArgs &a)
{
  int rc = true_peak_filter(coefs, phases, taps, a.f);
  if (rc != RR_OK) return rc;
  rsmp::FinishArgs f; // the sizes, strides and overflow rules are RRX_finish_device's, measuring only
  rc = finish_args(src_format, src, src_stride, 0, nullptr, 0, nstreams, frames, nch, gain, 0, 0, first_frame, peak ? peak : true_peak, nullptr, f);
  if (rc != RR_OK) return rc;
  if (!state_in && first_frame) return RR_INVPARAM; // a call that does not begin the stream needs the history in front of it
  if (!states_apart(state_in, state_out, uintptr_t(nstreams) * uintptr_t(nch) * rsmp::kTpMaxTaps)) return RR_INVPARAM;
  a.src = f.src;
  a.gain = gain;
  a.state_in = first_frame ? state_in : nullptr; // in front of absolute frame 0 lies +0.0, whatever the buffer holds
  a.state_out = state_out;
  a.true_peak = true_peak;
  a.peak = peak;
  a.tracks = nullptr;
  a.src_stride = f.src_stride;
  a.frames = frames;
  a.nstreams = nstreams;
  a.nch = nch;
  a.src_double = f.src_double;
  a.flush = flush != 0;
  return RR_OK;
}

// The true peak of whole tracks, in the rows of a ragged batch or at rest in a packed source: the refusals the two share and
// rsmp::TruePeakArgs.  `src_stride` is 0 for rows and src_total for a packed source; the source's format is the caller's to check.
static int tracks_true_peak_args(const RRX_track *tracks, int ntracks, int nch, const void *src, bool src_double, size_t src_stride, size_t frames,
                          const double *gain, const double *coefs, int phases, int taps, double *true_peak, double *peak,
                          rsmp::TruePeakArgs &a)
{
  if (!tracks || !src || ntracks < 1 || nch < 1) return RR_INVPARAM;
  if (!true_peak && !peak) return RR_INVPARAM;
  const int rc = true_peak_filter(coefs, phases, taps, a.f);
  if (rc != RR_OK) return rc;
  if (frames > most_frames(nch) / size_t(ntracks)) return RR_INVPARAM;
  a.src = src;
  a.gain = gain;
  a.state_in = nullptr;
  a.state_out = nullptr;
  a.true_peak = true_peak;
  a.peak = peak;
  a.tracks = reinterpret_cast<const rsmp::Track *>(tracks);
  a.src_stride = src_stride;
  a.frames = frames;
  a.nstreams = ntracks;
  a.nch = nch;
  a.src_double = src_double;
  a.flush = 1;
  return RR_OK;
}

// RRX_tracks_true_peak_packed_device / RRX_debug_tracks_true_peak_packed_host: everything that can be refused from the arguments
// alone; `kind` is the source's rsmp::TracksSrc
int true_peak_packed_args(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *packed, size_t src_total, size_t max_frames,
                          const double *gain, const double *coefs, int phases, int taps, double *true_peak, double *peak,
                          rsmp::TruePeakArgs &a, int &kind)
{
  kind = tracks_src_kind(src_format);
  if (kind < 0) return RR_INVPARAM;
  const int rc = tracks_true_peak_args(tracks, ntracks, nch, packed, false, src_total, max_frames, gain, coefs, phases, taps, true_peak, peak, a);
  if (rc != RR_OK) return rc;
  return src_total > most_frames(nch) ? RR_INVPARAM : RR_OK;
}

} // namespace

// True peak and sample peak of device-resident frames (true_peak.hip).
int RRX_true_peak_device(int device, void *hip_stream, int src_format, const void *d_src, size_t src_stride, int nstreams, size_t frames,
                         int nch, const double *d_gain, unsigned long long first_frame, const double *coefs, int phases, int taps, int flush,
                         const double *d_state_in, double *d_state_out, double *d_true_peak, double *d_peak)
{
  rsmp::TruePeakArgs a;
  const int rc = true_peak_args(src_format, d_src, src_stride, nstreams, frames, nch, d_gain, first_frame, coefs, phases, taps, flush,
                                d_state_in, d_state_out, d_true_peak, d_peak, a);
  if (rc != RR_OK) return rc;
  return on_device(device, !frames, [&] { return rsmp::launch_true_peak(static_cast<hipStream_t>(hip_stream), a); });
}

int RRX_debug_true_peak_host(int src_format, const void *src, size_t src_stride, int nstreams, size_t frames, int nch, const double *gain,
                             unsigned long long first_frame, const double *coefs, int phases, int taps, int flush, const double *state_in,
                             double *state_out, double *true_peak, double *peak)
{
  rsmp::TruePeakArgs a;
  return on_host(
      [&] {
        return true_peak_args(src_format, src, src_stride, nstreams, frames, nch, gain, first_frame, coefs, phases, taps, flush, state_in,
                              state_out, true_peak, peak, a);
      },
      !frames, [&] { rsmp::true_peak_host(a); });
}

// RRX_true_peak_device per track of a ragged batch (true_peak.hip).
int RRX_tracks_true_peak_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch, int src_format,
                                const void *d_rows, size_t row_frames, const double *d_gain, const double *coefs, int phases, int taps,
                                double *d_true_peak, double *d_peak)
{
  rsmp::TruePeakArgs a;
  if (!float_format(src_format)) return RR_INVPARAM;
  const int rc = tracks_true_peak_args(d_tracks, ntracks, nch, d_rows, src_format == RRX_FMT_DOUBLE, 0, row_frames, d_gain, coefs, phases, taps,
                                       d_true_peak, d_peak, a);
  if (rc != RR_OK) return rc;
  return on_device(device, !row_frames, [&] { return rsmp::launch_true_peak(static_cast<hipStream_t>(hip_stream), a); });
}

// True peak and sample peak of tracks at rest in a packed source (true_peak.hip).
int RRX_tracks_true_peak_packed_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch, int src_format,
                                       const void *d_packed, size_t src_total, size_t max_frames, const double *d_gain, const double *coefs,
                                       int phases, int taps, double *d_true_peak, double *d_peak)
{
  rsmp::TruePeakArgs a;
  int kind = 0;
  const int rc = true_peak_packed_args(d_tracks, ntracks, nch, src_format, d_packed, src_total, max_frames, d_gain, coefs, phases, taps,
                                       d_true_peak, d_peak, a, kind);
  if (rc != RR_OK) return rc;
  return on_device(device, !max_frames || !src_total,
                   [&] { return rsmp::launch_true_peak_packed(static_cast<hipStream_t>(hip_stream), a, kind); });
}

int RRX_debug_tracks_true_peak_packed_host(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *packed, size_t src_total,
                                           size_t max_frames, const double *gain, const double *coefs, int phases, int taps,
                                           double *true_peak, double *peak)
{
  rsmp::TruePeakArgs a;
  int kind = 0;
  return on_host(
      [&] {
        return true_peak_packed_args(tracks, ntracks, nch, src_format, packed, src_total, max_frames, gain, coefs, phases, taps, true_peak,
                                     peak, a, kind);
      },
      !max_frames || !src_total, [&] { rsmp::true_peak_packed_host(a, kind); });
}

// r and m of every stream (limit.hip), frames + taps + lookahead doubles each: 0 for what the data calls refuse
size_t RRX_limit_work_doubles(int nstreams, size_t frames, int taps, size_t lookahead)
{
  static_assert(RRX_LIMIT_MAX_LOOKAHEAD == rsmp::kLimitMaxLookahead && RRX_LIMIT_MAX_HOLD == rsmp::kLimitMaxHold, "the header's constants are the kernels'");
  if (nstreams < 1 || taps < 1 || taps > RRX_TP_MAX_TAPS || lookahead < 1 || lookahead > RRX_LIMIT_MAX_LOOKAHEAD) return 0;
  const size_t most = size_t(1) << 60, per = 2 * size_t(nstreams); // (2^32 at the most)
  if (frames >= most / per) return 0;
  const size_t each = frames + size_t(taps) + lookahead;               // below 2^60 + 2^11
  return each >= (most + per - 1) / per ? 0 : per * each;
}

namespace {

// the limiter's own arguments, shared by all its calls: ceiling, lookahead, hold, the formats and the work buffer, of which the
// call needs `need` doubles (0: refused), `work_stride` for each of r and m; a.f is set already
int limit_scalars(int src_format, int dst_format, double ceiling, size_t lookahead, size_t hold, double *work, size_t work_doubles, size_t need,
                  unsigned long long work_stride, rsmp::LimitArgs &a)
{
  if (!float_format(dst_format)) return RR_INVPARAM;
  if (!std::isfinite(ceiling) || !(ceiling > 0)) return RR_INVPARAM;
  if (lookahead < 1 || lookahead > RRX_LIMIT_MAX_LOOKAHEAD || hold > RRX_LIMIT_MAX_HOLD) return RR_INVPARAM;
  if (!need || !work || work_doubles < need) return RR_INVPARAM;
  a.work = work;
  a.work_stride = work_stride;
  a.lookahead = (unsigned)lookahead;
  a.hold = (unsigned)hold;
  a.ceiling = ceiling;
  a.inv_l = 1.0 / (double)lookahead;
  a.src_double = src_format == RRX_FMT_DOUBLE;
  a.dst_double = dst_format == RRX_FMT_DOUBLE;
  return RR_OK;
}

// the whole-row calls: the work buffer is RRX_limit_work_doubles(nstreams, frames, taps, lookahead)
int limit_common(int src_format, int dst_format, int nstreams, size_t frames, double ceiling, size_t lookahead, size_t hold, double *work,
                 size_t work_doubles, rsmp::LimitArgs &a)
{
  return limit_scalars(src_format, dst_format, ceiling, lookahead, hold, work, work_doubles,
                       RRX_limit_work_doubles(nstreams, frames, a.f.taps, lookahead), (unsigned long long)frames + (unsigned)a.f.taps + lookahead, a);
}

// the overlap rule of the limiter: the destination is exactly the source, with its format and pitch, or shares no byte with it
bool limit_overlap_ok(const void *src, uintptr_t src_bytes, const void *dst, uintptr_t dst_bytes, bool same_layout)
{
  const uintptr_t x = reinterpret_cast<uintptr_t>(src), y = reinterpret_cast<uintptr_t>(dst);
  if (x == y) return same_layout;
  return x < y ? y - x >= src_bytes : x - y >= dst_bytes;
}

// RRX_limit_device / RRX_debug_limit_host: everything that can be refused from the arguments alone
int limit_args(int src_format, const void *src, size_t src_stride, int dst_format, void *dst, size_t dst_stride, int nstreams, size_t frames,
               int nch, const double *gain, double ceiling, const double *coefs, int phases, int taps, size_t lookahead, size_t hold,
               double *reduction, unsigned long long *limited, double *work, size_t work_doubles, rsmp::LimitArgs &a)
{
  int rc = true_peak_filter(coefs, phases, taps, a.f);
  if (rc != RR_OK) return rc;
  double none = 0.0;
  rsmp::FinishArgs f; // the sizes, strides and overflow rules of the source are RRX_finish_device's, measuring only
  rc = finish_args(src_format, src, src_stride, 0, nullptr, 0, nstreams, frames, nch, gain, 0, 0, 0, &none, nullptr, f);
  if (rc != RR_OK) return rc;
  if (!dst) return RR_INVPARAM;
  if (nstreams > 1 && (dst_stride < frames || dst_stride > most_frames(nch) / size_t(nstreams))) return RR_INVPARAM;
  rc = limit_common(src_format, dst_format, nstreams, frames, ceiling, lookahead, hold, work, work_doubles, a);
  if (rc != RR_OK) return rc;
  const uintptr_t per = uintptr_t(nch), rows = uintptr_t(nstreams - 1); // samples below 2^60 each: no wrap
  const uintptr_t sb = (rows * src_stride + frames) * per * (a.src_double ? 8 : 4), db = (rows * dst_stride + frames) * per * (a.dst_double ? 8 : 4);
  if (!limit_overlap_ok(src, sb, dst, db, src_format == dst_format && (nstreams == 1 || src_stride == dst_stride))) return RR_INVPARAM;
  a.src = src;
  a.dst = dst;
  a.gain = gain;
  a.reduction = reduction;
  a.limited = limited;
  a.tracks = nullptr;
  a.src_stride = f.src_stride;
  a.dst_stride = nstreams > 1 ? (unsigned long long)dst_stride * nch : 0;
  a.frames = frames;
  a.nstreams = nstreams;
  a.nch = nch;
  return RR_OK;
}

// RRX_tracks_limit_device / RRX_tracks_limit_release_device: everything the limiter on the whole rows of a ragged batch can refuse
// from the arguments alone, with RRX_limit_work_doubles(ntracks, row_frames, taps, lookahead) of work asked for
static int tracks_limit_args(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *rows, int dst_format, void *dst_rows,
                      size_t row_frames, const double *gain, double ceiling, const double *coefs, int phases, int taps, size_t lookahead,
                      size_t hold, double *reduction, unsigned long long *limited, double *work, size_t work_doubles, rsmp::LimitArgs &a)
{
  if (!tracks || !rows || !dst_rows || ntracks < 1 || nch < 1) return RR_INVPARAM;
  if (!float_format(src_format)) return RR_INVPARAM;
  int rc = true_peak_filter(coefs, phases, taps, a.f);
  if (rc != RR_OK) return rc;
  if (row_frames > most_frames(nch) / size_t(ntracks)) return RR_INVPARAM;
  rc = limit_common(src_format, dst_format, ntracks, row_frames, ceiling, lookahead, hold, work, work_doubles, a);
  if (rc != RR_OK) return rc;
  const uintptr_t samples = uintptr_t(ntracks) * row_frames * uintptr_t(nch);
  if (!limit_overlap_ok(rows, samples * (a.src_double ? 8 : 4), dst_rows, samples * (a.dst_double ? 8 : 4), src_format == dst_format))
    return RR_INVPARAM;
  a.src = rows;
  a.dst = dst_rows;
  a.gain = gain;
  a.reduction = reduction;
  a.limited = limited;
  a.tracks = reinterpret_cast<const rsmp::Track *>(tracks);
  a.src_stride = a.dst_stride = 0;
  a.frames = row_frames;
  a.nstreams = ntracks;
  a.nch = nch;
  return RR_OK;
}

} // namespace

// The true-peak limiter on device-resident frames (limit.hip).
int RRX_limit_device(int device, void *hip_stream, int src_format, const void *d_src, size_t src_stride, int dst_format, void *d_dst,
                     size_t dst_stride, int nstreams, size_t frames, int nch, const double *d_gain, double ceiling, const double *coefs,
                     int phases, int taps, size_t lookahead, size_t hold, double *d_reduction, unsigned long long *d_limited, double *d_work,
                     size_t work_doubles)
{
  rsmp::LimitArgs a;
  const int rc = limit_args(src_format, d_src, src_stride, dst_format, d_dst, dst_stride, nstreams, frames, nch, d_gain, ceiling, coefs, phases,
                            taps, lookahead, hold, d_reduction, d_limited, d_work, work_doubles, a);
  if (rc != RR_OK) return rc;
  return on_device(device, !frames, [&] { return rsmp::launch_limit(static_cast<hipStream_t>(hip_stream), a); });
}

int RRX_debug_limit_host(int src_format, const void *src, size_t src_stride, int dst_format, void *dst, size_t dst_stride, int nstreams,
                         size_t frames, int nch, const double *gain, double ceiling, const double *coefs, int phases, int taps,
                         size_t lookahead, size_t hold, double *reduction, unsigned long long *limited, double *work, size_t work_doubles)
{
  rsmp::LimitArgs a;
  return on_host(
      [&] {
        return limit_args(src_format, src, src_stride, dst_format, dst, dst_stride, nstreams, frames, nch, gain, ceiling, coefs, phases, taps,
                          lookahead, hold, reduction, limited, work, work_doubles, a);
      },
      !frames, [&] { rsmp::limit_host(a); });
}

// RRX_limit_device per track of a ragged batch (limit.hip).
int RRX_tracks_limit_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch, int src_format, const void *d_rows,
                            int dst_format, void *d_dst_rows, size_t row_frames, const double *d_gain, double ceiling, const double *coefs,
                            int phases, int taps, size_t lookahead, size_t hold, double *d_reduction, unsigned long long *d_limited,
                            double *d_work, size_t work_doubles)
{
  rsmp::LimitArgs a;
  const int rc = tracks_limit_args(d_tracks, ntracks, nch, src_format, d_rows, dst_format, d_dst_rows, row_frames, d_gain, ceiling, coefs, phases,
                                   taps, lookahead, hold, d_reduction, d_limited, d_work, work_doubles, a);
  if (rc != RR_OK) return rc;
  return on_device(device, !row_frames, [&] { return rsmp::launch_limit(static_cast<hipStream_t>(hip_stream), a); });
}

// r, m and the block summaries C, A, B, S of every stream (limit_release.hip): 0 for what the data calls refuse
size_t RRX_limit_release_work_doubles(int nstreams, size_t frames, int taps, size_t lookahead, size_t block)
{
  static_assert(RRX_LIMIT_RELEASE_MIN_BLOCK == rsmp::kLimitReleaseMinBlock && RRX_LIMIT_RELEASE_MAX_BLOCK == rsmp::kLimitReleaseMaxBlock,
                "the header's constants are the kernels'");
  if (block < RRX_LIMIT_RELEASE_MIN_BLOCK || block > RRX_LIMIT_RELEASE_MAX_BLOCK) return 0;
  if (!RRX_limit_work_doubles(nstreams, frames, taps, lookahead)) return 0; // (frames below 2^60 / (2 * nstreams) from here on)
  const size_t most = size_t(1) << 60, n = size_t(nstreams);
  const size_t each = 2 * (frames + size_t(taps) + lookahead) + 4 * ((frames + lookahead - 1 + block - 1) / block + 1); // below 2^61
  return each >= (most + n - 1) / n ? 0 : n * each;
}

namespace {

// what the release adds to a validated limiter call: the pole, the block, and the work buffer's layout.  Per stream r, C, A in
// the first half and m, B, S in the second, each half `a.work_stride` doubles: limit.hip's kernels find r and m where they
// look for them.
int limit_release_args(double release, size_t block, double *work, size_t work_doubles, rsmp::LimitArgs &a, rsmp::LimitReleaseArgs &r)
{
  if (!(release >= 0.0) || !(release < 1.0)) return RR_INVPARAM; // (a NaN fails both)
  const size_t need = RRX_limit_release_work_doubles(a.nstreams, size_t(a.frames), a.f.taps, a.lookahead, block);
  if (!need || !work || work_doubles < need) return RR_INVPARAM;
  const unsigned long long each = a.frames + (unsigned)a.f.taps + a.lookahead;
  const unsigned long long sums = rsmp::limit_release_blocks(a.frames + (a.lookahead - 1), unsigned(block)) + 1;
  a.work_stride = each + 2 * sums;
  r.work = work;
  r.tracks = a.tracks;
  r.frames = a.frames;
  r.stream_stride = 2 * a.work_stride;
  r.m_off = a.work_stride;
  r.c_off = each;
  r.b_off = a.work_stride + each;
  r.sum_stride = sums;
  r.lookahead = a.lookahead;
  r.block = unsigned(block);
  r.a = release;
  r.b = 1.0 - release;
  r.nstreams = a.nstreams;
  return RR_OK;
}

} // namespace

// RRX_limit_device with an exponential release between the window minimum and the box (limit_release.hip).  The limiter's own
// *_args function wants RRX_limit_work_doubles of work, which the release's buffer always holds: it is told there is enough.
int RRX_limit_release_device(int device, void *hip_stream, int src_format, const void *d_src, size_t src_stride, int dst_format, void *d_dst,
                             size_t dst_stride, int nstreams, size_t frames, int nch, const double *d_gain, double ceiling, const double *coefs,
                             int phases, int taps, size_t lookahead, size_t hold, double release, size_t block, double *d_reduction,
                             unsigned long long *d_limited, double *d_work, size_t work_doubles)
{
  rsmp::LimitArgs a;
  rsmp::LimitReleaseArgs r;
  int rc = limit_args(src_format, d_src, src_stride, dst_format, d_dst, dst_stride, nstreams, frames, nch, d_gain, ceiling, coefs, phases, taps,
                      lookahead, hold, d_reduction, d_limited, d_work, ~size_t(0), a);
  if (rc == RR_OK) rc = limit_release_args(release, block, d_work, work_doubles, a, r);
  if (rc != RR_OK) return rc;
  return on_device(device, !frames, [&] { return rsmp::launch_limit_release(static_cast<hipStream_t>(hip_stream), a, r); });
}

int RRX_debug_limit_release_host(int src_format, const void *src, size_t src_stride, int dst_format, void *dst, size_t dst_stride, int nstreams,
                                 size_t frames, int nch, const double *gain, double ceiling, const double *coefs, int phases, int taps,
                                 size_t lookahead, size_t hold, double release, size_t block, double *reduction, unsigned long long *limited,
                                 double *work, size_t work_doubles)
{
  rsmp::LimitArgs a;
  rsmp::LimitReleaseArgs r;
  return on_host(
      [&] {
        const int rc = limit_args(src_format, src, src_stride, dst_format, dst, dst_stride, nstreams, frames, nch, gain, ceiling, coefs, phases,
                                  taps, lookahead, hold, reduction, limited, work, ~size_t(0), a);
        return rc != RR_OK ? rc : limit_release_args(release, block, work, work_doubles, a, r);
      },
      !frames, [&] { rsmp::limit_release_host(a, r); });
}

// RRX_limit_release_device per track of a ragged batch (limit_release.hip).
int RRX_tracks_limit_release_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch, int src_format,
                                    const void *d_rows, int dst_format, void *d_dst_rows, size_t row_frames, const double *d_gain, double ceiling,
                                    const double *coefs, int phases, int taps, size_t lookahead, size_t hold, double release, size_t block,
                                    double *d_reduction, unsigned long long *d_limited, double *d_work, size_t work_doubles)
{
  rsmp::LimitArgs a;
  rsmp::LimitReleaseArgs r;
  int rc = tracks_limit_args(d_tracks, ntracks, nch, src_format, d_rows, dst_format, d_dst_rows, row_frames, d_gain, ceiling, coefs, phases, taps,
                             lookahead, hold, d_reduction, d_limited, d_work, ~size_t(0), a);
  if (rc == RR_OK) rc = limit_release_args(release, block, d_work, work_doubles, a, r);
  if (rc != RR_OK) return rc;
  return on_device(device, !row_frames, [&] { return rsmp::launch_limit_release(static_cast<hipStream_t>(hip_stream), a, r); });
}

namespace {

// the two biquads of the loudness calls and M = A^hop: RR_INVPARAM for a NULL pointer, a non-finite coefficient or hop == 0
int loudness_filter(const double *coefs, size_t hop, rsmp::LoudnessArgs &a)
{
  if (!coefs || !hop) return RR_INVPARAM;
  for (int k = 0; k < 10; ++k) {
    a.c[k] = coefs[k];
    if (!std::isfinite(a.c[k])) return RR_INVPARAM;
  }
  rsmp::loudness_power(a.c, hop, a.m);
  return RR_OK;
}

// RRX_loudness_device / RRX_debug_loudness_host: everything that can be refused from the arguments alone
int loudness_args(int src_format, const void *src, size_t src_stride, int nstreams, size_t frames, int nch, const double *gain,
                  unsigned long long first_frame, const double *coefs, size_t hop, const double *state_in, double *state_out, double *energy,
                  size_t energy_stride, double *work, size_t work_doubles, rsmp::LoudnessArgs &a)
{
  if (!energy) return RR_INVPARAM;
  int rc = loudness_filter(coefs, hop, a);
  if (rc != RR_OK) return rc;
  rsmp::FinishArgs f; // the sizes, strides and overflow rules are RRX_finish_device's, measuring only
  rc = finish_args(src_format, src, src_stride, 0, nullptr, 0, nstreams, frames, nch, gain, 0, 0, first_frame, energy, nullptr, f);
  if (rc != RR_OK) return rc;
  if (first_frame % hop) return RR_INVPARAM;
  if (!state_in && first_frame) return RR_INVPARAM; // a call that does not begin the stream needs the state in front of it
  if (!states_apart(state_in, state_out, uintptr_t(nstreams) * uintptr_t(nch) * 4)) return RR_INVPARAM;
  const unsigned long long n = frames / hop, first_hop = first_frame / hop;
  if (first_hop + n > energy_stride) return RR_INVPARAM;                            // (first_frame + frames does not wrap: nor does this)
  if (energy_stride > most_frames(nch) / size_t(nstreams)) return RR_INVPARAM;
  const unsigned long long need = rsmp::loudness_work_doubles(nstreams, nch, frames, hop);   // (< 2^62: nstreams * frames * nch < 2^60)
  if (work_doubles < need || (need && !work)) return RR_INVPARAM;
  a.src = f.src;
  a.gain = gain;
  a.state_in = first_frame ? state_in : nullptr; // S_0 = +0.0, whatever the buffer holds
  a.state_out = state_out;
  a.energy = energy;
  a.work = work;
  a.tracks = nullptr;
  a.hops_out = nullptr;
  a.src_stride = f.src_stride;
  a.frames = frames;
  a.hop = hop;
  a.max_hops = n;
  a.first_hop = first_hop;
  a.energy_stride = energy_stride;
  a.nstreams = nstreams;
  a.nch = nch;
  a.src_double = f.src_double;
  return RR_OK;
}

// The hop energies of whole tracks, in the rows of a ragged batch or at rest in a packed source: the refusals the two share and
// rsmp::LoudnessArgs.  `src_stride` is 0 for rows and src_total for a packed source; the source's format is the caller's to check.
static int tracks_loudness_args(const RRX_track *tracks, int ntracks, int nch, const void *src, bool src_double, size_t src_stride, size_t frames,
                         const double *gain, const double *coefs, size_t hop, double *energy, size_t energy_stride, unsigned long long *hops,
                         double *work, size_t work_doubles, rsmp::LoudnessArgs &a)
{
  if (!tracks || !src || ntracks < 1 || nch < 1 || !energy || !hops) return RR_INVPARAM;
  const int rc = loudness_filter(coefs, hop, a);
  if (rc != RR_OK) return rc;
  const size_t most = most_frames(nch) / size_t(ntracks);
  if (frames > most || energy_stride > most) return RR_INVPARAM;
  const unsigned long long need = rsmp::loudness_work_doubles(ntracks, nch, frames, hop);
  if (work_doubles < need || (need && !work)) return RR_INVPARAM;
  a.src = src;
  a.gain = gain;
  a.state_in = nullptr;
  a.state_out = nullptr;
  a.energy = energy;
  a.work = work;
  a.tracks = reinterpret_cast<const rsmp::Track *>(tracks);
  a.hops_out = hops;
  a.src_stride = src_stride;
  a.frames = frames;
  a.hop = hop;
  a.max_hops = frames / hop;
  a.first_hop = 0;
  a.energy_stride = energy_stride;
  a.nstreams = ntracks;
  a.nch = nch;
  a.src_double = src_double;
  return RR_OK;
}

// RRX_tracks_loudness_packed_device / RRX_debug_tracks_loudness_packed_host: everything that can be refused from the arguments
// alone; `kind` is the source's rsmp::TracksSrc
int loudness_packed_args(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *packed, size_t src_total, size_t max_frames,
                         const double *gain, const double *coefs, size_t hop, double *energy, size_t energy_stride, unsigned long long *hops,
                         double *work, size_t work_doubles, rsmp::LoudnessArgs &a, int &kind)
{
  kind = tracks_src_kind(src_format);
  if (kind < 0) return RR_INVPARAM;
  const int rc = tracks_loudness_args(tracks, ntracks, nch, packed, false, src_total, max_frames, gain, coefs, hop, energy, energy_stride, hops,
                                      work, work_doubles, a);
  if (rc != RR_OK) return rc;
  return src_total > most_frames(nch) ? RR_INVPARAM : RR_OK;
}

// RRX_loudness_gate_device / RRX_debug_loudness_gate_host
int loudness_gate_args(const double *energy, size_t energy_stride, int nstreams, int nch, size_t nhops, const unsigned long long *hops,
                       const double *weights, size_t hop, double abs_threshold, double rel_factor, double *result, rsmp::LoudnessGateArgs &a)
{
  if (!energy || !result || nstreams < 1 || nch < 1 || !hop || nhops > energy_stride) return RR_INVPARAM;
  if (std::isnan(abs_threshold) || std::isnan(rel_factor)) return RR_INVPARAM;
  if (energy_stride > most_frames(nch) / size_t(nstreams)) return RR_INVPARAM;
  a.energy = energy;
  a.hops = hops;
  a.weights = weights;
  a.result = result;
  a.energy_stride = energy_stride;
  a.nhops = nhops;
  a.nstreams = nstreams;
  a.nch = nch;
  a.inv = 1.0 / (4.0 * (double)hop);
  a.abs_threshold = abs_threshold;
  a.rel_factor = rel_factor;
  return RR_OK;
}

} // namespace

size_t RRX_loudness_work_doubles(int nstreams, int nch, size_t frames, size_t hop)
{
  if (nstreams < 1 || nch < 1 || !hop) return 0;
  return size_t(rsmp::loudness_work_doubles(nstreams, nch, frames, hop));
}

// K-weighted hop energies of device-resident frames (loudness.hip).
int RRX_loudness_device(int device, void *hip_stream, int src_format, const void *d_src, size_t src_stride, int nstreams, size_t frames,
                        int nch, const double *d_gain, unsigned long long first_frame, const double *coefs, size_t hop,
                        const double *d_state_in, double *d_state_out, double *d_energy, size_t energy_stride, double *d_work,
                        size_t work_doubles)
{
  rsmp::LoudnessArgs a;
  const int rc = loudness_args(src_format, d_src, src_stride, nstreams, frames, nch, d_gain, first_frame, coefs, hop, d_state_in, d_state_out,
                               d_energy, energy_stride, d_work, work_doubles, a);
  if (rc != RR_OK) return rc;
  return on_device(device, !frames, [&] { return rsmp::launch_loudness(static_cast<hipStream_t>(hip_stream), a); });
}

int RRX_debug_loudness_host(int src_format, const void *src, size_t src_stride, int nstreams, size_t frames, int nch, const double *gain,
                            unsigned long long first_frame, const double *coefs, size_t hop, const double *state_in, double *state_out,
                            double *energy, size_t energy_stride, double *work, size_t work_doubles)
{
  rsmp::LoudnessArgs a;
  return on_host(
      [&] {
        return loudness_args(src_format, src, src_stride, nstreams, frames, nch, gain, first_frame, coefs, hop, state_in, state_out, energy,
                             energy_stride, work, work_doubles, a);
      },
      !frames, [&] { rsmp::loudness_host(a); });
}

// RRX_loudness_device per track of a ragged batch (loudness.hip).
int RRX_tracks_loudness_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch, int src_format,
                               const void *d_rows, size_t row_frames, const double *d_gain, const double *coefs, size_t hop, double *d_energy,
                               size_t energy_stride, unsigned long long *d_hops, double *d_work, size_t work_doubles)
{
  rsmp::LoudnessArgs a;
  if (!float_format(src_format)) return RR_INVPARAM;
  const int rc = tracks_loudness_args(d_tracks, ntracks, nch, d_rows, src_format == RRX_FMT_DOUBLE, 0, row_frames, d_gain, coefs, hop, d_energy,
                                      energy_stride, d_hops, d_work, work_doubles, a);
  if (rc != RR_OK) return rc;
  return on_device(device, !row_frames, [&] { return rsmp::launch_loudness(static_cast<hipStream_t>(hip_stream), a); });
}

// K-weighted hop energies of tracks at rest in a packed source (loudness.hip).
int RRX_tracks_loudness_packed_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch, int src_format,
                                      const void *d_packed, size_t src_total, size_t max_frames, const double *d_gain, const double *coefs,
                                      size_t hop, double *d_energy, size_t energy_stride, unsigned long long *d_hops, double *d_work,
                                      size_t work_doubles)
{
  rsmp::LoudnessArgs a;
  int kind = 0;
  const int rc = loudness_packed_args(d_tracks, ntracks, nch, src_format, d_packed, src_total, max_frames, d_gain, coefs, hop, d_energy,
                                      energy_stride, d_hops, d_work, work_doubles, a, kind);
  if (rc != RR_OK) return rc;
  return on_device(device, !max_frames || !src_total,
                   [&] { return rsmp::launch_loudness_packed(static_cast<hipStream_t>(hip_stream), a, kind); });
}

int RRX_debug_tracks_loudness_packed_host(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *packed, size_t src_total,
                                          size_t max_frames, const double *gain, const double *coefs, size_t hop, double *energy,
                                          size_t energy_stride, unsigned long long *hops, double *work, size_t work_doubles)
{
  rsmp::LoudnessArgs a;
  int kind = 0;
  return on_host(
      [&] {
        return loudness_packed_args(tracks, ntracks, nch, src_format, packed, src_total, max_frames, gain, coefs, hop, energy, energy_stride,
                                    hops, work, work_doubles, a, kind);
      },
      !max_frames || !src_total, [&] { rsmp::loudness_packed_host(a, kind); });
}

// The two-stage gate over hop energies (loudness.hip).
int RRX_loudness_gate_device(int device, void *hip_stream, const double *d_energy, size_t energy_stride, int nstreams, int nch, size_t nhops,
                             const unsigned long long *d_hops, const double *d_weights, size_t hop, double abs_threshold, double rel_factor,
                             double *d_result)
{
  rsmp::LoudnessGateArgs a;
  const int rc = loudness_gate_args(d_energy, energy_stride, nstreams, nch, nhops, d_hops, d_weights, hop, abs_threshold, rel_factor, d_result, a);
  if (rc != RR_OK) return rc;
  return on_device(device, false, [&] { return rsmp::launch_loudness_gate(static_cast<hipStream_t>(hip_stream), a); });
}

int RRX_debug_loudness_gate_host(const double *energy, size_t energy_stride, int nstreams, int nch, size_t nhops, const unsigned long long *hops,
                                 const double *weights, size_t hop, double abs_threshold, double rel_factor, double *result)
{
  rsmp::LoudnessGateArgs a;
  return on_host(
      [&] { return loudness_gate_args(energy, energy_stride, nstreams, nch, nhops, hops, weights, hop, abs_threshold, rel_factor, result, a); },
      false, [&] { rsmp::loudness_gate_host(a); });
}

namespace {

// RRX_loudness_blocks_device / RRX_debug_loudness_blocks_host: the gate's refusals and those of the block geometry
int loudness_blocks_args(const double *energy, size_t energy_stride, int nstreams, int nch, size_t nhops, const unsigned long long *hops,
                         const double *weights, size_t hop, size_t block_hops, size_t step_hops, double *blocks, size_t blocks_stride,
                         unsigned long long *nblocks, double *max, rsmp::LoudnessBlocksArgs &a)
{
  if (!energy || nstreams < 1 || nch < 1 || !hop || nhops > energy_stride) return RR_INVPARAM;
  if (energy_stride > most_frames(nch) / size_t(nstreams)) return RR_INVPARAM;
  if (!block_hops || !step_hops || (!blocks && !nblocks && !max)) return RR_INVPARAM;
  if ((blocks && !blocks_stride) || blocks_stride > most_frames(1) / size_t(nstreams)) return RR_INVPARAM; // (a block is one double)
  a.energy = energy;
  a.hops = hops;
  a.weights = weights;
  a.blocks = blocks;
  a.nblocks = nblocks;
  a.max = max;
  a.energy_stride = energy_stride;
  a.nhops = nhops;
  a.blocks_stride = blocks_stride;
  a.block_hops = block_hops;
  a.step_hops = step_hops;
  a.nstreams = nstreams;
  a.nch = nch;
  a.inv = 1.0 / ((double)block_hops * (double)hop);
  return RR_OK;
}

// the gate and the range over groups, and their twins; range: the percentiles are checked too, and abs_threshold < 0 is refused
int loudness_groups_args(const double *blocks, size_t blocks_stride, int nstreams, const unsigned long long *nblocks, const int *group, int ngroups,
                         double abs_threshold, double rel_factor, bool range, int pct_low, int pct_high, double *result, double *work,
                         size_t work_doubles, rsmp::LoudnessGroupsArgs &a)
{
  if (!blocks || !nblocks || !group || !result || !work || nstreams < 1 || ngroups < 1) return RR_INVPARAM;
  if (std::isnan(abs_threshold) || std::isnan(rel_factor)) return RR_INVPARAM;
  if (blocks_stride > most_frames(1) / size_t(nstreams)) return RR_INVPARAM; // (a block is one double)
  if (work_doubles < rsmp::loudness_groups_work_doubles(nstreams, ngroups)) return RR_INVPARAM;
  if (range && (abs_threshold < 0 || pct_low < 0 || pct_low > 100 || pct_high < 0 || pct_high > 100)) return RR_INVPARAM;
  a.blocks = blocks;
  a.nblocks = nblocks;
  a.group = group;
  a.result = result;
  a.work = work;
  a.blocks_stride = blocks_stride;
  a.nstreams = nstreams;
  a.ngroups = ngroups;
  a.pct_low = pct_low;
  a.pct_high = pct_high;
  a.abs_threshold = abs_threshold;
  a.rel_factor = rel_factor;
  return RR_OK;
}

} // namespace

// Sliding block powers and their maximum (loudness_stats.hip).
int RRX_loudness_blocks_device(int device, void *hip_stream, const double *d_energy, size_t energy_stride, int nstreams, int nch, size_t nhops,
                               const unsigned long long *d_hops, const double *d_weights, size_t hop, size_t block_hops, size_t step_hops,
                               double *d_blocks, size_t blocks_stride, unsigned long long *d_nblocks, double *d_max)
{
  rsmp::LoudnessBlocksArgs a;
  const int rc = loudness_blocks_args(d_energy, energy_stride, nstreams, nch, nhops, d_hops, d_weights, hop, block_hops, step_hops, d_blocks,
                                      blocks_stride, d_nblocks, d_max, a);
  if (rc != RR_OK) return rc;
  return on_device(device, false, [&] { return rsmp::launch_loudness_blocks(static_cast<hipStream_t>(hip_stream), a); });
}

int RRX_debug_loudness_blocks_host(const double *energy, size_t energy_stride, int nstreams, int nch, size_t nhops, const unsigned long long *hops,
                                   const double *weights, size_t hop, size_t block_hops, size_t step_hops, double *blocks, size_t blocks_stride,
                                   unsigned long long *nblocks, double *max)
{
  rsmp::LoudnessBlocksArgs a;
  return on_host(
      [&] {
        return loudness_blocks_args(energy, energy_stride, nstreams, nch, nhops, hops, weights, hop, block_hops, step_hops, blocks, blocks_stride,
                                    nblocks, max, a);
      },
      false, [&] { rsmp::loudness_blocks_host(a); });
}

size_t RRX_loudness_groups_work_doubles(int nstreams, int ngroups)
{
  if (nstreams < 1 || ngroups < 1) return 0;
  return size_t(rsmp::loudness_groups_work_doubles(nstreams, ngroups));
}

// The BS.1770 gate over the pooled blocks of groups of streams (loudness_stats.hip).
int RRX_loudness_gate_groups_device(int device, void *hip_stream, const double *d_blocks, size_t blocks_stride, int nstreams,
                                    const unsigned long long *d_nblocks, const int *d_group, int ngroups, double abs_threshold, double rel_factor,
                                    double *d_result, double *d_work, size_t work_doubles)
{
  rsmp::LoudnessGroupsArgs a;
  const int rc = loudness_groups_args(d_blocks, blocks_stride, nstreams, d_nblocks, d_group, ngroups, abs_threshold, rel_factor, false, 0, 0,
                                      d_result, d_work, work_doubles, a);
  if (rc != RR_OK) return rc;
  return on_device(device, false, [&] { return rsmp::launch_loudness_gate_groups(static_cast<hipStream_t>(hip_stream), a); });
}

int RRX_debug_loudness_gate_groups_host(const double *blocks, size_t blocks_stride, int nstreams, const unsigned long long *nblocks, const int *group,
                                        int ngroups, double abs_threshold, double rel_factor, double *result, double *work, size_t work_doubles)
{
  rsmp::LoudnessGroupsArgs a;
  return on_host(
      [&] {
        return loudness_groups_args(blocks, blocks_stride, nstreams, nblocks, group, ngroups, abs_threshold, rel_factor, false, 0, 0, result, work,
                                    work_doubles, a);
      },
      false, [&] { rsmp::loudness_gate_groups_host(a); });
}

// Gated percentiles per group by exact selection (loudness_stats.hip).
int RRX_loudness_range_groups_device(int device, void *hip_stream, const double *d_blocks, size_t blocks_stride, int nstreams,
                                     const unsigned long long *d_nblocks, const int *d_group, int ngroups, double abs_threshold, double rel_factor,
                                     int pct_low, int pct_high, double *d_result, double *d_work, size_t work_doubles)
{
  rsmp::LoudnessGroupsArgs a;
  const int rc = loudness_groups_args(d_blocks, blocks_stride, nstreams, d_nblocks, d_group, ngroups, abs_threshold, rel_factor, true, pct_low,
                                      pct_high, d_result, d_work, work_doubles, a);
  if (rc != RR_OK) return rc;
  return on_device(device, false, [&] { return rsmp::launch_loudness_range_groups(static_cast<hipStream_t>(hip_stream), a); });
}

int RRX_debug_loudness_range_groups_host(const double *blocks, size_t blocks_stride, int nstreams, const unsigned long long *nblocks,
                                         const int *group, int ngroups, double abs_threshold, double rel_factor, int pct_low, int pct_high,
                                         double *result, double *work, size_t work_doubles)
{
  rsmp::LoudnessGroupsArgs a;
  return on_host(
      [&] {
        return loudness_groups_args(blocks, blocks_stride, nstreams, nblocks, group, ngroups, abs_threshold, rel_factor, true, pct_low, pct_high,
                                    result, work, work_doubles, a);
      },
      false, [&] { rsmp::loudness_range_groups_host(a); });
}

namespace {

// RRX_tracks_finish_shaped_device and the window form of it: what RRX_tracks_finish_device refuses and fills, and what the shaped
// dither adds -- a destination format even when nothing is written (the statistics are those of the write), and the filter
static int tracks_shaped_args(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *rows, size_t row_frames, int dst_format,
                       void *dst, size_t dst_total, const double *gain, int dither, unsigned long long seed, const double *coefs, int order,
                       size_t segment, double *peak, unsigned long long *clipped, rsmp::TracksShapedArgs &a)
{
  if (!pcm_format(dst_format)) return RR_INVPARAM; // measure only included
  if (shaped_filter(coefs, order, a.coefs) != RR_OK) return RR_INVPARAM;
  const int rc = tracks_finish_args(tracks, ntracks, nch, src_format, rows, row_frames, dst_format, dst, dst_total, gain, dither, seed, peak,
                                    clipped, a.t);
  if (rc != RR_OK) return rc;
  a.t.bits = pcm_bits(dst_format);
  a.segment = segment;
  a.order = order;
  return RR_OK;
}

} // namespace

// The shaped output stage of a ragged batch (finish_shaped.hip).
int RRX_tracks_finish_shaped_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch, int src_format,
                                    const void *d_rows, size_t row_frames, int dst_format, void *d_dst, size_t dst_total, const double *d_gain,
                                    int dither, unsigned long long seed, const double *coefs, int order, size_t segment, double *d_peak,
                                    unsigned long long *d_clipped)
{
  rsmp::TracksShapedArgs a;
  const int rc = tracks_shaped_args(d_tracks, ntracks, nch, src_format, d_rows, row_frames, dst_format, d_dst, dst_total, d_gain, dither, seed,
                                    coefs, order, segment, d_peak, d_clipped, a);
  if (rc != RR_OK) return rc;
  return on_device(device, !row_frames, [&] { return rsmp::launch_tracks_finish_shaped(static_cast<hipStream_t>(hip_stream), a); });
}

namespace {

// the window of a window call: RR_INVPARAM unless it lies inside the rows, fits its pitch and the window buffer is one a device can hold
int tracks_window_args(int ntracks, int nch, size_t row_frames, size_t win_first, size_t win_frames, size_t win_stride, rsmp::TracksWindow &w)
{
  if (win_first + win_frames < win_first || win_first + win_frames > row_frames || win_stride < win_frames) return RR_INVPARAM;
  if (win_stride > most_frames(nch) / size_t(ntracks)) return RR_INVPARAM;
  w.first = win_first;
  w.frames = win_frames;
  w.stride = win_stride;
  return RR_OK;
}

// the two state rules of the window calls that carry a state per track: no state only for a window at frame 0, and two buffers
// of `doubles` doubles that do not overlap
int measure_window_state(const double *state_in, double *state_out, size_t win_first, uintptr_t doubles)
{
  if (!state_in && win_first) return RR_INVPARAM; // only a window at frame 0 finds every track at its first frame or not begun
  return states_apart(state_in, state_out, doubles) ? RR_OK : RR_INVPARAM;
}

} // namespace

// RRX_tracks_stage_device_samples on a window of the rows (tracks.hip).
int RRX_tracks_stage_window_device(int device, void *hip_stream, size_t in_rate, size_t out_rate, const RRX_track *d_tracks, int ntracks, int nch,
                                   int src_format, const void *d_packed, size_t src_total, size_t row_frames, size_t win_first, size_t win_frames,
                                   fb_sample_t *d_win, size_t win_stride)
{
  rsmp::TracksStageArgs a;
  rsmp::TracksWindow w;
  int rc = tracks_stage_args(in_rate, out_rate, d_tracks, ntracks, nch, src_format, d_packed, src_total, d_win, row_frames, a);
  if (rc == RR_OK) rc = tracks_window_args(ntracks, nch, row_frames, win_first, win_frames, win_stride, w);
  if (rc != RR_OK) return rc;
  return on_device(device, !win_frames, [&] { return rsmp::launch_tracks_stage_window(static_cast<hipStream_t>(hip_stream), a, w); });
}

namespace {

// The three album calls (include/ratelib_amd_album.h): what the un-linked stage calls refuse, and the window.  Whole rows are the
// window [0, row_frames) of rows that are their own buffer.
int tracks_album_args(size_t in_rate, size_t out_rate, const RRX_track *tracks, const RRX_track_link *links, int ntracks, int nch, int src_format,
                      const void *packed, size_t src_total, size_t row_frames, size_t win_first, size_t win_frames, fb_sample_t *win,
                      size_t win_stride, rsmp::TracksAlbumArgs &a, rsmp::TracksWindow &w)
{
  static_assert(sizeof(RRX_track_link) == sizeof(rsmp::TrackLink) && sizeof(RRX_track_link) == 2 * sizeof(unsigned long long),
                "RRX_track_link mirrors rsmp::TrackLink");
  static_assert(RRX_LINK_NONE == rsmp::kLinkNone, "RRX_LINK_NONE mirrors rsmp::kLinkNone");
  int rc = tracks_stage_args(in_rate, out_rate, tracks, ntracks, nch, src_format, packed, src_total, win, row_frames, a.s);
  if (rc == RR_OK) rc = tracks_window_args(ntracks, nch, row_frames, win_first, win_frames, win_stride, w);
  a.links = reinterpret_cast<const rsmp::TrackLink *>(links);
  return rc;
}

} // namespace

// The stage pass of a ragged batch with links (tracks_album.hip); without them, RRX_tracks_stage_device_samples.
int RRX_tracks_stage_album_device(int device, void *hip_stream, size_t in_rate, size_t out_rate, const RRX_track *d_tracks,
                                  const RRX_track_link *d_links, int ntracks, int nch, int src_format, const void *d_packed, size_t src_total,
                                  fb_sample_t *d_rows, size_t row_frames)
{
  if (!d_links)
    return RRX_tracks_stage_device_samples(device, hip_stream, in_rate, out_rate, d_tracks, ntracks, nch, src_format, d_packed, src_total, d_rows,
                                           row_frames);
  rsmp::TracksAlbumArgs a;
  rsmp::TracksWindow w;
  const int rc = tracks_album_args(in_rate, out_rate, d_tracks, d_links, ntracks, nch, src_format, d_packed, src_total, row_frames, 0, row_frames,
                                   d_rows, row_frames, a, w);
  if (rc != RR_OK) return rc;
  return on_device(device, false, [&] { return rsmp::launch_tracks_stage_album(static_cast<hipStream_t>(hip_stream), a, w); });
}

int RRX_tracks_stage_album_window_device(int device, void *hip_stream, size_t in_rate, size_t out_rate, const RRX_track *d_tracks,
                                         const RRX_track_link *d_links, int ntracks, int nch, int src_format, const void *d_packed,
                                         size_t src_total, size_t row_frames, size_t win_first, size_t win_frames, fb_sample_t *d_win,
                                         size_t win_stride)
{
  if (!d_links)
    return RRX_tracks_stage_window_device(device, hip_stream, in_rate, out_rate, d_tracks, ntracks, nch, src_format, d_packed, src_total,
                                          row_frames, win_first, win_frames, d_win, win_stride);
  rsmp::TracksAlbumArgs a;
  rsmp::TracksWindow w;
  const int rc = tracks_album_args(in_rate, out_rate, d_tracks, d_links, ntracks, nch, src_format, d_packed, src_total, row_frames, win_first,
                                   win_frames, d_win, win_stride, a, w);
  if (rc != RR_OK) return rc;
  return on_device(device, !win_frames, [&] { return rsmp::launch_tracks_stage_album(static_cast<hipStream_t>(hip_stream), a, w); });
}

int RRX_debug_tracks_stage_album_host(size_t in_rate, size_t out_rate, const RRX_track *tracks, const RRX_track_link *links, int ntracks, int nch,
                                      int src_format, const void *packed, size_t src_total, size_t row_frames, size_t win_first,
                                      size_t win_frames, fb_sample_t *win, size_t win_stride)
{
  rsmp::TracksAlbumArgs a;
  rsmp::TracksWindow w;
  std::vector<rsmp::TrackLink> none; // links == NULL: every edge is extrapolated
  return on_host(
      [&] {
        const int rc = tracks_album_args(in_rate, out_rate, tracks, links, ntracks, nch, src_format, packed, src_total, row_frames, win_first,
                                         win_frames, win, win_stride, a, w);
        if (rc == RR_OK && !links) {
          none.assign(size_t(ntracks), rsmp::TrackLink{rsmp::kLinkNone, rsmp::kLinkNone});
          a.links = none.data();
        }
        return rc;
      },
      !win_frames, [&] { rsmp::tracks_stage_album_host(a, w); });
}

// RRX_tracks_finish_device on a window of the output rows (tracks.hip).
int RRX_tracks_finish_window_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch, int src_format,
                                    const void *d_win, size_t win_stride, size_t row_frames, size_t win_first, size_t win_frames, int dst_format,
                                    void *d_dst, size_t dst_total, const double *d_gain, int dither, unsigned long long seed, double *d_peak,
                                    unsigned long long *d_clipped)
{
  rsmp::TracksFinishArgs a;
  rsmp::TracksWindow w;
  int rc = tracks_finish_args(d_tracks, ntracks, nch, src_format, d_win, row_frames, dst_format, d_dst, dst_total, d_gain, dither, seed, d_peak,
                              d_clipped, a);
  if (rc == RR_OK) rc = tracks_window_args(ntracks, nch, row_frames, win_first, win_frames, win_stride, w);
  if (rc != RR_OK) return rc;
  return on_device(device, !row_frames || !win_frames,
                   [&] { return rsmp::launch_tracks_finish_window(static_cast<hipStream_t>(hip_stream), a, w); });
}

namespace {

// RRX_tracks_finish_shaped_window_device / RRX_debug_tracks_finish_shaped_window_host: everything that can be refused from the
// arguments alone -- what RRX_tracks_finish_shaped_device refuses, the window and the state rules
int tracks_shaped_window_args(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *win, size_t win_stride, size_t row_frames,
                              size_t win_first, size_t win_frames, int dst_format, void *dst, size_t dst_total, const double *gain, int dither,
                              unsigned long long seed, const double *coefs, int order, size_t segment, const double *state_in, double *state_out,
                              double *peak, unsigned long long *clipped, rsmp::TracksShapedWindowArgs &a)
{
  const int rc = tracks_shaped_args(tracks, ntracks, nch, src_format, win, row_frames, dst_format, dst, dst_total, gain, dither, seed, coefs, order,
                                    segment, peak, clipped, a.s);
  if (rc != RR_OK) return rc;
  if (tracks_window_args(ntracks, nch, row_frames, win_first, win_frames, win_stride, a.w) != RR_OK) return RR_INVPARAM;
  if (measure_window_state(state_in, state_out, win_first, uintptr_t(ntracks) * uintptr_t(nch) * rsmp::kShapeMaxOrder) != RR_OK) return RR_INVPARAM;
  a.state_in = state_in;
  a.state_out = state_out;
  return RR_OK;
}

} // namespace

// RRX_tracks_finish_shaped_device on a window of the output rows, the error history carried per track (finish_shaped.hip).
int RRX_tracks_finish_shaped_window_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch, int src_format,
                                           const void *d_win, size_t win_stride, size_t row_frames, size_t win_first, size_t win_frames,
                                           int dst_format, void *d_dst, size_t dst_total, const double *d_gain, int dither, unsigned long long seed,
                                           const double *coefs, int order, size_t segment, const double *d_state_in, double *d_state_out,
                                           double *d_peak, unsigned long long *d_clipped)
{
  rsmp::TracksShapedWindowArgs a;
  const int rc = tracks_shaped_window_args(d_tracks, ntracks, nch, src_format, d_win, win_stride, row_frames, win_first, win_frames, dst_format,
                                           d_dst, dst_total, d_gain, dither, seed, coefs, order, segment, d_state_in, d_state_out, d_peak,
                                           d_clipped, a);
  if (rc != RR_OK) return rc;
  return on_device(device, !row_frames || !win_frames,
                   [&] { return rsmp::launch_tracks_finish_shaped_window(static_cast<hipStream_t>(hip_stream), a); });
}

int RRX_debug_tracks_finish_shaped_window_host(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *win, size_t win_stride,
                                               size_t row_frames, size_t win_first, size_t win_frames, int dst_format, void *dst,
                                               size_t dst_total, const double *gain, int dither, unsigned long long seed, const double *coefs,
                                               int order, size_t segment, const double *state_in, double *state_out, double *peak,
                                               unsigned long long *clipped)
{
  rsmp::TracksShapedWindowArgs a;
  return on_host(
      [&] {
        return tracks_shaped_window_args(tracks, ntracks, nch, src_format, win, win_stride, row_frames, win_first, win_frames, dst_format, dst,
                                         dst_total, gain, dither, seed, coefs, order, segment, state_in, state_out, peak, clipped, a);
      },
      !row_frames || !win_frames, [&] { rsmp::tracks_finish_shaped_window_host(a); });
}

// Test hook: what the window kernels take from one table entry -- tracks_stage_cut and tracks_finish_cut (tracks.hpp), the functions
// the kernels call, on a host entry.  stage[10]: bk, cp, fw, z (two values each), src_frame, readable; finish[4]: w0, w1, index, dst_frame.
int RRX_debug_tracks_window_cut(const RRX_track *entry, size_t row_frames, size_t src_total, size_t dst_total, int write, size_t win_first,
                                size_t win_frames, unsigned long long *stage, unsigned long long *finish)
{
  if (!rsmp::knobs().test_hooks) return -1;
  if (!entry || !stage || !finish || win_first + win_frames < win_first || win_first + win_frames > row_frames) return RR_INVPARAM;
  rsmp::Track tr;
  std::memcpy(&tr, entry, sizeof(tr));
  const rsmp::TracksWindow w = {win_first, win_frames, win_frames};
  const rsmp::TracksStageCut c = rsmp::tracks_stage_cut(tr, row_frames, src_total, w);
  const unsigned long long s[10] = {c.bk[0], c.bk[1], c.cp[0], c.cp[1], c.fw[0], c.fw[1], c.z[0], c.z[1], c.src_frame, c.readable};
  std::memcpy(stage, s, sizeof(s));
  const rsmp::TracksFinishCut f = rsmp::tracks_finish_cut(tr, row_frames, dst_total, write != 0, w);
  const unsigned long long o[4] = {f.w0, f.w1, f.index, f.dst_frame};
  std::memcpy(finish, o, sizeof(o));
  return RR_OK;
}

namespace {

// RRX_tracks_true_peak_window_device / RRX_debug_tracks_true_peak_window_host: everything that can be refused from the arguments
// alone -- what RRX_tracks_true_peak_device refuses, the three window refusals and the two state rules
int tracks_true_peak_window_args(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *win, size_t win_stride,
                                 size_t row_frames, size_t win_first, size_t win_frames, const double *gain, const double *coefs, int phases,
                                 int taps, const double *state_in, double *state_out, double *true_peak, double *peak,
                                 rsmp::TruePeakWindowArgs &a)
{
  if (!tracks || !win || ntracks < 1 || nch < 1) return RR_INVPARAM;
  if (!float_format(src_format)) return RR_INVPARAM;
  if (!true_peak && !peak) return RR_INVPARAM;
  if (true_peak_filter(coefs, phases, taps, a.f) != RR_OK) return RR_INVPARAM;
  if (row_frames > most_frames(nch) / size_t(ntracks)) return RR_INVPARAM;
  if (tracks_window_args(ntracks, nch, row_frames, win_first, win_frames, win_stride, a.w) != RR_OK) return RR_INVPARAM;
  if (measure_window_state(state_in, state_out, win_first, uintptr_t(ntracks) * uintptr_t(nch) * rsmp::kTpMaxTaps) != RR_OK) return RR_INVPARAM;
  a.src = win;
  a.gain = gain;
  a.state_in = state_in;
  a.state_out = state_out;
  a.true_peak = true_peak;
  a.peak = peak;
  a.tracks = reinterpret_cast<const rsmp::Track *>(tracks);
  a.row_frames = row_frames;
  a.ntracks = ntracks;
  a.nch = nch;
  a.src_double = src_format == RRX_FMT_DOUBLE;
  return RR_OK;
}

// RRX_tracks_loudness_window_device / RRX_debug_tracks_loudness_window_host, likewise
int tracks_loudness_window_args(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *win, size_t win_stride,
                                size_t row_frames, size_t win_first, size_t win_frames, const double *gain, const double *coefs, size_t hop,
                                const double *state_in, double *state_out, double *energy, size_t energy_stride, unsigned long long *hops,
                                double *work, size_t work_doubles, rsmp::LoudnessWindowArgs &a)
{
  static_assert(RRX_LOUDNESS_WIN_STATE == rsmp::kLoudnessWinState, "the header's constant is the kernels'");
  if (!tracks || !win || ntracks < 1 || nch < 1 || !energy || !hops) return RR_INVPARAM;
  if (!float_format(src_format)) return RR_INVPARAM;
  rsmp::LoudnessArgs f;
  if (loudness_filter(coefs, hop, f) != RR_OK) return RR_INVPARAM;
  const size_t most = most_frames(nch) / size_t(ntracks);
  if (row_frames > most || energy_stride > most) return RR_INVPARAM;
  if (tracks_window_args(ntracks, nch, row_frames, win_first, win_frames, win_stride, a.w) != RR_OK) return RR_INVPARAM;
  const unsigned long long need = rsmp::loudness_window_work_doubles(ntracks, nch, win_frames, hop); // (< 2^63: ntracks * win_frames * nch < 2^60)
  if (work_doubles < need || (need && !work)) return RR_INVPARAM;
  if (measure_window_state(state_in, state_out, win_first, uintptr_t(ntracks) * uintptr_t(nch) * rsmp::kLoudnessWinState) != RR_OK) return RR_INVPARAM;
  a.src = win;
  a.gain = gain;
  a.state_in = state_in;
  a.state_out = state_out;
  a.energy = energy;
  a.work = work;
  a.tracks = reinterpret_cast<const rsmp::Track *>(tracks);
  a.hops_out = hops;
  a.row_frames = row_frames;
  a.hop = hop;
  a.pieces = win_frames / hop + 2;
  a.energy_stride = energy_stride;
  a.ntracks = ntracks;
  a.nch = nch;
  a.src_double = src_format == RRX_FMT_DOUBLE;
  std::memcpy(a.c, f.c, sizeof(a.c));
  std::memcpy(a.m, f.m, sizeof(a.m));
  return RR_OK;
}

} // namespace

// RRX_tracks_true_peak_device on a window of the output rows, the filter's history carried per track (measure_window.hip).
int RRX_tracks_true_peak_window_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch, int src_format,
                                       const void *d_win, size_t win_stride, size_t row_frames, size_t win_first, size_t win_frames,
                                       const double *d_gain, const double *coefs, int phases, int taps, const double *d_state_in,
                                       double *d_state_out, double *d_true_peak, double *d_peak)
{
  rsmp::TruePeakWindowArgs a;
  const int rc = tracks_true_peak_window_args(d_tracks, ntracks, nch, src_format, d_win, win_stride, row_frames, win_first, win_frames, d_gain,
                                              coefs, phases, taps, d_state_in, d_state_out, d_true_peak, d_peak, a);
  if (rc != RR_OK) return rc;
  return on_device(device, !row_frames || !win_frames, [&] { return rsmp::launch_true_peak_window(static_cast<hipStream_t>(hip_stream), a); });
}

int RRX_debug_tracks_true_peak_window_host(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *win, size_t win_stride,
                                           size_t row_frames, size_t win_first, size_t win_frames, const double *gain, const double *coefs,
                                           int phases, int taps, const double *state_in, double *state_out, double *true_peak, double *peak)
{
  rsmp::TruePeakWindowArgs a;
  return on_host(
      [&] {
        return tracks_true_peak_window_args(tracks, ntracks, nch, src_format, win, win_stride, row_frames, win_first, win_frames, gain, coefs,
                                            phases, taps, state_in, state_out, true_peak, peak, a);
      },
      !row_frames || !win_frames, [&] { rsmp::true_peak_window_host(a); });
}

size_t RRX_tracks_loudness_window_work_doubles(int ntracks, int nch, size_t win_frames, size_t hop)
{
  if (ntracks < 1 || nch < 1 || !hop) return 0;
  return size_t(rsmp::loudness_window_work_doubles(ntracks, nch, win_frames, hop));
}

// RRX_tracks_loudness_device on a window of the output rows, the hop in progress carried per track (measure_window.hip).
int RRX_tracks_loudness_window_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch, int src_format,
                                      const void *d_win, size_t win_stride, size_t row_frames, size_t win_first, size_t win_frames,
                                      const double *d_gain, const double *coefs, size_t hop, const double *d_state_in, double *d_state_out,
                                      double *d_energy, size_t energy_stride, unsigned long long *d_hops, double *d_work, size_t work_doubles)
{
  rsmp::LoudnessWindowArgs a;
  const int rc = tracks_loudness_window_args(d_tracks, ntracks, nch, src_format, d_win, win_stride, row_frames, win_first, win_frames, d_gain,
                                             coefs, hop, d_state_in, d_state_out, d_energy, energy_stride, d_hops, d_work, work_doubles, a);
  if (rc != RR_OK) return rc;
  return on_device(device, !row_frames || !win_frames, [&] { return rsmp::launch_loudness_window(static_cast<hipStream_t>(hip_stream), a); });
}

int RRX_debug_tracks_loudness_window_host(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *win, size_t win_stride,
                                          size_t row_frames, size_t win_first, size_t win_frames, const double *gain, const double *coefs,
                                          size_t hop, const double *state_in, double *state_out, double *energy, size_t energy_stride,
                                          unsigned long long *hops, double *work, size_t work_doubles)
{
  rsmp::LoudnessWindowArgs a;
  return on_host(
      [&] {
        return tracks_loudness_window_args(tracks, ntracks, nch, src_format, win, win_stride, row_frames, win_first, win_frames, gain, coefs,
                                           hop, state_in, state_out, energy, energy_stride, hops, work, work_doubles, a);
      },
      !row_frames || !win_frames, [&] { rsmp::loudness_window_host(a); });
}

// how far a frame's gain reaches into the samples around it (limit.hpp): host only
int RRX_limit_window_reach(int taps, size_t lookahead, size_t hold, size_t *back, size_t *ahead)
{
  if (!back || !ahead || taps < 1 || taps > RRX_TP_MAX_TAPS) return RR_INVPARAM;
  if (lookahead < 1 || lookahead > RRX_LIMIT_MAX_LOOKAHEAD || hold > RRX_LIMIT_MAX_HOLD) return RR_INVPARAM;
  *back = size_t(rsmp::limit_reach_back(taps, unsigned(lookahead), unsigned(hold)));
  *ahead = size_t(rsmp::limit_reach_ahead(taps, unsigned(lookahead)));
  return RR_OK;
}

// r and m of every track for one window (limit.hip), win_frames + 2 * lookahead + hold + 2 * taps doubles each: 0 for what the
// data call refuses
size_t RRX_tracks_limit_window_work_doubles(int ntracks, size_t win_frames, int taps, size_t lookahead, size_t hold)
{
  if (ntracks < 1 || taps < 1 || taps > RRX_TP_MAX_TAPS || lookahead < 1 || lookahead > RRX_LIMIT_MAX_LOOKAHEAD || hold > RRX_LIMIT_MAX_HOLD)
    return 0;
  const size_t most = size_t(1) << 60, per = 2 * size_t(ntracks); // (2^32 at the most)
  if (win_frames >= most / per) return 0;
  const size_t each = win_frames + 2 * lookahead + hold + 2 * size_t(taps); // below 2^60 + 2^13
  return each >= (most + per - 1) / per ? 0 : per * each;
}

namespace {

// RRX_tracks_limit_window_device / RRX_debug_tracks_limit_window_host: everything that can be refused from the arguments alone
int tracks_limit_window_args(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *buf, size_t buf_stride, size_t buf_first,
                             size_t buf_frames, size_t row_frames, size_t win_first, size_t win_frames, int dst_format, void *dst,
                             size_t dst_stride, const double *gain, double ceiling, const double *coefs, int phases, int taps, size_t lookahead,
                             size_t hold, double *reduction, unsigned long long *limited, double *work, size_t work_doubles, rsmp::LimitArgs &a,
                             rsmp::LimitWindow &lw)
{
  if (!tracks || !buf || !dst || ntracks < 1 || nch < 1) return RR_INVPARAM;
  if (!float_format(src_format)) return RR_INVPARAM;
  int rc = true_peak_filter(coefs, phases, taps, a.f);
  if (rc != RR_OK) return rc;
  const size_t most = most_frames(nch) / size_t(ntracks); // (nor has a virtual row, of which the buffer holds a part)
  if (row_frames > most || buf_stride > most) return RR_INVPARAM;
  rsmp::TracksWindow w; // the window lies inside the rows, fits the destination's pitch, and the destination is one a device can hold
  if (tracks_window_args(ntracks, nch, row_frames, win_first, win_frames, dst_stride, w) != RR_OK) return RR_INVPARAM;
  rc = limit_scalars(src_format, dst_format, ceiling, lookahead, hold, work, work_doubles,
                     RRX_tracks_limit_window_work_doubles(ntracks, win_frames, a.f.taps, lookahead, hold),
                     (unsigned long long)win_frames + 2 * lookahead + hold + 2 * (unsigned)a.f.taps, a);
  if (rc != RR_OK) return rc;
  // coverage: the window and its halo, as far as the rows go (every term is below 2^60 + 2^13)
  const size_t back = size_t(rsmp::limit_reach_back(a.f.taps, unsigned(lookahead), unsigned(hold)));
  const size_t ahead = size_t(rsmp::limit_reach_ahead(a.f.taps, unsigned(lookahead)));
  const size_t want_first = win_first > back ? win_first - back : 0;
  const size_t want_end = win_first + win_frames + ahead < row_frames ? win_first + win_frames + ahead : row_frames;
  if (buf_first + buf_frames < buf_first || buf_first + buf_frames > row_frames || buf_stride < buf_frames) return RR_INVPARAM;
  if (buf_first > want_first || buf_first + buf_frames < want_end) return RR_INVPARAM;
  const uintptr_t sb = uintptr_t(ntracks) * buf_stride * uintptr_t(nch) * (a.src_double ? 8 : 4);
  const uintptr_t db = uintptr_t(ntracks) * dst_stride * uintptr_t(nch) * (a.dst_double ? 8 : 4);
  if (buf == dst || !limit_overlap_ok(buf, sb, dst, db, false)) return RR_INVPARAM;
  a.src = buf;
  a.dst = dst;
  a.gain = gain;
  a.reduction = reduction;
  a.limited = limited;
  a.tracks = reinterpret_cast<const rsmp::Track *>(tracks);
  a.src_stride = (unsigned long long)buf_stride * nch;
  a.dst_stride = (unsigned long long)dst_stride * nch;
  a.frames = row_frames;
  a.nstreams = ntracks;
  a.nch = nch;
  lw.win_first = win_first;
  lw.win_frames = win_frames;
  lw.buf_first = buf_first;
  lw.buf_frames = buf_frames;
  return RR_OK;
}

} // namespace

// RRX_tracks_limit_device on a window of the rows, from a buffer that holds the window and its halo (limit.hip).
int RRX_tracks_limit_window_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch, int src_format,
                                   const void *d_buf, size_t buf_stride, size_t buf_first, size_t buf_frames, size_t row_frames,
                                   size_t win_first, size_t win_frames, int dst_format, void *d_dst, size_t dst_stride, const double *d_gain,
                                   double ceiling, const double *coefs, int phases, int taps, size_t lookahead, size_t hold, double *d_reduction,
                                   unsigned long long *d_limited, double *d_work, size_t work_doubles)
{
  rsmp::LimitArgs a;
  rsmp::LimitWindow w;
  const int rc = tracks_limit_window_args(d_tracks, ntracks, nch, src_format, d_buf, buf_stride, buf_first, buf_frames, row_frames, win_first,
                                          win_frames, dst_format, d_dst, dst_stride, d_gain, ceiling, coefs, phases, taps, lookahead, hold,
                                          d_reduction, d_limited, d_work, work_doubles, a, w);
  if (rc != RR_OK) return rc;
  return on_device(device, !row_frames || !win_frames, [&] { return rsmp::launch_limit(static_cast<hipStream_t>(hip_stream), a, &w); });
}

int RRX_debug_tracks_limit_window_host(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *buf, size_t buf_stride,
                                       size_t buf_first, size_t buf_frames, size_t row_frames, size_t win_first, size_t win_frames,
                                       int dst_format, void *dst, size_t dst_stride, const double *gain, double ceiling, const double *coefs,
                                       int phases, int taps, size_t lookahead, size_t hold, double *reduction, unsigned long long *limited,
                                       double *work, size_t work_doubles)
{
  rsmp::LimitArgs a;
  rsmp::LimitWindow w;
  return on_host(
      [&] {
        return tracks_limit_window_args(tracks, ntracks, nch, src_format, buf, buf_stride, buf_first, buf_frames, row_frames, win_first,
                                        win_frames, dst_format, dst, dst_stride, gain, ceiling, coefs, phases, taps, lookahead, hold, reduction,
                                        limited, work, work_doubles, a, w);
      },
      !row_frames || !win_frames, [&] { rsmp::limit_host(a, &w); });
}

// the window call's r and m of every track and C, A, B, S of the pieces of a window (limit_release_window.hip): 0 for what the
// data call refuses
size_t RRX_tracks_limit_release_window_work_doubles(int ntracks, size_t win_frames, int taps, size_t lookahead, size_t hold, size_t block)
{
  if (block < RRX_LIMIT_RELEASE_MIN_BLOCK || block > RRX_LIMIT_RELEASE_MAX_BLOCK) return 0;
  if (!RRX_tracks_limit_window_work_doubles(ntracks, win_frames, taps, lookahead, hold)) return 0; // (win_frames below 2^60 / (2 * ntracks))
  const size_t most = size_t(1) << 60, n = size_t(ntracks);
  const size_t each = 2 * (win_frames + 2 * lookahead + hold + 2 * size_t(taps)) +
                      4 * size_t(rsmp::limit_release_window_pieces(win_frames, unsigned(lookahead), unsigned(block))); // below 2^61
  return each >= (most + n - 1) / n ? 0 : n * each;
}

namespace {

// RRX_tracks_limit_release_window_device / RRX_debug_tracks_limit_release_window_host: what the release, its block, the two
// states and the work buffer add to a validated window call.  Per track r, C, A in the first half of its share and m, B, S in
// the second, each half `a.work_stride` doubles: limit.hip's kernels find r and m where they look for them.
int tracks_limit_release_window_args(double release, size_t block, const double *state_in, double *state_out, double *work, size_t work_doubles,
                                     rsmp::LimitArgs &a, const rsmp::LimitWindow &w, rsmp::LimitReleaseWindowArgs &r)
{
  static_assert(RRX_LIMIT_RELEASE_WIN_STATE == rsmp::kLimitReleaseWinState, "the header's constant is the kernels'");
  if (!(release >= 0.0) || !(release < 1.0)) return RR_INVPARAM; // (a NaN fails both)
  const size_t need = RRX_tracks_limit_release_window_work_doubles(a.nstreams, size_t(w.win_frames), a.f.taps, a.lookahead, a.hold, block);
  if (!need || !work || work_doubles < need) return RR_INVPARAM;
  if (measure_window_state(state_in, state_out, size_t(w.win_first), uintptr_t(a.nstreams) * rsmp::kLimitReleaseWinState) != RR_OK) return RR_INVPARAM;
  const unsigned long long each = w.win_frames + 2 * a.lookahead + a.hold + 2 * (unsigned)a.f.taps;
  const unsigned long long sums = rsmp::limit_release_window_pieces(w.win_frames, a.lookahead, unsigned(block));
  a.work_stride = each + 2 * sums;
  r.work = work;
  r.tracks = a.tracks;
  r.state_in = state_in;
  r.state_out = state_out;
  r.row_frames = a.frames;
  r.win_first = w.win_first;
  r.win_frames = w.win_frames;
  r.stream_stride = 2 * a.work_stride;
  r.m_off = a.work_stride;
  r.c_off = each;
  r.b_off = a.work_stride + each;
  r.sum_stride = sums;
  r.lookahead = a.lookahead;
  r.block = unsigned(block);
  r.a = release;
  r.b = 1.0 - release;
  r.ntracks = a.nstreams;
  return RR_OK;
}

} // namespace

// RRX_tracks_limit_window_device with the release of RRX_tracks_limit_release_device, the scan's state carried per track
// (limit_release_window.hip).  The window call's *_args function wants its own share of work, which the release's buffer always
// holds: it is told there is enough.
int RRX_tracks_limit_release_window_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch, int src_format,
                                           const void *d_buf, size_t buf_stride, size_t buf_first, size_t buf_frames, size_t row_frames,
                                           size_t win_first, size_t win_frames, int dst_format, void *d_dst, size_t dst_stride,
                                           const double *d_gain, double ceiling, const double *coefs, int phases, int taps, size_t lookahead,
                                           size_t hold, double release, size_t block, const double *d_state_in, double *d_state_out,
                                           double *d_reduction, unsigned long long *d_limited, double *d_work, size_t work_doubles)
{
  rsmp::LimitArgs a;
  rsmp::LimitWindow w;
  rsmp::LimitReleaseWindowArgs r;
  int rc = tracks_limit_window_args(d_tracks, ntracks, nch, src_format, d_buf, buf_stride, buf_first, buf_frames, row_frames, win_first,
                                    win_frames, dst_format, d_dst, dst_stride, d_gain, ceiling, coefs, phases, taps, lookahead, hold,
                                    d_reduction, d_limited, d_work, ~size_t(0), a, w);
  if (rc == RR_OK) rc = tracks_limit_release_window_args(release, block, d_state_in, d_state_out, d_work, work_doubles, a, w, r);
  if (rc != RR_OK) return rc;
  return on_device(device, !row_frames || !win_frames,
                   [&] { return rsmp::launch_limit_release_window(static_cast<hipStream_t>(hip_stream), a, w, r); });
}

int RRX_debug_tracks_limit_release_window_host(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *buf, size_t buf_stride,
                                               size_t buf_first, size_t buf_frames, size_t row_frames, size_t win_first, size_t win_frames,
                                               int dst_format, void *dst, size_t dst_stride, const double *gain, double ceiling,
                                               const double *coefs, int phases, int taps, size_t lookahead, size_t hold, double release,
                                               size_t block, const double *state_in, double *state_out, double *reduction,
                                               unsigned long long *limited, double *work, size_t work_doubles)
{
  rsmp::LimitArgs a;
  rsmp::LimitWindow w;
  rsmp::LimitReleaseWindowArgs r;
  return on_host(
      [&] {
        const int rc = tracks_limit_window_args(tracks, ntracks, nch, src_format, buf, buf_stride, buf_first, buf_frames, row_frames, win_first,
                                                win_frames, dst_format, dst, dst_stride, gain, ceiling, coefs, phases, taps, lookahead, hold,
                                                reduction, limited, work, ~size_t(0), a, w);
        return rc != RR_OK ? rc : tracks_limit_release_window_args(release, block, state_in, state_out, work, work_doubles, a, w, r);
      },
      !row_frames || !win_frames, [&] { rsmp::limit_release_window_host(a, w, r); });
}

namespace {

// the matrix of the mixing calls: RR_INVPARAM for a NULL pointer, a channel count outside 1..RRX_MIX_MAX_CH or a non-finite
// coefficient; `m` gets the connected terms
static int mix_matrix(const double *mix, int nch_src, int nch_dst, rsmp::TracksMix &m)
{
  static_assert(RRX_MIX_MAX_CH == rsmp::kMixMaxCh, "the header's constant is the kernels'");
  if (!mix || nch_src < 1 || nch_src > RRX_MIX_MAX_CH || nch_dst < 1 || nch_dst > RRX_MIX_MAX_CH) return RR_INVPARAM;
  return rsmp::tracks_mix_build(mix, nch_src, nch_dst, m) ? RR_OK : RR_INVPARAM;
}

// RRX_mix_device / RRX_debug_mix_host: everything that can be refused from the arguments alone
static int mix_rows_args(int fmt, const void *src, size_t src_stride, int nstreams, size_t frames, int nch_src, void *dst, size_t dst_stride,
                         int nch_dst, const double *mix, rsmp::MixRowsArgs &a, rsmp::TracksMix &m)
{
  const int rc = mix_matrix(mix, nch_src, nch_dst, m);
  if (rc != RR_OK) return rc;
  if (!float_format(fmt) || !src || !dst || nstreams < 1) return RR_INVPARAM;
  if (nstreams > 1 && (src_stride < frames || dst_stride < frames)) return RR_INVPARAM;
  if (frames > most_frames(RRX_MIX_MAX_CH)) return RR_INVPARAM;
  if (nstreams > 1 && (src_stride > most_frames(RRX_MIX_MAX_CH) / size_t(nstreams) || dst_stride > most_frames(RRX_MIX_MAX_CH) / size_t(nstreams)))
    return RR_INVPARAM;
  // the two buffers share no byte (equal pointers overlap); samples below 2^60 each: no wrap
  const uintptr_t size = fmt == RRX_FMT_DOUBLE ? 8 : 4, rows = uintptr_t(nstreams - 1);
  const uintptr_t sb = (rows * src_stride + frames) * uintptr_t(nch_src) * size, db = (rows * dst_stride + frames) * uintptr_t(nch_dst) * size;
  const uintptr_t x = reinterpret_cast<uintptr_t>(src), y = reinterpret_cast<uintptr_t>(dst);
  if (x == y || (x < y ? y - x < sb : x - y < db)) return RR_INVPARAM;
  a.src = src;
  a.dst = dst;
  a.src_stride = nstreams > 1 ? (unsigned long long)src_stride * nch_src : 0;
  a.dst_stride = nstreams > 1 ? (unsigned long long)dst_stride * nch_dst : 0;
  a.frames = frames;
  a.nstreams = nstreams;
  a.is_double = fmt == RRX_FMT_DOUBLE;
  return RR_OK;
}

// RRX_tracks_stage_mix_device / RRX_tracks_stage_mix_window_device: the matrix, then what the un-mixed calls refuse, with nch_src
// in the source sizes and nch in the row sizes
static int tracks_stage_mix_args(size_t in_rate, size_t out_rate, const RRX_track *tracks, int ntracks, int src_format, int nch_src,
                                 const void *packed, size_t src_total, int nch, const double *mix, fb_sample_t *rows, size_t row_frames,
                                 rsmp::TracksStageArgs &a, rsmp::TracksMix &m)
{
  int rc = mix_matrix(mix, nch_src, nch, m);
  if (rc == RR_OK) rc = tracks_stage_args(in_rate, out_rate, tracks, ntracks, nch, src_format, packed, src_total, rows, row_frames, a);
  if (rc != RR_OK) return rc;
  return src_total > most_frames(nch_src) ? RR_INVPARAM : RR_OK;
}

} // namespace

// A matrix on device-resident rows (tracks_mix.hip).
int RRX_mix_device(int device, void *hip_stream, int fmt, const void *d_src, size_t src_stride, int nstreams, size_t frames, int nch_src,
                   void *d_dst, size_t dst_stride, int nch_dst, const double *mix)
{
  rsmp::MixRowsArgs a;
  rsmp::TracksMix m;
  const int rc = mix_rows_args(fmt, d_src, src_stride, nstreams, frames, nch_src, d_dst, dst_stride, nch_dst, mix, a, m);
  if (rc != RR_OK) return rc;
  return on_device(device, !frames, [&] { return rsmp::launch_mix_rows(static_cast<hipStream_t>(hip_stream), a, m); });
}

int RRX_debug_mix_host(int fmt, const void *src, size_t src_stride, int nstreams, size_t frames, int nch_src, void *dst, size_t dst_stride,
                       int nch_dst, const double *mix)
{
  rsmp::MixRowsArgs a;
  rsmp::TracksMix m;
  return on_host([&] { return mix_rows_args(fmt, src, src_stride, nstreams, frames, nch_src, dst, dst_stride, nch_dst, mix, a, m); }, !frames,
                 [&] { rsmp::mix_rows_host(a, m); });
}

// The stage pass of a ragged batch with the mix on load (tracks_mix.hip).
int RRX_tracks_stage_mix_device(int device, void *hip_stream, size_t in_rate, size_t out_rate, const RRX_track *d_tracks, int ntracks,
                                int src_format, int nch_src, const void *d_packed, size_t src_total, int nch, const double *mix,
                                fb_sample_t *d_rows, size_t row_frames)
{
  rsmp::TracksStageArgs a;
  rsmp::TracksMix m;
  const int rc = tracks_stage_mix_args(in_rate, out_rate, d_tracks, ntracks, src_format, nch_src, d_packed, src_total, nch, mix, d_rows,
                                       row_frames, a, m);
  if (rc != RR_OK) return rc;
  return on_device(device, false, [&] { return rsmp::launch_tracks_stage_mix(static_cast<hipStream_t>(hip_stream), a, m); });
}

int RRX_tracks_stage_mix_window_device(int device, void *hip_stream, size_t in_rate, size_t out_rate, const RRX_track *d_tracks, int ntracks,
                                       int src_format, int nch_src, const void *d_packed, size_t src_total, int nch, const double *mix,
                                       size_t row_frames, size_t win_first, size_t win_frames, fb_sample_t *d_win, size_t win_stride)
{
  rsmp::TracksStageArgs a;
  rsmp::TracksMix m;
  rsmp::TracksWindow w;
  int rc = tracks_stage_mix_args(in_rate, out_rate, d_tracks, ntracks, src_format, nch_src, d_packed, src_total, nch, mix, d_win, row_frames, a, m);
  if (rc == RR_OK) rc = tracks_window_args(ntracks, nch, row_frames, win_first, win_frames, win_stride, w);
  if (rc != RR_OK) return rc;
  return on_device(device, !win_frames, [&] { return rsmp::launch_tracks_stage_mix_window(static_cast<hipStream_t>(hip_stream), a, m, w); });
}

// Test hook: the mixed float32 frames of a host source, a serial loop over the function the kernels call
int RRX_debug_tracks_mix_host(int src_format, const void *src, int nch_src, size_t first_frame, size_t count, int nch, const double *mix,
                              float *out)
{
  if (!rsmp::knobs().test_hooks) return -1;
  const int kind = tracks_src_kind(src_format);
  rsmp::TracksMix m;
  if (kind < 0 || !src || !out || mix_matrix(mix, nch_src, nch, m) != RR_OK) return RR_INVPARAM;
  const size_t fb = size_t(nch_src) * rsmp::tracks_src_bytes(kind);
  for (size_t i = 0; i < count; ++i)
    for (int o = 0; o < nch; ++o) out[i * nch + o] = rsmp::tracks_mix_sample(m, kind, static_cast<const unsigned char *>(src) + (first_frame + i) * fb, o);
  return RR_OK;
}

} // extern "C"
