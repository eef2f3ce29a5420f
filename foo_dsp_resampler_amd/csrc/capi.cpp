// C ABI: the reference's ratelib.h entry points (rate/rate_uni.c:27-111,210-231) plus the
// device / batch extensions of include/ratelib_amd.h, all thin shims over rsmp::Engine.
#include "../../include/ratelib_amd.h"

#include "engine.hpp"
#include "finish.hpp"
#include "finish_shaped.hpp"
#include "loudness.hpp"
#include "loudness_stats.hpp"
#include "lpc.hpp"
#include "measure_window.hpp"
#include "tracks.hpp"
#include "true_peak.hpp"
#include "limit.hpp"
#include "limit_release.hpp"
#include "limit_release_window.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

struct RR_handle_tag {
  rsmp::Engine *eng;
};

namespace {

void (*g_alloc_handler)(void) = nullptr;
int g_initialized = 0;
// RATELIB_AMD_DEVICES (read by init_ratelib): devices RR_open / RRX_open_batch deal new handles over, round-robin.
// Empty = a handle lives on the calling thread's current device.
std::vector<int> g_devices;
std::atomic<unsigned> g_next_device{0};

// "all" or a comma list of device indices; false when it names a device the process does not have or that is not gfx950
bool parse_devices(const char *spec, int count, std::vector<int> &out)
{
  out.clear();
  if (!spec || !*spec) return true;
  if (std::strcmp(spec, "all") == 0) {
    for (int d = 0; d < count; ++d) out.push_back(d);
  } else {
    for (const char *p = spec; *p;) {
      char *end = nullptr;
      const long d = std::strtol(p, &end, 10);
      if (end == p || d < 0 || d >= count) return false;
      out.push_back(int(d));
      p = *end == ',' ? end + 1 : end;
      if (*end && *end != ',') return false;
    }
  }
  for (int d : out)
    if (!rsmp::device_is_gfx950(d)) return false;
  return true;
}

rsmp::Config to_config(const RR_config *c)
{
  rsmp::Config k;
  k.in_rate = c->in_rate;
  k.out_rate = c->out_rate;
  k.phase = c->phase;
  k.bandwidth = c->bandwidth;
  k.allow_aliasing = c->allow_aliasing;
  k.quality = c->quality == RR_best ? 0 : 1;
  return k;
}

// engine codes are numerically the RR_error values; an allocation failure additionally runs the
// registered handler (xmalloc.c:38-43) from this plain host frame, where unwinding is safe
int finish(int rc)
{
  if (rc == RR_ENOMEM && g_alloc_handler) g_alloc_handler();
  return rc;
}

// No C++ exception of ours may cross the C ABI: host-side containers can throw std::bad_alloc, which is
// reported like any other allocation failure (the handler itself may throw, as the plugin's does; that is the
// caller's contract, rate/xmalloc.c:38-43).
template <class Fn> int guarded(RR_handle *h, Fn fn)
{
  int rc;
  rsmp::DeviceScope on(h->eng->device()); // the handle's device, whatever the calling thread has selected
  if (!on.ok()) return finish(RR_INTERNAL);
  try {
    rc = fn();
  } catch (const std::bad_alloc &) {
    rc = RR_ENOMEM;
  } catch (...) {
    rc = RR_INTERNAL;
  }
  return finish(rc);
}

// The data calls, for host and for device memory: `format` is what the caller believes the buffers hold and must be the
// handle's.  It is checked before anything moves, so a mismatch leaves the handle as it was.
int push_host(RR_handle *h, int format, const void *ibuf, size_t in_stride, size_t isamp)
{
  if (!h) return RR_NULLHANDLE;
  if (h->eng->format() != format) return RR_INVPARAM;
  return guarded(h, [&] { return h->eng->push_host(ibuf, in_stride, isamp); });
}

int pull_host(RR_handle *h, int format, void *obuf, size_t out_stride, size_t osamp, size_t *ogen)
{
  if (!h) return RR_NULLHANDLE;
  if (h->eng->format() != format) return RR_INVPARAM;
  return guarded(h, [&] { return h->eng->pull_host(obuf, out_stride, osamp, ogen); });
}

int flow_host(RR_handle *h, int format, const void *ibuf, size_t in_stride, void *obuf, size_t out_stride, size_t isamp, size_t osamp,
              size_t *iused, size_t *ogen)
{
  if (!h) return RR_NULLHANDLE;
  if (h->eng->format() != format) return RR_INVPARAM;
  return guarded(h, [&] { return h->eng->flow_host(ibuf, in_stride, obuf, out_stride, isamp, osamp, iused, ogen); });
}

int push_device(RR_handle *h, int format, const void *d_ibuf, size_t in_stride, size_t isamp)
{
  if (!h) return RR_NULLHANDLE;
  if (h->eng->format() != format) return RR_INVPARAM;
  return guarded(h, [&] { return h->eng->push_device(d_ibuf, in_stride, isamp); });
}

int pull_device(RR_handle *h, int format, void *d_obuf, size_t out_stride, size_t osamp, size_t *ogen)
{
  if (!h) return RR_NULLHANDLE;
  if (h->eng->format() != format) return RR_INVPARAM;
  return guarded(h, [&] { return h->eng->pull_device(d_obuf, out_stride, osamp, ogen); });
}

int flow_device(RR_handle *h, int format, const void *d_ibuf, size_t in_stride, void *d_obuf, size_t out_stride, size_t isamp,
                size_t osamp, size_t *iused, size_t *ogen)
{
  if (!h) return RR_NULLHANDLE;
  if (h->eng->format() != format) return RR_INVPARAM;
  return guarded(h, [&] { return h->eng->flow_device(d_ibuf, in_stride, d_obuf, out_stride, isamp, osamp, iused, ogen); });
}

// device: -1 = the default placement (RATELIB_AMD_DEVICES round-robin, else the calling thread's current device)
int open_common(const RR_config *config, int nchannels, int nstreams, int device, RR_handle **const handle, int format = RRX_FMT_FLOAT)
{
  if (handle == nullptr) return RR_INVPARAM;
  *handle = nullptr;
  if (!g_initialized) return RR_EXTUNINIT;
  if (config == nullptr) return RR_INVPARAM;
  RR_handle *h = new (std::nothrow) RR_handle_tag();
  if (!h) return finish(RR_ENOMEM);
  h->eng = nullptr;
  if (device < 0 && !g_devices.empty()) device = g_devices[g_next_device.fetch_add(1) % g_devices.size()];
  int rc;
  try {
    rc = rsmp::Engine::create(to_config(config), nchannels, nstreams, device, &h->eng, format);
  } catch (const std::bad_alloc &) {
    rc = RR_ENOMEM;
  } catch (...) {
    rc = RR_INTERNAL;
  }
  if (rc != RR_OK) {
    delete h;
    return finish(rc);
  }
  *handle = h;
  return RR_OK;
}

} // namespace

extern "C" {

int init_ratelib(void (*alloc_error_handler)(void))
{
  g_initialized = 0;
  if (alloc_error_handler == nullptr) return -1;
  g_alloc_handler = alloc_error_handler;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n < 1) return -1; // no GPU: refuse loudly, there is no CPU path
  if (!parse_devices(std::getenv("RATELIB_AMD_DEVICES"), n, g_devices)) return -1; // names a device we cannot run on
  if (g_devices.empty() && !rsmp::device_is_gfx950()) return -1; // the code object is gfx950-only: refuse here, not at the first launch
  (void)rsmp::knobs(); // the environment is read here, once
  g_initialized = 1;
  return 0;
}

void close_ratelib(void) { g_initialized = 0; }

int RR_open(const RR_config *config, int nchannels, RR_handle **const handle) { return open_common(config, nchannels, 1, -1, handle); }

int RRX_open_batch(const RR_config *config, int nchannels, int nstreams, RR_handle **const handle)
{
  return open_common(config, nchannels, nstreams, -1, handle);
}

int RRX_open_batch_on(const RR_config *config, int nchannels, int nstreams, int device, RR_handle **const handle)
{
  if (device < 0) {
    if (handle) *handle = nullptr;
    return RR_INVPARAM;
  }
  return open_common(config, nchannels, nstreams, device, handle);
}

int RRX_device(const RR_handle *h) { return h ? h->eng->device() : -1; }

int RRX_open_batch_fmt(const RR_config *config, int nchannels, int nstreams, int device, int format, RR_handle **const handle)
{
  if (format != RRX_FMT_FLOAT && format != RRX_FMT_DOUBLE && format != RRX_FMT_S16 && format != RRX_FMT_S32) { // checked before anything touches a device
    if (handle) *handle = nullptr;
    return RR_INVPARAM;
  }
  if (device < -1) {
    if (handle) *handle = nullptr;
    return RR_INVPARAM;
  }
  return open_common(config, nchannels, nstreams, device, handle, format);
}

int RRX_format(const RR_handle *h) { return h ? h->eng->format() : -1; }

// One format-tagged set for all four formats; on float and double handles this is the code path of RRX_*_strided /
// RRX_*_device and RRX_*_double.
int RRX_push_samples(RR_handle *h, int format, const void *ibuf, size_t in_stride, size_t isamp)
{ return push_host(h, format, ibuf, in_stride, isamp); }

int RRX_pull_samples(RR_handle *h, int format, void *obuf, size_t out_stride, size_t osamp, size_t *ogen)
{ return pull_host(h, format, obuf, out_stride, osamp, ogen); }

int RRX_flow_samples(RR_handle *h, int format, const void *ibuf, size_t in_stride, void *obuf, size_t out_stride, size_t isamp,
                     size_t osamp, size_t *iused, size_t *ogen)
{
  if (h && h->eng->nstreams() == 1) in_stride = isamp, out_stride = osamp; // packed, as RR_flow
  return flow_host(h, format, ibuf, in_stride, obuf, out_stride, isamp, osamp, iused, ogen);
}

int RRX_push_device_samples(RR_handle *h, int format, const void *d_ibuf, size_t in_stride, size_t isamp)
{ return push_device(h, format, d_ibuf, in_stride, isamp); }

int RRX_pull_device_samples(RR_handle *h, int format, void *d_obuf, size_t out_stride, size_t osamp, size_t *ogen)
{ return pull_device(h, format, d_obuf, out_stride, osamp, ogen); }

int RRX_flow_device_samples(RR_handle *h, int format, const void *d_ibuf, size_t in_stride, void *d_obuf, size_t out_stride,
                            size_t isamp, size_t osamp, size_t *iused, size_t *ogen)
{ return flow_device(h, format, d_ibuf, in_stride, d_obuf, out_stride, isamp, osamp, iused, ogen); }

int RRX_push_double(RR_handle *h, const double *ibuf, size_t in_stride, size_t isamp)
{ return push_host(h, RRX_FMT_DOUBLE, ibuf, in_stride, isamp); }

int RRX_pull_double(RR_handle *h, double *obuf, size_t out_stride, size_t osamp, size_t *ogen)
{ return pull_host(h, RRX_FMT_DOUBLE, obuf, out_stride, osamp, ogen); }

int RRX_flow_double(RR_handle *h, const double *ibuf, size_t in_stride, double *obuf, size_t out_stride, size_t isamp, size_t osamp,
                    size_t *iused, size_t *ogen)
{
  if (h && h->eng->nstreams() == 1) in_stride = isamp, out_stride = osamp; // packed, as RR_flow
  return flow_host(h, RRX_FMT_DOUBLE, ibuf, in_stride, obuf, out_stride, isamp, osamp, iused, ogen);
}

int RRX_push_device_double(RR_handle *h, const double *d_ibuf, size_t in_stride, size_t isamp)
{ return push_device(h, RRX_FMT_DOUBLE, d_ibuf, in_stride, isamp); }

int RRX_pull_device_double(RR_handle *h, double *d_obuf, size_t out_stride, size_t osamp, size_t *ogen)
{ return pull_device(h, RRX_FMT_DOUBLE, d_obuf, out_stride, osamp, ogen); }

int RRX_flow_device_double(RR_handle *h, const double *d_ibuf, size_t in_stride, double *d_obuf, size_t out_stride, size_t isamp,
                           size_t osamp, size_t *iused, size_t *ogen)
{ return flow_device(h, RRX_FMT_DOUBLE, d_ibuf, in_stride, d_obuf, out_stride, isamp, osamp, iused, ogen); }

int RR_push(RR_handle *h, const fb_sample_t *ibuf, size_t isamp) { return push_host(h, RRX_FMT_FLOAT, ibuf, isamp, isamp); }

int RR_pull(RR_handle *h, fb_sample_t *obuf, size_t osamp, size_t *ogen)
{
  const size_t n = h ? (osamp < h->eng->available() ? osamp : h->eng->available()) : 0; // (one stream: the stride is not used)
  return pull_host(h, RRX_FMT_FLOAT, obuf, n, osamp, ogen);
}

int RR_flow(RR_handle *h, const fb_sample_t *ibuf, fb_sample_t *obuf, size_t isamp, size_t osamp, size_t *iused, size_t *ogen)
{
  if (h && h->eng->nstreams() != 1) return RR_INVPARAM; // packed layout of a batch is ambiguous here
  return flow_host(h, RRX_FMT_FLOAT, ibuf, isamp, obuf, osamp, isamp, osamp, iused, ogen);
}

int RR_drain(RR_handle *h)
{
  if (!h) return RR_NULLHANDLE;
  return guarded(h, [&] { return h->eng->drain(); });
}

int RRX_reset(RR_handle *h)
{
  if (!h) return RR_NULLHANDLE;
  return guarded(h, [&] { return h->eng->reset(); });
}

void RR_close(RR_handle **h)
{
  if (h == nullptr || *h == nullptr) return;
  delete (*h)->eng; // (~Engine selects the handle's device for its frees itself)
  delete *h;
  *h = nullptr;
}

const char *RR_strerror(int error)
{ // same strings as rate_uni.c:92-111
  switch (error) {
    case RR_OK: return "OK";
    case RR_ENOMEM: return "Not enough memory";
    case RR_INTERNAL: return "Internal error";
    case RR_NULLHANDLE: return "NULL handle";
    case RR_RATEERROR: return "Error in rate() functions";
    case RR_EXTUNINIT: return "Externals not initialized";
    default: return "Other error";
  }
}

int RRX_push_device(RR_handle *h, const fb_sample_t *d_ibuf, size_t in_stride, size_t isamp)
{ return push_device(h, RRX_FMT_FLOAT, d_ibuf, in_stride, isamp); }

int RRX_pull_device(RR_handle *h, fb_sample_t *d_obuf, size_t out_stride, size_t osamp, size_t *ogen)
{ return pull_device(h, RRX_FMT_FLOAT, d_obuf, out_stride, osamp, ogen); }

int RRX_flow_device(RR_handle *h, const fb_sample_t *d_ibuf, size_t in_stride, fb_sample_t *d_obuf, size_t out_stride,
                    size_t isamp, size_t osamp, size_t *iused, size_t *ogen)
{ return flow_device(h, RRX_FMT_FLOAT, d_ibuf, in_stride, d_obuf, out_stride, isamp, osamp, iused, ogen); }

int RRX_push_strided(RR_handle *h, const fb_sample_t *ibuf, size_t in_stride, size_t isamp)
{ return push_host(h, RRX_FMT_FLOAT, ibuf, in_stride, isamp); }

int RRX_pull_strided(RR_handle *h, fb_sample_t *obuf, size_t out_stride, size_t osamp, size_t *ogen)
{ return pull_host(h, RRX_FMT_FLOAT, obuf, out_stride, osamp, ogen); }

int RRX_set_stream(RR_handle *h, void *hip_stream)
{
  if (!h) return RR_NULLHANDLE;
  const bool own = hip_stream == RRX_STREAM_OWN;
  return guarded(h, [&] { return h->eng->set_stream(own ? nullptr : static_cast<hipStream_t>(hip_stream), own); });
}

int RRX_sync(RR_handle *h)
{
  if (!h) return RR_NULLHANDLE;
  return guarded(h, [&] { return h->eng->sync(); });
}

int RRX_profile(RR_handle *h, int enable)
{
  if (!h) return RR_NULLHANDLE;
  return guarded(h, [&] { h->eng->set_profiling(enable != 0); return int(RR_OK); });
}

int RRX_profile_read(RR_handle *h, double *hot_ms, long long *hot_launches, double *other_ms, long long *other_launches)
{
  if (!h) return RR_NULLHANDLE;
  return guarded(h, [&] { return h->eng->read_profile(hot_ms, hot_launches, other_ms, other_launches); });
}

int RRX_profile_report(RR_handle *h, char *buf, size_t cap)
{
  if (!h) return -RR_NULLHANDLE;
  if (!buf || !cap) return -RR_INVPARAM;
  std::string s;
  int rc = guarded(h, [&] { return h->eng->read_profile_json(s); });
  if (rc) return -rc;
  size_t n = s.size() < cap - 1 ? s.size() : cap - 1;
  std::memcpy(buf, s.data(), n);
  buf[n] = 0;
  return int(n);
}

void RRX_debug_fail_alloc(int nth) { rsmp::Engine::fail_alloc_after(nth); }

// RRX_walk_geom -> the prep kernel's arguments for entries 0 .. k (false: refused)
static bool walk_geom_args(const RRX_walk_geom *g, int k, rsmp::FusedPrepArgs &pa)
{
  if (!rsmp::knobs().test_hooks || !g || k < 0) return false;
  if (g->polyL < 1 || g->step < 1 || g->V < 1 || g->n < 1 || g->KS < 1 || g->nsub < 0 || (g->nsub > 0 && g->Vs < 1)) return false;
  pa.b_offset = g->b_offset;
  pa.B0 = g->B0;
  pa.at0 = g->at0;
  pa.V = g->V;
  pa.polyL = g->polyL;
  pa.step = g->step;
  pa.n = g->n;
  pa.nblocks = k + 1;
  pa.two_round = g->two_round;
  pa.KS = g->KS;
  pa.qb_max = g->qb_max;
  pa.qb_min = g->qb_min;
  pa.ra_end = g->ra_end;
  pa.rb_start = g->rb_start;
  pa.clip_lo = 0;
  pa.clip_hi = 0x7fffffffffffffffLL;
  pa.nsub = g->nsub;
  pa.Vs = g->Vs;
  return true;
}

long long RRX_debug_tile_walk(const RRX_walk_geom *g, int k, long long *head, int *slots, size_t cap)
{
  rsmp::FusedPrepArgs pa;
  if (!head || (cap && !slots) || !walk_geom_args(g, k, pa)) return -1;
  return (long long)rsmp::fused_walk_enumerate(pa, k, head, slots, cap);
}

int RRX_debug_walk_start(const RRX_walk_geom *g, int k, RRX_walk_start *out)
{
  rsmp::FusedPrepArgs pa;
  if (!out || !walk_geom_args(g, k, pa)) return -1;
  static_assert(sizeof(RRX_walk_start) == 56 * sizeof(int), "RRX_walk_start mirrors rsmp::WalkStart");
  rsmp::fused_walk_start_host(pa, k, reinterpret_cast<int *>(out));
  return 0;
}

int RRX_debug_window_start(const RRX_walk_geom *g, int group, int bq, int *arith, int *table, unsigned rcp[3])
{
  if (!rsmp::knobs().test_hooks || !g || !arith || !table || !rcp) return -1;
  if (g->polyL < 1 || g->step < 1 || group < 0 || group >= (g->polyL + 15) / 16 || bq < 0 || bq > 3) return -2;
  return rsmp::fused_window_start_host(g->at0, g->step, g->polyL, group, bq, arith, table, rcp) ? 0 : -2;
}

// lpc/lpc.h:27 on device-resident frames.  Everything that can be refused from the arguments alone is refused before any
// device is touched.
int RRX_lpc_extrapolate_device(int device, void *hip_stream, fb_sample_t *d_data, size_t stream_stride, int nstreams, size_t data_len,
                               int nch, int lpc_order, size_t extra_bkwd, size_t extra_fwd)
{
  if (!d_data || nstreams < 1 || nch < 1 || lpc_order < 1 || lpc_order > rsmp::kLpcMaxOrder || data_len <= size_t(lpc_order)) return RR_INVPARAM;
  if (nstreams > 1 && stream_stride < extra_bkwd + data_len + extra_fwd) return RR_INVPARAM;
  if (device < -1 || (long long)nstreams * nch > 0x7fffffffLL) return RR_INVPARAM; // (one workgroup per channel of every stream)
  if (!g_initialized) return RR_EXTUNINIT;
  if (!extra_bkwd && !extra_fwd) return RR_OK;
  if (device >= 0) { // as RRX_open_batch_on
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) return RR_EXTUNINIT;
    if (device >= n) return RR_INVPARAM;
  }
  if (!rsmp::device_is_gfx950(device)) return RR_EXTUNINIT;
  rsmp::DeviceScope on(device); // restores the caller's device on return
  if (!on.ok()) return RR_INTERNAL;
  const hipError_t e = rsmp::launch_lpc_extrapolate(static_cast<hipStream_t>(hip_stream), d_data, stream_stride, nstreams, data_len,
                                                    nch, lpc_order, extra_bkwd, extra_fwd);
  return e == hipSuccess ? RR_OK : RR_INTERNAL;
}

namespace {

// RRX_finish_device / RRX_debug_finish_host: everything that can be refused from the arguments alone; fills `a` when it is RR_OK
int finish_args(int src_format, const void *src, size_t src_stride, int dst_format, void *dst, size_t dst_stride, int nstreams,
                size_t frames, int nch, const double *gain, int dither, unsigned long long seed, unsigned long long first_frame,
                double *peak, unsigned long long *clipped, rsmp::FinishArgs &a)
{
  if (!src || nstreams < 1 || nch < 1) return RR_INVPARAM;
  if (src_format != RRX_FMT_FLOAT && src_format != RRX_FMT_DOUBLE) return RR_INVPARAM;
  if (dst && dst_format != RRX_FMT_S16 && dst_format != RRX_FMT_S24_3 && dst_format != RRX_FMT_S32) return RR_INVPARAM;
  if (nstreams > 1 && (src_stride < frames || (dst && dst_stride < frames))) return RR_INVPARAM;
  if (!dst && !peak && !clipped) return RR_INVPARAM;
  if (first_frame + frames < first_frame) return RR_INVPARAM;               // the frame counter of the dither would wrap
  // No buffer has 2^60 samples: with that, frames * nch, stride * nch and the row offsets stream * stride * nch below and in
  // finish.hip (times up to 8 bytes a sample) cannot wrap, and a workgroup's 32-bit clip count cannot either (launch_typed).
  const size_t most = (~size_t(0) >> 4) / size_t(nch);
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
  a.bits = !dst ? 31 : dst_format == RRX_FMT_S16 ? 15 : dst_format == RRX_FMT_S24_3 ? 23 : 31; // measure only: the S32 grid
  a.dither = dither != 0;
  return RR_OK;
}

} // namespace

// The output stage on device-resident frames (finish.hip).  Refusals first, as in RRX_lpc_extrapolate_device.
int RRX_finish_device(int device, void *hip_stream, int src_format, const void *d_src, size_t src_stride, int dst_format, void *d_dst,
                      size_t dst_stride, int nstreams, size_t frames, int nch, const double *d_gain, int dither, unsigned long long seed,
                      unsigned long long first_frame, double *d_peak, unsigned long long *d_clipped)
{
  rsmp::FinishArgs a;
  const int rc = finish_args(src_format, d_src, src_stride, dst_format, d_dst, dst_stride, nstreams, frames, nch, d_gain, dither, seed,
                             first_frame, d_peak, d_clipped, a);
  if (rc != RR_OK) return rc;
  if (device < -1) return RR_INVPARAM;
  if (!g_initialized) return RR_EXTUNINIT;
  if (!frames) return RR_OK;
  if (device >= 0) { // as RRX_open_batch_on
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) return RR_EXTUNINIT;
    if (device >= n) return RR_INVPARAM;
  }
  if (!rsmp::device_is_gfx950(device)) return RR_EXTUNINIT;
  rsmp::DeviceScope on(device); // restores the caller's device on return
  if (!on.ok()) return RR_INTERNAL;
  return rsmp::launch_finish(static_cast<hipStream_t>(hip_stream), a) == hipSuccess ? RR_OK : RR_INTERNAL;
}

int RRX_debug_finish_host(int src_format, const void *src, size_t src_stride, int dst_format, void *dst, size_t dst_stride, int nstreams,
                          size_t frames, int nch, const double *gain, int dither, unsigned long long seed, unsigned long long first_frame,
                          double *peak, unsigned long long *clipped)
{
  if (!rsmp::knobs().test_hooks) return -1;
  rsmp::FinishArgs a;
  const int rc = finish_args(src_format, src, src_stride, dst_format, dst, dst_stride, nstreams, frames, nch, gain, dither, seed,
                             first_frame, peak, clipped, a);
  if (rc != RR_OK) return rc;
  if (frames) rsmp::finish_host(a);
  return RR_OK;
}

// foo_dsp_rate.cpp:96-101 with samples_len of util.h:38-48
int RRX_edge_geometry(size_t in_rate, size_t out_rate, size_t *n_add, size_t *n_drop, size_t *prime_len, size_t *inbuf)
{
  if (!in_rate || !out_rate || !n_add || !n_drop || !prime_len || !inbuf) return RR_INVPARAM;
  size_t a = in_rate, b = out_rate;
  while (b) { const size_t c = a % b; a = b; b = c; } // a = gcd
  const size_t v = a, r1 = in_rate / v, r2 = out_rate / v, z = r1 > r2 ? r1 : r2;
  size_t n = (v + 20 - 1) / 20; // 1/20 s ...
  if (z * n > 8192) n = 8192 / z; // ... but neither count above 8192 ...
  if (n < 1) n = 1;               // ... unless one period already is
  *n_add = r1 * n;
  *n_drop = r2 * n;
  const size_t prime = std::min<size_t>(std::max<size_t>(in_rate / 20, 1024), 16384);
  *prime_len = std::max<size_t>(prime, 2 * rsmp::kLpcMaxOrder + 1);
  *inbuf = std::min<size_t>(std::max<size_t>(in_rate / 10, 2048), 65536);
  return RR_OK;
}

namespace {

// The counters of a handle without the handle: Engine::init's fifo preloads and the counter half of Engine::advance
// (engine.cpp: advance_dft / advance_poly / advance_half with launch == false), on the plan alone, so that the geometry of a
// track can be stated without a device.  tests/test_tracks_api.py holds it to the CPU resampler's totals and
// tests/test_gpu_tracks.py to a real handle's.
struct CounterChain {
  const rsmp::ChainPlan &plan;
  rsmp::Book b;

  explicit CounterChain(const rsmp::ChainPlan &p) : plan(p)
  {
    const int ns = int(plan.stages.size());
    b.wr.assign(ns + 1, 0);
    b.rd.assign(ns + 1, 0);
    b.st.assign(ns, rsmp::Book::St());
    for (int i = 0; i < ns; ++i) {
      const rsmp::StageSpec &sp = plan.stages[i];
      b.wr[i] = sp.preload; // rate_base.h:417-422
      if (sp.kind == rsmp::StageKind::Dft) b.st[i].remL = sp.remL0;
      else if (sp.kind == rsmp::StageKind::Poly) b.st[i].at = sp.order == 0 ? (sp.at0 >> 32) : sp.at0;
    }
  }

  // one pass of rate_process after n frames were appended to fifo 0 (rate_base.h:425-441)
  void push(size_t n)
  {
    b.samples_in += n;
    while (b.samples_in > plan.cfg.in_rate && b.samples_out > plan.cfg.out_rate) {
      b.samples_in -= plan.cfg.in_rate;
      b.samples_out -= plan.cfg.out_rate;
    }
    b.wr[0] += (long long)n;
    for (int i = 0; i < int(plan.stages.size()); ++i) {
      const rsmp::StageSpec &sp = plan.stages[i];
      rsmp::Book::St &st = b.st[i];
      long long &rd = b.rd[i], &wro = b.wr[i + 1];
      const long long occ = b.wr[i] - rd;
      if (sp.kind == rsmp::StageKind::Dft) { // dft_filter.h:78-84, :150-152, :187
        const rsmp::DftFilter &f = plan.dft[sp.filt];
        const int N = f.N, ov = f.num_taps - 1, V = N - ov, L = sp.L;
        const bool stuffing = L != 1 && !(L >= 2 && !(L & (L - 1)));
        const int kept = sp.step < 0 ? N - ((((1 << -sp.step) - 1) * N + ov) >> -sp.step) : V;
        long long num_in = std::max<long long>(0, occ);
        while (st.remL + (long long)L * num_in >= N) {
          const int span = V - st.remL + L - 1;
          const int take = span / L, rem = span % L;
          rd += take;
          num_in -= take;
          if (stuffing) st.remL = L - 1 - rem;
          if (sp.step > 1) {
            const int j = (V - st.remM + sp.step - 1) / sp.step;
            st.remM = st.remM + j * sp.step - V;
            wro += j;
          } else
            wro += kept;
          ++st.B;
        }
      } else if (sp.kind == rsmp::StageKind::Poly) { // rate_filters_generic.h:281 / :477, :302-304 / :499-500
        const long long num_in = std::max<long long>(0, occ - sp.pre_post);
        long long count = 0;
        const long long step = sp.order == 0 ? (sp.step64 >> 32) : sp.step64;
        const long long lim = sp.order == 0 ? num_in * sp.L : (num_in << 32);
        if (st.at < lim) count = (lim - st.at + step - 1) / step;
        const long long at_end = st.at + count * step;
        if (sp.order == 0) {
          rd += at_end / sp.L;
          st.at = at_end % sp.L;
        } else {
          rd += at_end >> 32;
          st.at = at_end & 0xffffffffLL;
        }
        wro += count;
      } else { // rate_filters_generic.h:83, fifo.h:169
        const long long avail = std::max<long long>(0, occ - sp.pre_post);
        const long long num_out = (avail + 1) / 2;
        if (2 * num_out <= occ) rd += 2 * num_out;
        wro += num_out;
      }
    }
  }

  // Frames a handle yields in all for `total` frames pushed in isamp_max pieces, everything available pulled after each push,
  // then drained and pulled: Resampler.convert_track_device's loop.  The drain target is Engine::drain's (rate_base.h:454-468),
  // from the counters as rate_input's wrap by whole seconds left them.
  size_t drained_total(size_t total)
  {
    size_t pulled = 0;
    const size_t step = std::max<size_t>(plan.isamp_max, 1);
    for (size_t pos = 0; pos < total; pos += step) {
      push(std::min(step, total - pos));
      const size_t n = size_t(b.wr.back() - b.rd.back());
      b.rd.back() += (long long)n; // rate_base.h:447-448
      b.samples_out += n;
      pulled += n;
    }
    const size_t target = size_t(double(b.samples_in) / plan.factor + .5);
    return target <= b.samples_out ? pulled : pulled + (target - b.samples_out);
  }
};

// No track has 2^36 frames (18 days at 44.1 kHz): the geometry below walks a track's pushes one by one, and with this bound no sum
// of two of its terms can wrap.
constexpr size_t kTrackFramesMax = size_t(1) << 36;

// RRX_track_geometry on a plan that exists already
int track_geometry(const rsmp::ChainPlan &plan, size_t frames, size_t *lead, size_t *ext_frames, size_t *out_first, size_t *out_frames)
{
  if (frames > kTrackFramesMax) return RR_INVPARAM;
  size_t n_add = 0, n_drop = 0, prime = 0, inbuf = 0;
  const int rc = RRX_edge_geometry(plan.cfg.in_rate, plan.cfg.out_rate, &n_add, &n_drop, &prime, &inbuf);
  if (rc != RR_OK) return rc;
  const bool extend = frames > size_t(2 * rsmp::kLpcMaxOrder); // foo_dsp_rate.cpp:222-239: up to 64 frames go through as they are
  *lead = extend ? n_add : 0;
  *ext_frames = frames + 2 * *lead;
  *out_first = extend ? n_drop : 0;
  const size_t total = CounterChain(plan).drained_total(*ext_frames);
  *out_frames = total > 2 * *out_first ? total - 2 * *out_first : 0;
  return RR_OK;
}

// rows of `frames` input frames give at most this many output frames (the capacity Resampler.convert_track_device allocates);
// false: it does not fit a size_t
bool out_row_capacity(const rsmp::ChainPlan &plan, size_t frames, size_t *cap)
{
  const unsigned __int128 c = (unsigned __int128)frames * plan.cfg.out_rate / plan.cfg.in_rate + 2;
  if (c > (unsigned __int128)(~size_t(0))) return false;
  *cap = size_t(c);
  return true;
}

} // namespace

int RRX_track_geometry(const RR_config *config, size_t frames, size_t *lead, size_t *ext_frames, size_t *out_first, size_t *out_frames)
{
  if (!config || !lead || !ext_frames || !out_first || !out_frames) return RR_INVPARAM;
  try {
    rsmp::ChainPlan plan;
    const int rc = rsmp::make_plan(to_config(config), plan);
    if (rc) return rc;
    return track_geometry(plan, frames, lead, ext_frames, out_first, out_frames);
  } catch (const std::bad_alloc &) {
    return finish(RR_ENOMEM);
  } catch (...) {
    return RR_INTERNAL;
  }
}

int RRX_tracks_plan(const RR_config *config, const size_t *frames, int ntracks, RRX_track *table, size_t *row_frames, size_t *out_row_cap,
                    size_t *src_total, size_t *dst_total)
{
  if (!config || !frames || ntracks < 1 || !table || !row_frames || !out_row_cap || !src_total || !dst_total) return RR_INVPARAM;
  try {
    rsmp::ChainPlan plan;
    int rc = rsmp::make_plan(to_config(config), plan);
    if (rc) return rc;
    size_t src = 0, dst = 0, row = 0;
    for (int t = 0; t < ntracks; ++t) // (before any track is walked: a refusal costs nothing)
      if (frames[t] > kTrackFramesMax || (src += frames[t]) < frames[t]) return RR_INVPARAM;
    src = 0;
    for (int t = 0; t < ntracks; ++t) {
      size_t lead = 0, ext = 0, out_first = 0, out_frames = 0;
      if (t > 0 && frames[t] == frames[t - 1]) { // equal neighbours (the zero-length tail of a batch, an album of singles): walked once
        lead = table[t - 1].lead, ext = frames[t] + 2 * lead, out_first = table[t - 1].out_first, out_frames = table[t - 1].out_frames;
      } else if ((rc = track_geometry(plan, frames[t], &lead, &ext, &out_first, &out_frames)) != RR_OK)
        return rc;
      table[t].src_first = src;
      table[t].frames = frames[t];
      table[t].lead = lead;
      table[t].out_first = out_first;
      table[t].out_frames = out_frames;
      table[t].dst_first = dst;
      src += frames[t];
      if (dst + out_frames < dst) return RR_INVPARAM;
      dst += out_frames;
      row = std::max(row, ext);
    }
    size_t cap = 0;
    if (!out_row_capacity(plan, row, &cap)) return RR_INVPARAM;
    *row_frames = row;
    *out_row_cap = cap;
    *src_total = src;
    *dst_total = dst;
    return RR_OK;
  } catch (const std::bad_alloc &) {
    return finish(RR_ENOMEM);
  } catch (...) {
    return RR_INTERNAL;
  }
}

// The library as length-sorted batches.  Sorted descending and cut every nstreams tracks, batch b's row is the ext_frames of its first
// track: RRX_tracks_plan is still asked, batch by batch, so that row_frames[b] IS its answer and its refusals are this call's.
int RRX_tracks_batches(const RR_config *config, const size_t *frames, int ntracks, int nstreams, int *order, size_t *row_frames,
                       int *nbatches, unsigned long long *resampled, unsigned long long *useful)
{
  if (!config || !frames || ntracks < 1 || nstreams < 1 || !order || !nbatches) return RR_INVPARAM;
  try {
    for (int t = 0; t < ntracks; ++t) order[t] = t;
    std::stable_sort(order, order + ntracks, [&](int a, int b) { return frames[a] > frames[b]; });
    std::vector<size_t> sorted(size_t(ntracks), 0);
    for (int t = 0; t < ntracks; ++t) sorted[size_t(t)] = frames[order[t]];
    { // the whole library first: the refusals that depend on every track (sums that overflow) are those of one RRX_tracks_plan
      size_t sum = 0;
      for (int t = 0; t < ntracks; ++t)
        if (frames[t] > kTrackFramesMax || (sum += frames[t]) < frames[t]) return RR_INVPARAM;
    }
    const int nb = (ntracks - 1) / nstreams + 1;
    std::vector<RRX_track> table(size_t(std::min(ntracks, nstreams)));
    unsigned long long res = 0, use = 0;
    for (int b = 0; b < nb; ++b) {
      const int t0 = b * nstreams, n = std::min(nstreams, ntracks - t0);
      size_t row = 0, cap = 0, src = 0, dst = 0;
      const int rc = RRX_tracks_plan(config, sorted.data() + t0, n, table.data(), &row, &cap, &src, &dst);
      if (rc != RR_OK) return rc;
      if (row_frames) row_frames[b] = row;
      const unsigned long long add = (unsigned long long)nstreams * row;
      if (row && add / row != (unsigned long long)nstreams) return RR_INVPARAM;
      if (res + add < res) return RR_INVPARAM;
      res += add;
      for (int t = 0; t < n; ++t) {
        const unsigned long long ext = table[size_t(t)].frames + 2 * table[size_t(t)].lead; // (below 2^37)
        if (use + ext < use) return RR_INVPARAM;
        use += ext;
      }
    }
    *nbatches = nb;
    if (resampled) *resampled = res;
    if (useful) *useful = use;
    return RR_OK;
  } catch (const std::bad_alloc &) {
    return finish(RR_ENOMEM);
  } catch (...) {
    return RR_INTERNAL;
  }
}

namespace {

// the device argument of a handle-free device call, checked as RRX_lpc_extrapolate_device checks it: RR_OK, or what the call returns
int check_device(int device)
{
  if (device >= 0) { // as RRX_open_batch_on
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) return RR_EXTUNINIT;
    if (device >= n) return RR_INVPARAM;
  }
  return rsmp::device_is_gfx950(device) ? RR_OK : RR_EXTUNINIT;
}

} // namespace

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

} // namespace

// The stage pass of a ragged batch (tracks.hip).  Refusals first, as in RRX_lpc_extrapolate_device.
int RRX_tracks_stage_device_samples(int device, void *hip_stream, size_t in_rate, size_t out_rate, const RRX_track *d_tracks, int ntracks,
                                    int nch, int src_format, const void *d_packed, size_t src_total, fb_sample_t *d_rows, size_t row_frames)
{
  static_assert(sizeof(RRX_track) == sizeof(rsmp::Track) && sizeof(RRX_track) == 6 * sizeof(unsigned long long), "RRX_track mirrors rsmp::Track");
  const int kind = tracks_src_kind(src_format);
  if (kind < 0) return RR_INVPARAM;
  if (!d_tracks || !d_packed || !d_rows || ntracks < 1 || nch < 1 || !in_rate || !out_rate || !row_frames) return RR_INVPARAM;
  if (device < -1 || (long long)ntracks * nch > 0x3fffffffLL) return RR_INVPARAM; // (two workgroups per channel of every track)
  // no buffer has 2^60 samples: with that no offset the kernels compute can wrap
  const size_t most = (~size_t(0) >> 4) / size_t(nch);
  if (src_total > most || row_frames > most / size_t(ntracks)) return RR_INVPARAM;
  size_t n_add = 0, n_drop = 0, prime = 0, inbuf = 0;
  if (RRX_edge_geometry(in_rate, out_rate, &n_add, &n_drop, &prime, &inbuf) != RR_OK || prime > size_t(rsmp::kLpcLdsFrames)) return RR_INVPARAM;
  if (!g_initialized) return RR_EXTUNINIT;
  const int rc = check_device(device);
  if (rc != RR_OK) return rc;
  rsmp::DeviceScope on(device); // restores the caller's device on return
  if (!on.ok()) return RR_INTERNAL;
  rsmp::TracksStageArgs a;
  a.tracks = reinterpret_cast<const rsmp::Track *>(d_tracks);
  a.src = d_packed;
  a.rows = d_rows;
  a.src_total = src_total;
  a.row_frames = row_frames;
  a.ntracks = ntracks;
  a.nch = nch;
  a.prime_len = int(prime);
  a.src_kind = kind;
  return rsmp::launch_tracks_stage(static_cast<hipStream_t>(hip_stream), a) == hipSuccess ? RR_OK : RR_INTERNAL;
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

// The output stage of a ragged batch (tracks.hip).  Refusals first, as in RRX_finish_device.
int RRX_tracks_finish_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch, int src_format,
                             const void *d_rows, size_t row_frames, int dst_format, void *d_dst, size_t dst_total, const double *d_gain,
                             int dither, unsigned long long seed, double *d_peak, unsigned long long *d_clipped)
{
  if (!d_tracks || !d_rows || ntracks < 1 || nch < 1) return RR_INVPARAM;
  if (src_format != RRX_FMT_FLOAT && src_format != RRX_FMT_DOUBLE) return RR_INVPARAM;
  if (d_dst && dst_format != RRX_FMT_S16 && dst_format != RRX_FMT_S24_3 && dst_format != RRX_FMT_S32) return RR_INVPARAM;
  if (!d_dst && !d_peak && !d_clipped) return RR_INVPARAM;
  const size_t most = (~size_t(0) >> 4) / size_t(nch); // no buffer has 2^60 samples (RRX_finish_device)
  if (row_frames > most / size_t(ntracks) || (d_dst && dst_total > most)) return RR_INVPARAM;
  if (device < -1) return RR_INVPARAM;
  if (!g_initialized) return RR_EXTUNINIT;
  if (!row_frames) return RR_OK;
  const int rc = check_device(device);
  if (rc != RR_OK) return rc;
  rsmp::DeviceScope on(device); // restores the caller's device on return
  if (!on.ok()) return RR_INTERNAL;
  rsmp::TracksFinishArgs a;
  a.tracks = reinterpret_cast<const rsmp::Track *>(d_tracks);
  a.src = d_rows;
  a.dst = d_dst;
  a.gain = d_gain;
  a.peak = d_peak;
  a.clipped = d_clipped;
  a.row_frames = row_frames;
  a.dst_total = dst_total;
  a.seed = seed;
  a.ntracks = ntracks;
  a.nch = nch;
  a.src_double = src_format == RRX_FMT_DOUBLE;
  a.bits = !d_dst ? 31 : dst_format == RRX_FMT_S16 ? 15 : dst_format == RRX_FMT_S24_3 ? 23 : 31; // measure only: the S32 grid
  a.dither = dither != 0;
  return rsmp::launch_tracks_finish(static_cast<hipStream_t>(hip_stream), a) == hipSuccess ? RR_OK : RR_INTERNAL;
}

namespace {

bool pcm_format(int f) { return f == RRX_FMT_S16 || f == RRX_FMT_S24_3 || f == RRX_FMT_S32; }
int pcm_bits(int f) { return f == RRX_FMT_S16 ? 15 : f == RRX_FMT_S24_3 ? 23 : 31; }

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
  if (state_in && state_out) { // [nstreams * nch][16] doubles each, nstreams * nch < 2^60 / frames: no wrap for a buffer that exists
    const uintptr_t x = reinterpret_cast<uintptr_t>(state_in), y = reinterpret_cast<uintptr_t>(state_out);
    const uintptr_t bytes = uintptr_t(nstreams) * uintptr_t(nch) * rsmp::kShapeMaxOrder * sizeof(double);
    if (x < y ? y - x < bytes : x - y < bytes) return RR_INVPARAM;
  }
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

// The output stage with noise-shaped dither (finish_shaped.hip).  Refusals first, as in RRX_finish_device.
int RRX_finish_shaped_device(int device, void *hip_stream, int src_format, const void *d_src, size_t src_stride, int dst_format, void *d_dst,
                             size_t dst_stride, int nstreams, size_t frames, int nch, const double *d_gain, int dither, unsigned long long seed,
                             unsigned long long first_frame, const double *coefs, int order, size_t segment, const double *d_state_in,
                             double *d_state_out, double *d_peak, unsigned long long *d_clipped)
{
  rsmp::ShapedArgs a;
  const int rc = finish_shaped_args(src_format, d_src, src_stride, dst_format, d_dst, dst_stride, nstreams, frames, nch, d_gain, dither, seed,
                                    first_frame, coefs, order, segment, d_state_in, d_state_out, d_peak, d_clipped, a);
  if (rc != RR_OK) return rc;
  if (device < -1) return RR_INVPARAM;
  if (!g_initialized) return RR_EXTUNINIT;
  if (!frames) return RR_OK;
  const int dev = check_device(device);
  if (dev != RR_OK) return dev;
  rsmp::DeviceScope on(device); // restores the caller's device on return
  if (!on.ok()) return RR_INTERNAL;
  return rsmp::launch_finish_shaped(static_cast<hipStream_t>(hip_stream), a) == hipSuccess ? RR_OK : RR_INTERNAL;
}

int RRX_debug_finish_shaped_host(int src_format, const void *src, size_t src_stride, int dst_format, void *dst, size_t dst_stride, int nstreams,
                                 size_t frames, int nch, const double *gain, int dither, unsigned long long seed,
                                 unsigned long long first_frame, const double *coefs, int order, size_t segment, const double *state_in,
                                 double *state_out, double *peak, unsigned long long *clipped)
{
  if (!rsmp::knobs().test_hooks) return -1;
  rsmp::ShapedArgs a;
  const int rc = finish_shaped_args(src_format, src, src_stride, dst_format, dst, dst_stride, nstreams, frames, nch, gain, dither, seed,
                                    first_frame, coefs, order, segment, state_in, state_out, peak, clipped, a);
  if (rc != RR_OK) return rc;
  if (frames) rsmp::finish_shaped_host(a);
  return RR_OK;
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
  if (state_in && state_out) { // [nstreams * nch][16] doubles each (finish_shaped_args)
    const uintptr_t x = reinterpret_cast<uintptr_t>(state_in), y = reinterpret_cast<uintptr_t>(state_out);
    const uintptr_t bytes = uintptr_t(nstreams) * uintptr_t(nch) * rsmp::kTpMaxTaps * sizeof(double);
    if (x < y ? y - x < bytes : x - y < bytes) return RR_INVPARAM;
  }
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

} // namespace

// True peak and sample peak of device-resident frames (true_peak.hip).  Refusals first, as in RRX_finish_device.
int RRX_true_peak_device(int device, void *hip_stream, int src_format, const void *d_src, size_t src_stride, int nstreams, size_t frames,
                         int nch, const double *d_gain, unsigned long long first_frame, const double *coefs, int phases, int taps, int flush,
                         const double *d_state_in, double *d_state_out, double *d_true_peak, double *d_peak)
{
  rsmp::TruePeakArgs a;
  const int rc = true_peak_args(src_format, d_src, src_stride, nstreams, frames, nch, d_gain, first_frame, coefs, phases, taps, flush,
                                d_state_in, d_state_out, d_true_peak, d_peak, a);
  if (rc != RR_OK) return rc;
  if (device < -1) return RR_INVPARAM;
  if (!g_initialized) return RR_EXTUNINIT;
  if (!frames) return RR_OK;
  const int dev = check_device(device);
  if (dev != RR_OK) return dev;
  rsmp::DeviceScope on(device); // restores the caller's device on return
  if (!on.ok()) return RR_INTERNAL;
  return rsmp::launch_true_peak(static_cast<hipStream_t>(hip_stream), a) == hipSuccess ? RR_OK : RR_INTERNAL;
}

int RRX_debug_true_peak_host(int src_format, const void *src, size_t src_stride, int nstreams, size_t frames, int nch, const double *gain,
                             unsigned long long first_frame, const double *coefs, int phases, int taps, int flush, const double *state_in,
                             double *state_out, double *true_peak, double *peak)
{
  if (!rsmp::knobs().test_hooks) return -1;
  rsmp::TruePeakArgs a;
  const int rc = true_peak_args(src_format, src, src_stride, nstreams, frames, nch, gain, first_frame, coefs, phases, taps, flush, state_in,
                                state_out, true_peak, peak, a);
  if (rc != RR_OK) return rc;
  if (frames) rsmp::true_peak_host(a);
  return RR_OK;
}

// RRX_true_peak_device per track of a ragged batch (true_peak.hip).  Refusals first, as in RRX_tracks_finish_device.
int RRX_tracks_true_peak_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch, int src_format,
                                const void *d_rows, size_t row_frames, const double *d_gain, const double *coefs, int phases, int taps,
                                double *d_true_peak, double *d_peak)
{
  rsmp::TruePeakArgs a;
  if (!d_tracks || !d_rows || ntracks < 1 || nch < 1) return RR_INVPARAM;
  if (src_format != RRX_FMT_FLOAT && src_format != RRX_FMT_DOUBLE) return RR_INVPARAM;
  if (!d_true_peak && !d_peak) return RR_INVPARAM;
  const int rc = true_peak_filter(coefs, phases, taps, a.f);
  if (rc != RR_OK) return rc;
  const size_t most = (~size_t(0) >> 4) / size_t(nch); // no buffer has 2^60 samples (RRX_finish_device)
  if (row_frames > most / size_t(ntracks)) return RR_INVPARAM;
  if (device < -1) return RR_INVPARAM;
  if (!g_initialized) return RR_EXTUNINIT;
  if (!row_frames) return RR_OK;
  const int dev = check_device(device);
  if (dev != RR_OK) return dev;
  rsmp::DeviceScope on(device); // restores the caller's device on return
  if (!on.ok()) return RR_INTERNAL;
  a.src = d_rows;
  a.gain = d_gain;
  a.state_in = nullptr;
  a.state_out = nullptr;
  a.true_peak = d_true_peak;
  a.peak = d_peak;
  a.tracks = reinterpret_cast<const rsmp::Track *>(d_tracks);
  a.src_stride = 0;
  a.frames = row_frames;
  a.nstreams = ntracks;
  a.nch = nch;
  a.src_double = src_format == RRX_FMT_DOUBLE;
  a.flush = 1;
  return rsmp::launch_true_peak(static_cast<hipStream_t>(hip_stream), a) == hipSuccess ? RR_OK : RR_INTERNAL;
}

namespace {

// RRX_tracks_true_peak_packed_device / RRX_debug_tracks_true_peak_packed_host: everything that can be refused from the arguments
// alone; `kind` is the source's rsmp::TracksSrc
int true_peak_packed_args(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *packed, size_t src_total, size_t max_frames,
                          const double *gain, const double *coefs, int phases, int taps, double *true_peak, double *peak,
                          rsmp::TruePeakArgs &a, int &kind)
{
  if (!tracks || !packed || ntracks < 1 || nch < 1) return RR_INVPARAM;
  kind = tracks_src_kind(src_format);
  if (kind < 0) return RR_INVPARAM;
  if (!true_peak && !peak) return RR_INVPARAM;
  const int rc = true_peak_filter(coefs, phases, taps, a.f);
  if (rc != RR_OK) return rc;
  const size_t most = (~size_t(0) >> 4) / size_t(nch); // no buffer has 2^60 samples (RRX_finish_device)
  if (src_total > most || max_frames > most / size_t(ntracks)) return RR_INVPARAM;
  a.src = packed;
  a.gain = gain;
  a.state_in = nullptr;
  a.state_out = nullptr;
  a.true_peak = true_peak;
  a.peak = peak;
  a.tracks = reinterpret_cast<const rsmp::Track *>(tracks);
  a.src_stride = src_total;
  a.frames = max_frames;
  a.nstreams = ntracks;
  a.nch = nch;
  a.src_double = 0;
  a.flush = 1;
  return RR_OK;
}

} // namespace

// True peak and sample peak of tracks at rest in a packed source (true_peak.hip).  Refusals first, as in RRX_tracks_true_peak_device.
int RRX_tracks_true_peak_packed_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch, int src_format,
                                       const void *d_packed, size_t src_total, size_t max_frames, const double *d_gain, const double *coefs,
                                       int phases, int taps, double *d_true_peak, double *d_peak)
{
  rsmp::TruePeakArgs a;
  int kind = 0;
  const int rc = true_peak_packed_args(d_tracks, ntracks, nch, src_format, d_packed, src_total, max_frames, d_gain, coefs, phases, taps,
                                       d_true_peak, d_peak, a, kind);
  if (rc != RR_OK) return rc;
  if (device < -1) return RR_INVPARAM;
  if (!g_initialized) return RR_EXTUNINIT;
  if (!max_frames || !src_total) return RR_OK;
  const int dev = check_device(device);
  if (dev != RR_OK) return dev;
  rsmp::DeviceScope on(device); // restores the caller's device on return
  if (!on.ok()) return RR_INTERNAL;
  return rsmp::launch_true_peak_packed(static_cast<hipStream_t>(hip_stream), a, kind) == hipSuccess ? RR_OK : RR_INTERNAL;
}

int RRX_debug_tracks_true_peak_packed_host(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *packed, size_t src_total,
                                           size_t max_frames, const double *gain, const double *coefs, int phases, int taps,
                                           double *true_peak, double *peak)
{
  if (!rsmp::knobs().test_hooks) return -1;
  rsmp::TruePeakArgs a;
  int kind = 0;
  const int rc = true_peak_packed_args(tracks, ntracks, nch, src_format, packed, src_total, max_frames, gain, coefs, phases, taps, true_peak,
                                       peak, a, kind);
  if (rc != RR_OK) return rc;
  if (max_frames && src_total) rsmp::true_peak_packed_host(a, kind);
  return RR_OK;
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
  if (dst_format != RRX_FMT_FLOAT && dst_format != RRX_FMT_DOUBLE) return RR_INVPARAM;
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
  const size_t most = (~size_t(0) >> 4) / size_t(nch);
  if (nstreams > 1 && (dst_stride < frames || dst_stride > most / size_t(nstreams))) return RR_INVPARAM;
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

} // namespace

// The true-peak limiter on device-resident frames (limit.hip).  Refusals first, as in RRX_true_peak_device.
int RRX_limit_device(int device, void *hip_stream, int src_format, const void *d_src, size_t src_stride, int dst_format, void *d_dst,
                     size_t dst_stride, int nstreams, size_t frames, int nch, const double *d_gain, double ceiling, const double *coefs,
                     int phases, int taps, size_t lookahead, size_t hold, double *d_reduction, unsigned long long *d_limited, double *d_work,
                     size_t work_doubles)
{
  rsmp::LimitArgs a;
  const int rc = limit_args(src_format, d_src, src_stride, dst_format, d_dst, dst_stride, nstreams, frames, nch, d_gain, ceiling, coefs, phases,
                            taps, lookahead, hold, d_reduction, d_limited, d_work, work_doubles, a);
  if (rc != RR_OK) return rc;
  if (device < -1) return RR_INVPARAM;
  if (!g_initialized) return RR_EXTUNINIT;
  if (!frames) return RR_OK;
  const int dev = check_device(device);
  if (dev != RR_OK) return dev;
  rsmp::DeviceScope on(device); // restores the caller's device on return
  if (!on.ok()) return RR_INTERNAL;
  return rsmp::launch_limit(static_cast<hipStream_t>(hip_stream), a) == hipSuccess ? RR_OK : RR_INTERNAL;
}

int RRX_debug_limit_host(int src_format, const void *src, size_t src_stride, int dst_format, void *dst, size_t dst_stride, int nstreams,
                         size_t frames, int nch, const double *gain, double ceiling, const double *coefs, int phases, int taps,
                         size_t lookahead, size_t hold, double *reduction, unsigned long long *limited, double *work, size_t work_doubles)
{
  if (!rsmp::knobs().test_hooks) return -1;
  rsmp::LimitArgs a;
  const int rc = limit_args(src_format, src, src_stride, dst_format, dst, dst_stride, nstreams, frames, nch, gain, ceiling, coefs, phases, taps,
                            lookahead, hold, reduction, limited, work, work_doubles, a);
  if (rc != RR_OK) return rc;
  if (frames) rsmp::limit_host(a);
  return RR_OK;
}

// RRX_limit_device per track of a ragged batch (limit.hip).  Refusals first, as in RRX_tracks_true_peak_device.
int RRX_tracks_limit_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch, int src_format, const void *d_rows,
                            int dst_format, void *d_dst_rows, size_t row_frames, const double *d_gain, double ceiling, const double *coefs,
                            int phases, int taps, size_t lookahead, size_t hold, double *d_reduction, unsigned long long *d_limited,
                            double *d_work, size_t work_doubles)
{
  rsmp::LimitArgs a;
  if (!d_tracks || !d_rows || !d_dst_rows || ntracks < 1 || nch < 1) return RR_INVPARAM;
  if (src_format != RRX_FMT_FLOAT && src_format != RRX_FMT_DOUBLE) return RR_INVPARAM;
  int rc = true_peak_filter(coefs, phases, taps, a.f);
  if (rc != RR_OK) return rc;
  const size_t most = (~size_t(0) >> 4) / size_t(nch); // no buffer has 2^60 samples (RRX_finish_device)
  if (row_frames > most / size_t(ntracks)) return RR_INVPARAM;
  rc = limit_common(src_format, dst_format, ntracks, row_frames, ceiling, lookahead, hold, d_work, work_doubles, a);
  if (rc != RR_OK) return rc;
  const uintptr_t samples = uintptr_t(ntracks) * row_frames * uintptr_t(nch);
  if (!limit_overlap_ok(d_rows, samples * (a.src_double ? 8 : 4), d_dst_rows, samples * (a.dst_double ? 8 : 4), src_format == dst_format))
    return RR_INVPARAM;
  if (device < -1) return RR_INVPARAM;
  if (!g_initialized) return RR_EXTUNINIT;
  if (!row_frames) return RR_OK;
  const int dev = check_device(device);
  if (dev != RR_OK) return dev;
  rsmp::DeviceScope on(device); // restores the caller's device on return
  if (!on.ok()) return RR_INTERNAL;
  a.src = d_rows;
  a.dst = d_dst_rows;
  a.gain = d_gain;
  a.reduction = d_reduction;
  a.limited = d_limited;
  a.tracks = reinterpret_cast<const rsmp::Track *>(d_tracks);
  a.src_stride = a.dst_stride = 0;
  a.frames = row_frames;
  a.nstreams = ntracks;
  a.nch = nch;
  return rsmp::launch_limit(static_cast<hipStream_t>(hip_stream), a) == hipSuccess ? RR_OK : RR_INTERNAL;
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

// RRX_limit_device with an exponential release between the window minimum and the box (limit_release.hip).  Refusals first.
int RRX_limit_release_device(int device, void *hip_stream, int src_format, const void *d_src, size_t src_stride, int dst_format, void *d_dst,
                             size_t dst_stride, int nstreams, size_t frames, int nch, const double *d_gain, double ceiling, const double *coefs,
                             int phases, int taps, size_t lookahead, size_t hold, double release, size_t block, double *d_reduction,
                             unsigned long long *d_limited, double *d_work, size_t work_doubles)
{
  rsmp::LimitArgs a;
  rsmp::LimitReleaseArgs r;
  // (limit_args wants RRX_limit_work_doubles of work, which the release's buffer always holds)
  int rc = limit_args(src_format, d_src, src_stride, dst_format, d_dst, dst_stride, nstreams, frames, nch, d_gain, ceiling, coefs, phases, taps,
                      lookahead, hold, d_reduction, d_limited, d_work, ~size_t(0), a);
  if (rc != RR_OK) return rc;
  rc = limit_release_args(release, block, d_work, work_doubles, a, r);
  if (rc != RR_OK) return rc;
  if (device < -1) return RR_INVPARAM;
  if (!g_initialized) return RR_EXTUNINIT;
  if (!frames) return RR_OK;
  const int dev = check_device(device);
  if (dev != RR_OK) return dev;
  rsmp::DeviceScope on(device); // restores the caller's device on return
  if (!on.ok()) return RR_INTERNAL;
  return rsmp::launch_limit_release(static_cast<hipStream_t>(hip_stream), a, r) == hipSuccess ? RR_OK : RR_INTERNAL;
}

int RRX_debug_limit_release_host(int src_format, const void *src, size_t src_stride, int dst_format, void *dst, size_t dst_stride, int nstreams,
                                 size_t frames, int nch, const double *gain, double ceiling, const double *coefs, int phases, int taps,
                                 size_t lookahead, size_t hold, double release, size_t block, double *reduction, unsigned long long *limited,
                                 double *work, size_t work_doubles)
{
  if (!rsmp::knobs().test_hooks) return -1;
  rsmp::LimitArgs a;
  rsmp::LimitReleaseArgs r;
  int rc = limit_args(src_format, src, src_stride, dst_format, dst, dst_stride, nstreams, frames, nch, gain, ceiling, coefs, phases, taps,
                      lookahead, hold, reduction, limited, work, ~size_t(0), a);
  if (rc != RR_OK) return rc;
  rc = limit_release_args(release, block, work, work_doubles, a, r);
  if (rc != RR_OK) return rc;
  if (frames) rsmp::limit_release_host(a, r);
  return RR_OK;
}

// RRX_limit_release_device per track of a ragged batch (limit_release.hip).  Refusals first, as in RRX_tracks_limit_device.
int RRX_tracks_limit_release_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch, int src_format,
                                    const void *d_rows, int dst_format, void *d_dst_rows, size_t row_frames, const double *d_gain, double ceiling,
                                    const double *coefs, int phases, int taps, size_t lookahead, size_t hold, double release, size_t block,
                                    double *d_reduction, unsigned long long *d_limited, double *d_work, size_t work_doubles)
{
  rsmp::LimitArgs a;
  rsmp::LimitReleaseArgs r;
  if (!d_tracks || !d_rows || !d_dst_rows || ntracks < 1 || nch < 1) return RR_INVPARAM;
  if (src_format != RRX_FMT_FLOAT && src_format != RRX_FMT_DOUBLE) return RR_INVPARAM;
  int rc = true_peak_filter(coefs, phases, taps, a.f);
  if (rc != RR_OK) return rc;
  const size_t most = (~size_t(0) >> 4) / size_t(nch); // no buffer has 2^60 samples (RRX_finish_device)
  if (row_frames > most / size_t(ntracks)) return RR_INVPARAM;
  rc = limit_common(src_format, dst_format, ntracks, row_frames, ceiling, lookahead, hold, d_work, ~size_t(0), a);
  if (rc != RR_OK) return rc;
  const uintptr_t samples = uintptr_t(ntracks) * row_frames * uintptr_t(nch);
  if (!limit_overlap_ok(d_rows, samples * (a.src_double ? 8 : 4), d_dst_rows, samples * (a.dst_double ? 8 : 4), src_format == dst_format))
    return RR_INVPARAM;
  a.src = d_rows;
  a.dst = d_dst_rows;
  a.gain = d_gain;
  a.reduction = d_reduction;
  a.limited = d_limited;
  a.tracks = reinterpret_cast<const rsmp::Track *>(d_tracks);
  a.src_stride = a.dst_stride = 0;
  a.frames = row_frames;
  a.nstreams = ntracks;
  a.nch = nch;
  rc = limit_release_args(release, block, d_work, work_doubles, a, r);
  if (rc != RR_OK) return rc;
  if (device < -1) return RR_INVPARAM;
  if (!g_initialized) return RR_EXTUNINIT;
  if (!row_frames) return RR_OK;
  const int dev = check_device(device);
  if (dev != RR_OK) return dev;
  rsmp::DeviceScope on(device); // restores the caller's device on return
  if (!on.ok()) return RR_INTERNAL;
  return rsmp::launch_limit_release(static_cast<hipStream_t>(hip_stream), a, r) == hipSuccess ? RR_OK : RR_INTERNAL;
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
  if (state_in && state_out) {                      // [nstreams * nch][4] doubles each (finish_shaped_args)
    const uintptr_t x = reinterpret_cast<uintptr_t>(state_in), y = reinterpret_cast<uintptr_t>(state_out);
    const uintptr_t bytes = uintptr_t(nstreams) * uintptr_t(nch) * 4 * sizeof(double);
    if (x < y ? y - x < bytes : x - y < bytes) return RR_INVPARAM;
  }
  const unsigned long long n = frames / hop, first_hop = first_frame / hop;
  if (first_hop + n > energy_stride) return RR_INVPARAM;                            // (first_frame + frames does not wrap: nor does this)
  if (energy_stride > (~size_t(0) >> 4) / size_t(nch) / size_t(nstreams)) return RR_INVPARAM; // no buffer has 2^60 doubles
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

// RRX_loudness_gate_device / RRX_debug_loudness_gate_host
int loudness_gate_args(const double *energy, size_t energy_stride, int nstreams, int nch, size_t nhops, const unsigned long long *hops,
                       const double *weights, size_t hop, double abs_threshold, double rel_factor, double *result, rsmp::LoudnessGateArgs &a)
{
  if (!energy || !result || nstreams < 1 || nch < 1 || !hop || nhops > energy_stride) return RR_INVPARAM;
  if (std::isnan(abs_threshold) || std::isnan(rel_factor)) return RR_INVPARAM;
  if (energy_stride > (~size_t(0) >> 4) / size_t(nch) / size_t(nstreams)) return RR_INVPARAM; // no buffer has 2^60 doubles
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

// K-weighted hop energies of device-resident frames (loudness.hip).  Refusals first, as in RRX_finish_device.
int RRX_loudness_device(int device, void *hip_stream, int src_format, const void *d_src, size_t src_stride, int nstreams, size_t frames,
                        int nch, const double *d_gain, unsigned long long first_frame, const double *coefs, size_t hop,
                        const double *d_state_in, double *d_state_out, double *d_energy, size_t energy_stride, double *d_work,
                        size_t work_doubles)
{
  rsmp::LoudnessArgs a;
  const int rc = loudness_args(src_format, d_src, src_stride, nstreams, frames, nch, d_gain, first_frame, coefs, hop, d_state_in, d_state_out,
                               d_energy, energy_stride, d_work, work_doubles, a);
  if (rc != RR_OK) return rc;
  if (device < -1) return RR_INVPARAM;
  if (!g_initialized) return RR_EXTUNINIT;
  if (!frames) return RR_OK;
  const int dev = check_device(device);
  if (dev != RR_OK) return dev;
  rsmp::DeviceScope on(device); // restores the caller's device on return
  if (!on.ok()) return RR_INTERNAL;
  return rsmp::launch_loudness(static_cast<hipStream_t>(hip_stream), a) == hipSuccess ? RR_OK : RR_INTERNAL;
}

int RRX_debug_loudness_host(int src_format, const void *src, size_t src_stride, int nstreams, size_t frames, int nch, const double *gain,
                            unsigned long long first_frame, const double *coefs, size_t hop, const double *state_in, double *state_out,
                            double *energy, size_t energy_stride, double *work, size_t work_doubles)
{
  if (!rsmp::knobs().test_hooks) return -1;
  rsmp::LoudnessArgs a;
  const int rc = loudness_args(src_format, src, src_stride, nstreams, frames, nch, gain, first_frame, coefs, hop, state_in, state_out, energy,
                               energy_stride, work, work_doubles, a);
  if (rc != RR_OK) return rc;
  if (frames) rsmp::loudness_host(a);
  return RR_OK;
}

// RRX_loudness_device per track of a ragged batch (loudness.hip).  Refusals first, as in RRX_tracks_true_peak_device.
int RRX_tracks_loudness_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch, int src_format,
                               const void *d_rows, size_t row_frames, const double *d_gain, const double *coefs, size_t hop, double *d_energy,
                               size_t energy_stride, unsigned long long *d_hops, double *d_work, size_t work_doubles)
{
  rsmp::LoudnessArgs a;
  if (!d_tracks || !d_rows || ntracks < 1 || nch < 1 || !d_energy || !d_hops) return RR_INVPARAM;
  if (src_format != RRX_FMT_FLOAT && src_format != RRX_FMT_DOUBLE) return RR_INVPARAM;
  const int rc = loudness_filter(coefs, hop, a);
  if (rc != RR_OK) return rc;
  const size_t most = (~size_t(0) >> 4) / size_t(nch); // no buffer has 2^60 samples (RRX_finish_device)
  if (row_frames > most / size_t(ntracks) || energy_stride > most / size_t(ntracks)) return RR_INVPARAM;
  const unsigned long long need = rsmp::loudness_work_doubles(ntracks, nch, row_frames, hop);
  if (work_doubles < need || (need && !d_work)) return RR_INVPARAM;
  if (device < -1) return RR_INVPARAM;
  if (!g_initialized) return RR_EXTUNINIT;
  if (!row_frames) return RR_OK;
  const int dev = check_device(device);
  if (dev != RR_OK) return dev;
  rsmp::DeviceScope on(device); // restores the caller's device on return
  if (!on.ok()) return RR_INTERNAL;
  a.src = d_rows;
  a.gain = d_gain;
  a.state_in = nullptr;
  a.state_out = nullptr;
  a.energy = d_energy;
  a.work = d_work;
  a.tracks = reinterpret_cast<const rsmp::Track *>(d_tracks);
  a.hops_out = d_hops;
  a.src_stride = 0;
  a.frames = row_frames;
  a.hop = hop;
  a.max_hops = row_frames / hop;
  a.first_hop = 0;
  a.energy_stride = energy_stride;
  a.nstreams = ntracks;
  a.nch = nch;
  a.src_double = src_format == RRX_FMT_DOUBLE;
  return rsmp::launch_loudness(static_cast<hipStream_t>(hip_stream), a) == hipSuccess ? RR_OK : RR_INTERNAL;
}

namespace {

// RRX_tracks_loudness_packed_device / RRX_debug_tracks_loudness_packed_host: everything that can be refused from the arguments
// alone; `kind` is the source's rsmp::TracksSrc
int loudness_packed_args(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *packed, size_t src_total, size_t max_frames,
                         const double *gain, const double *coefs, size_t hop, double *energy, size_t energy_stride, unsigned long long *hops,
                         double *work, size_t work_doubles, rsmp::LoudnessArgs &a, int &kind)
{
  if (!tracks || !packed || ntracks < 1 || nch < 1 || !energy || !hops) return RR_INVPARAM;
  kind = tracks_src_kind(src_format);
  if (kind < 0) return RR_INVPARAM;
  const int rc = loudness_filter(coefs, hop, a);
  if (rc != RR_OK) return rc;
  const size_t most = (~size_t(0) >> 4) / size_t(nch); // no buffer has 2^60 samples (RRX_finish_device)
  if (src_total > most || max_frames > most / size_t(ntracks) || energy_stride > most / size_t(ntracks)) return RR_INVPARAM;
  const unsigned long long need = rsmp::loudness_work_doubles(ntracks, nch, max_frames, hop);
  if (work_doubles < need || (need && !work)) return RR_INVPARAM;
  a.src = packed;
  a.gain = gain;
  a.state_in = nullptr;
  a.state_out = nullptr;
  a.energy = energy;
  a.work = work;
  a.tracks = reinterpret_cast<const rsmp::Track *>(tracks);
  a.hops_out = hops;
  a.src_stride = src_total;
  a.frames = max_frames;
  a.hop = hop;
  a.max_hops = max_frames / hop;
  a.first_hop = 0;
  a.energy_stride = energy_stride;
  a.nstreams = ntracks;
  a.nch = nch;
  a.src_double = 0;
  return RR_OK;
}

} // namespace

// K-weighted hop energies of tracks at rest in a packed source (loudness.hip).  Refusals first, as in RRX_tracks_loudness_device.
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
  if (device < -1) return RR_INVPARAM;
  if (!g_initialized) return RR_EXTUNINIT;
  if (!max_frames || !src_total) return RR_OK;
  const int dev = check_device(device);
  if (dev != RR_OK) return dev;
  rsmp::DeviceScope on(device); // restores the caller's device on return
  if (!on.ok()) return RR_INTERNAL;
  return rsmp::launch_loudness_packed(static_cast<hipStream_t>(hip_stream), a, kind) == hipSuccess ? RR_OK : RR_INTERNAL;
}

int RRX_debug_tracks_loudness_packed_host(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *packed, size_t src_total,
                                          size_t max_frames, const double *gain, const double *coefs, size_t hop, double *energy,
                                          size_t energy_stride, unsigned long long *hops, double *work, size_t work_doubles)
{
  if (!rsmp::knobs().test_hooks) return -1;
  rsmp::LoudnessArgs a;
  int kind = 0;
  const int rc = loudness_packed_args(tracks, ntracks, nch, src_format, packed, src_total, max_frames, gain, coefs, hop, energy, energy_stride,
                                      hops, work, work_doubles, a, kind);
  if (rc != RR_OK) return rc;
  if (max_frames && src_total) rsmp::loudness_packed_host(a, kind);
  return RR_OK;
}

// The two-stage gate over hop energies (loudness.hip).  Refusals first, as in RRX_finish_device.
int RRX_loudness_gate_device(int device, void *hip_stream, const double *d_energy, size_t energy_stride, int nstreams, int nch, size_t nhops,
                             const unsigned long long *d_hops, const double *d_weights, size_t hop, double abs_threshold, double rel_factor,
                             double *d_result)
{
  rsmp::LoudnessGateArgs a;
  const int rc = loudness_gate_args(d_energy, energy_stride, nstreams, nch, nhops, d_hops, d_weights, hop, abs_threshold, rel_factor, d_result, a);
  if (rc != RR_OK) return rc;
  if (device < -1) return RR_INVPARAM;
  if (!g_initialized) return RR_EXTUNINIT;
  const int dev = check_device(device);
  if (dev != RR_OK) return dev;
  rsmp::DeviceScope on(device); // restores the caller's device on return
  if (!on.ok()) return RR_INTERNAL;
  return rsmp::launch_loudness_gate(static_cast<hipStream_t>(hip_stream), a) == hipSuccess ? RR_OK : RR_INTERNAL;
}

int RRX_debug_loudness_gate_host(const double *energy, size_t energy_stride, int nstreams, int nch, size_t nhops, const unsigned long long *hops,
                                 const double *weights, size_t hop, double abs_threshold, double rel_factor, double *result)
{
  if (!rsmp::knobs().test_hooks) return -1;
  rsmp::LoudnessGateArgs a;
  const int rc = loudness_gate_args(energy, energy_stride, nstreams, nch, nhops, hops, weights, hop, abs_threshold, rel_factor, result, a);
  if (rc != RR_OK) return rc;
  rsmp::loudness_gate_host(a);
  return RR_OK;
}

namespace {

// RRX_loudness_blocks_device / RRX_debug_loudness_blocks_host: the gate's refusals and those of the block geometry
int loudness_blocks_args(const double *energy, size_t energy_stride, int nstreams, int nch, size_t nhops, const unsigned long long *hops,
                         const double *weights, size_t hop, size_t block_hops, size_t step_hops, double *blocks, size_t blocks_stride,
                         unsigned long long *nblocks, double *max, rsmp::LoudnessBlocksArgs &a)
{
  if (!energy || nstreams < 1 || nch < 1 || !hop || nhops > energy_stride) return RR_INVPARAM;
  if (energy_stride > (~size_t(0) >> 4) / size_t(nch) / size_t(nstreams)) return RR_INVPARAM; // no buffer has 2^60 doubles
  if (!block_hops || !step_hops || (!blocks && !nblocks && !max)) return RR_INVPARAM;
  if ((blocks && !blocks_stride) || blocks_stride > (~size_t(0) >> 4) / size_t(nstreams)) return RR_INVPARAM;
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
  if (blocks_stride > (~size_t(0) >> 4) / size_t(nstreams)) return RR_INVPARAM; // no buffer has 2^60 doubles
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

// Sliding block powers and their maximum (loudness_stats.hip).  Refusals first, as in RRX_finish_device.
int RRX_loudness_blocks_device(int device, void *hip_stream, const double *d_energy, size_t energy_stride, int nstreams, int nch, size_t nhops,
                               const unsigned long long *d_hops, const double *d_weights, size_t hop, size_t block_hops, size_t step_hops,
                               double *d_blocks, size_t blocks_stride, unsigned long long *d_nblocks, double *d_max)
{
  rsmp::LoudnessBlocksArgs a;
  const int rc = loudness_blocks_args(d_energy, energy_stride, nstreams, nch, nhops, d_hops, d_weights, hop, block_hops, step_hops, d_blocks,
                                      blocks_stride, d_nblocks, d_max, a);
  if (rc != RR_OK) return rc;
  if (device < -1) return RR_INVPARAM;
  if (!g_initialized) return RR_EXTUNINIT;
  const int dev = check_device(device);
  if (dev != RR_OK) return dev;
  rsmp::DeviceScope on(device); // restores the caller's device on return
  if (!on.ok()) return RR_INTERNAL;
  return rsmp::launch_loudness_blocks(static_cast<hipStream_t>(hip_stream), a) == hipSuccess ? RR_OK : RR_INTERNAL;
}

int RRX_debug_loudness_blocks_host(const double *energy, size_t energy_stride, int nstreams, int nch, size_t nhops, const unsigned long long *hops,
                                   const double *weights, size_t hop, size_t block_hops, size_t step_hops, double *blocks, size_t blocks_stride,
                                   unsigned long long *nblocks, double *max)
{
  if (!rsmp::knobs().test_hooks) return -1;
  rsmp::LoudnessBlocksArgs a;
  const int rc = loudness_blocks_args(energy, energy_stride, nstreams, nch, nhops, hops, weights, hop, block_hops, step_hops, blocks, blocks_stride,
                                      nblocks, max, a);
  if (rc != RR_OK) return rc;
  rsmp::loudness_blocks_host(a);
  return RR_OK;
}

size_t RRX_loudness_groups_work_doubles(int nstreams, int ngroups)
{
  if (nstreams < 1 || ngroups < 1) return 0;
  return size_t(rsmp::loudness_groups_work_doubles(nstreams, ngroups));
}

// The BS.1770 gate over the pooled blocks of groups of streams (loudness_stats.hip).  Refusals first, as in RRX_finish_device.
int RRX_loudness_gate_groups_device(int device, void *hip_stream, const double *d_blocks, size_t blocks_stride, int nstreams,
                                    const unsigned long long *d_nblocks, const int *d_group, int ngroups, double abs_threshold, double rel_factor,
                                    double *d_result, double *d_work, size_t work_doubles)
{
  rsmp::LoudnessGroupsArgs a;
  const int rc = loudness_groups_args(d_blocks, blocks_stride, nstreams, d_nblocks, d_group, ngroups, abs_threshold, rel_factor, false, 0, 0,
                                      d_result, d_work, work_doubles, a);
  if (rc != RR_OK) return rc;
  if (device < -1) return RR_INVPARAM;
  if (!g_initialized) return RR_EXTUNINIT;
  const int dev = check_device(device);
  if (dev != RR_OK) return dev;
  rsmp::DeviceScope on(device); // restores the caller's device on return
  if (!on.ok()) return RR_INTERNAL;
  return rsmp::launch_loudness_gate_groups(static_cast<hipStream_t>(hip_stream), a) == hipSuccess ? RR_OK : RR_INTERNAL;
}

int RRX_debug_loudness_gate_groups_host(const double *blocks, size_t blocks_stride, int nstreams, const unsigned long long *nblocks, const int *group,
                                        int ngroups, double abs_threshold, double rel_factor, double *result, double *work, size_t work_doubles)
{
  if (!rsmp::knobs().test_hooks) return -1;
  rsmp::LoudnessGroupsArgs a;
  const int rc = loudness_groups_args(blocks, blocks_stride, nstreams, nblocks, group, ngroups, abs_threshold, rel_factor, false, 0, 0, result, work,
                                      work_doubles, a);
  if (rc != RR_OK) return rc;
  rsmp::loudness_gate_groups_host(a);
  return RR_OK;
}

// Gated percentiles per group by exact selection (loudness_stats.hip).  Refusals first, as in RRX_finish_device.
int RRX_loudness_range_groups_device(int device, void *hip_stream, const double *d_blocks, size_t blocks_stride, int nstreams,
                                     const unsigned long long *d_nblocks, const int *d_group, int ngroups, double abs_threshold, double rel_factor,
                                     int pct_low, int pct_high, double *d_result, double *d_work, size_t work_doubles)
{
  rsmp::LoudnessGroupsArgs a;
  const int rc = loudness_groups_args(d_blocks, blocks_stride, nstreams, d_nblocks, d_group, ngroups, abs_threshold, rel_factor, true, pct_low,
                                      pct_high, d_result, d_work, work_doubles, a);
  if (rc != RR_OK) return rc;
  if (device < -1) return RR_INVPARAM;
  if (!g_initialized) return RR_EXTUNINIT;
  const int dev = check_device(device);
  if (dev != RR_OK) return dev;
  rsmp::DeviceScope on(device); // restores the caller's device on return
  if (!on.ok()) return RR_INTERNAL;
  return rsmp::launch_loudness_range_groups(static_cast<hipStream_t>(hip_stream), a) == hipSuccess ? RR_OK : RR_INTERNAL;
}

int RRX_debug_loudness_range_groups_host(const double *blocks, size_t blocks_stride, int nstreams, const unsigned long long *nblocks,
                                         const int *group, int ngroups, double abs_threshold, double rel_factor, int pct_low, int pct_high,
                                         double *result, double *work, size_t work_doubles)
{
  if (!rsmp::knobs().test_hooks) return -1;
  rsmp::LoudnessGroupsArgs a;
  const int rc = loudness_groups_args(blocks, blocks_stride, nstreams, nblocks, group, ngroups, abs_threshold, rel_factor, true, pct_low, pct_high,
                                      result, work, work_doubles, a);
  if (rc != RR_OK) return rc;
  rsmp::loudness_range_groups_host(a);
  return RR_OK;
}

// The shaped output stage of a ragged batch (finish_shaped.hip).  Refusals first, as in RRX_tracks_finish_device.
int RRX_tracks_finish_shaped_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch, int src_format,
                                    const void *d_rows, size_t row_frames, int dst_format, void *d_dst, size_t dst_total, const double *d_gain,
                                    int dither, unsigned long long seed, const double *coefs, int order, size_t segment, double *d_peak,
                                    unsigned long long *d_clipped)
{
  rsmp::TracksShapedArgs a;
  if (!d_tracks || !d_rows || ntracks < 1 || nch < 1) return RR_INVPARAM;
  if (src_format != RRX_FMT_FLOAT && src_format != RRX_FMT_DOUBLE) return RR_INVPARAM;
  if (!pcm_format(dst_format)) return RR_INVPARAM; // measure only included
  if (shaped_filter(coefs, order, a.coefs) != RR_OK) return RR_INVPARAM;
  if (!d_dst && !d_peak && !d_clipped) return RR_INVPARAM;
  const size_t most = (~size_t(0) >> 4) / size_t(nch); // no buffer has 2^60 samples (RRX_finish_device)
  if (row_frames > most / size_t(ntracks) || (d_dst && dst_total > most)) return RR_INVPARAM;
  if (device < -1) return RR_INVPARAM;
  if (!g_initialized) return RR_EXTUNINIT;
  if (!row_frames) return RR_OK;
  const int rc = check_device(device);
  if (rc != RR_OK) return rc;
  rsmp::DeviceScope on(device); // restores the caller's device on return
  if (!on.ok()) return RR_INTERNAL;
  a.t.tracks = reinterpret_cast<const rsmp::Track *>(d_tracks);
  a.t.src = d_rows;
  a.t.dst = d_dst;
  a.t.gain = d_gain;
  a.t.peak = d_peak;
  a.t.clipped = d_clipped;
  a.t.row_frames = row_frames;
  a.t.dst_total = dst_total;
  a.t.seed = seed;
  a.t.ntracks = ntracks;
  a.t.nch = nch;
  a.t.src_double = src_format == RRX_FMT_DOUBLE;
  a.t.bits = pcm_bits(dst_format);
  a.t.dither = dither != 0;
  a.segment = segment;
  a.order = order;
  return rsmp::launch_tracks_finish_shaped(static_cast<hipStream_t>(hip_stream), a) == hipSuccess ? RR_OK : RR_INTERNAL;
}

namespace {

// the window of a window call: RR_INVPARAM unless it lies inside the rows, fits its pitch and the window buffer is one a device can hold
int tracks_window_args(int ntracks, int nch, size_t row_frames, size_t win_first, size_t win_frames, size_t win_stride, rsmp::TracksWindow &w)
{
  if (win_first + win_frames < win_first || win_first + win_frames > row_frames || win_stride < win_frames) return RR_INVPARAM;
  if (win_stride > (~size_t(0) >> 4) / size_t(nch) / size_t(ntracks)) return RR_INVPARAM;
  w.first = win_first;
  w.frames = win_frames;
  w.stride = win_stride;
  return RR_OK;
}

} // namespace

// RRX_tracks_stage_device_samples on a window of the rows (tracks.hip).  Refusals first.
int RRX_tracks_stage_window_device(int device, void *hip_stream, size_t in_rate, size_t out_rate, const RRX_track *d_tracks, int ntracks, int nch,
                                   int src_format, const void *d_packed, size_t src_total, size_t row_frames, size_t win_first, size_t win_frames,
                                   fb_sample_t *d_win, size_t win_stride)
{
  const int kind = tracks_src_kind(src_format);
  if (kind < 0) return RR_INVPARAM;
  if (!d_tracks || !d_packed || !d_win || ntracks < 1 || nch < 1 || !in_rate || !out_rate || !row_frames) return RR_INVPARAM;
  if (device < -1 || (long long)ntracks * nch > 0x3fffffffLL) return RR_INVPARAM; // (two workgroups per channel of every track)
  const size_t most = (~size_t(0) >> 4) / size_t(nch);                            // no buffer has 2^60 samples, and no virtual row either
  if (src_total > most || row_frames > most / size_t(ntracks)) return RR_INVPARAM;
  rsmp::TracksWindow w;
  if (tracks_window_args(ntracks, nch, row_frames, win_first, win_frames, win_stride, w) != RR_OK) return RR_INVPARAM;
  size_t n_add = 0, n_drop = 0, prime = 0, inbuf = 0;
  if (RRX_edge_geometry(in_rate, out_rate, &n_add, &n_drop, &prime, &inbuf) != RR_OK || prime > size_t(rsmp::kLpcLdsFrames)) return RR_INVPARAM;
  if (!g_initialized) return RR_EXTUNINIT;
  if (!win_frames) return RR_OK;
  const int rc = check_device(device);
  if (rc != RR_OK) return rc;
  rsmp::DeviceScope on(device); // restores the caller's device on return
  if (!on.ok()) return RR_INTERNAL;
  rsmp::TracksStageArgs a;
  a.tracks = reinterpret_cast<const rsmp::Track *>(d_tracks);
  a.src = d_packed;
  a.rows = d_win;
  a.src_total = src_total;
  a.row_frames = row_frames;
  a.ntracks = ntracks;
  a.nch = nch;
  a.prime_len = int(prime);
  a.src_kind = kind;
  return rsmp::launch_tracks_stage_window(static_cast<hipStream_t>(hip_stream), a, w) == hipSuccess ? RR_OK : RR_INTERNAL;
}

// RRX_tracks_finish_device on a window of the output rows (tracks.hip).  Refusals first.
int RRX_tracks_finish_window_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch, int src_format,
                                    const void *d_win, size_t win_stride, size_t row_frames, size_t win_first, size_t win_frames, int dst_format,
                                    void *d_dst, size_t dst_total, const double *d_gain, int dither, unsigned long long seed, double *d_peak,
                                    unsigned long long *d_clipped)
{
  if (!d_tracks || !d_win || ntracks < 1 || nch < 1) return RR_INVPARAM;
  if (src_format != RRX_FMT_FLOAT && src_format != RRX_FMT_DOUBLE) return RR_INVPARAM;
  if (d_dst && dst_format != RRX_FMT_S16 && dst_format != RRX_FMT_S24_3 && dst_format != RRX_FMT_S32) return RR_INVPARAM;
  if (!d_dst && !d_peak && !d_clipped) return RR_INVPARAM;
  const size_t most = (~size_t(0) >> 4) / size_t(nch); // no buffer has 2^60 samples (RRX_finish_device)
  if (row_frames > most / size_t(ntracks) || (d_dst && dst_total > most)) return RR_INVPARAM;
  rsmp::TracksWindow w;
  if (tracks_window_args(ntracks, nch, row_frames, win_first, win_frames, win_stride, w) != RR_OK) return RR_INVPARAM;
  if (device < -1) return RR_INVPARAM;
  if (!g_initialized) return RR_EXTUNINIT;
  if (!row_frames || !win_frames) return RR_OK;
  const int rc = check_device(device);
  if (rc != RR_OK) return rc;
  rsmp::DeviceScope on(device); // restores the caller's device on return
  if (!on.ok()) return RR_INTERNAL;
  rsmp::TracksFinishArgs a;
  a.tracks = reinterpret_cast<const rsmp::Track *>(d_tracks);
  a.src = d_win;
  a.dst = d_dst;
  a.gain = d_gain;
  a.peak = d_peak;
  a.clipped = d_clipped;
  a.row_frames = row_frames;
  a.dst_total = dst_total;
  a.seed = seed;
  a.ntracks = ntracks;
  a.nch = nch;
  a.src_double = src_format == RRX_FMT_DOUBLE;
  a.bits = !d_dst ? 31 : dst_format == RRX_FMT_S16 ? 15 : dst_format == RRX_FMT_S24_3 ? 23 : 31; // measure only: the S32 grid
  a.dither = dither != 0;
  return rsmp::launch_tracks_finish_window(static_cast<hipStream_t>(hip_stream), a, w) == hipSuccess ? RR_OK : RR_INTERNAL;
}

namespace {

// RRX_tracks_finish_shaped_window_device / RRX_debug_tracks_finish_shaped_window_host: everything that can be refused from the
// arguments alone -- what RRX_tracks_finish_window_device refuses, what RRX_tracks_finish_shaped_device adds, and the state rules
int tracks_shaped_window_args(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *win, size_t win_stride, size_t row_frames,
                              size_t win_first, size_t win_frames, int dst_format, void *dst, size_t dst_total, const double *gain, int dither,
                              unsigned long long seed, const double *coefs, int order, size_t segment, const double *state_in, double *state_out,
                              double *peak, unsigned long long *clipped, rsmp::TracksShapedWindowArgs &a)
{
  if (!tracks || !win || ntracks < 1 || nch < 1) return RR_INVPARAM;
  if (src_format != RRX_FMT_FLOAT && src_format != RRX_FMT_DOUBLE) return RR_INVPARAM;
  if (!pcm_format(dst_format)) return RR_INVPARAM; // measure only included
  if (shaped_filter(coefs, order, a.s.coefs) != RR_OK) return RR_INVPARAM;
  if (!dst && !peak && !clipped) return RR_INVPARAM;
  const size_t most = (~size_t(0) >> 4) / size_t(nch); // no buffer has 2^60 samples (RRX_finish_device)
  if (row_frames > most / size_t(ntracks) || (dst && dst_total > most)) return RR_INVPARAM;
  if (tracks_window_args(ntracks, nch, row_frames, win_first, win_frames, win_stride, a.w) != RR_OK) return RR_INVPARAM;
  if (!state_in && win_first) return RR_INVPARAM; // only a window at frame 0 finds every track at its first frame or not begun
  if (state_in && state_out) { // [ntracks * nch][16] doubles each, ntracks * nch < 2^60: no wrap for a buffer that exists
    const uintptr_t x = reinterpret_cast<uintptr_t>(state_in), y = reinterpret_cast<uintptr_t>(state_out);
    const uintptr_t bytes = uintptr_t(ntracks) * uintptr_t(nch) * rsmp::kShapeMaxOrder * sizeof(double);
    if (x < y ? y - x < bytes : x - y < bytes) return RR_INVPARAM;
  }
  a.s.t.tracks = reinterpret_cast<const rsmp::Track *>(tracks);
  a.s.t.src = win;
  a.s.t.dst = dst;
  a.s.t.gain = gain;
  a.s.t.peak = peak;
  a.s.t.clipped = clipped;
  a.s.t.row_frames = row_frames;
  a.s.t.dst_total = dst_total;
  a.s.t.seed = seed;
  a.s.t.ntracks = ntracks;
  a.s.t.nch = nch;
  a.s.t.src_double = src_format == RRX_FMT_DOUBLE;
  a.s.t.bits = pcm_bits(dst_format);
  a.s.t.dither = dither != 0;
  a.s.segment = segment;
  a.s.order = order;
  a.state_in = state_in;
  a.state_out = state_out;
  return RR_OK;
}

} // namespace

// RRX_tracks_finish_shaped_device on a window of the output rows, the error history carried per track (finish_shaped.hip).
// Refusals first.
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
  if (device < -1) return RR_INVPARAM;
  if (!g_initialized) return RR_EXTUNINIT;
  if (!row_frames || !win_frames) return RR_OK;
  const int dev = check_device(device);
  if (dev != RR_OK) return dev;
  rsmp::DeviceScope on(device); // restores the caller's device on return
  if (!on.ok()) return RR_INTERNAL;
  return rsmp::launch_tracks_finish_shaped_window(static_cast<hipStream_t>(hip_stream), a) == hipSuccess ? RR_OK : RR_INTERNAL;
}

int RRX_debug_tracks_finish_shaped_window_host(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *win, size_t win_stride,
                                               size_t row_frames, size_t win_first, size_t win_frames, int dst_format, void *dst,
                                               size_t dst_total, const double *gain, int dither, unsigned long long seed, const double *coefs,
                                               int order, size_t segment, const double *state_in, double *state_out, double *peak,
                                               unsigned long long *clipped)
{
  if (!rsmp::knobs().test_hooks) return -1;
  rsmp::TracksShapedWindowArgs a;
  const int rc = tracks_shaped_window_args(tracks, ntracks, nch, src_format, win, win_stride, row_frames, win_first, win_frames, dst_format, dst,
                                           dst_total, gain, dither, seed, coefs, order, segment, state_in, state_out, peak, clipped, a);
  if (rc != RR_OK) return rc;
  if (row_frames && win_frames) rsmp::tracks_finish_shaped_window_host(a);
  return RR_OK;
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

// the two state rules of the measuring window calls: no state only for a window at frame 0, and two buffers of `doubles` doubles
// that do not overlap (equal pointers count)
int measure_window_state(const double *state_in, double *state_out, size_t win_first, uintptr_t doubles)
{
  if (!state_in && win_first) return RR_INVPARAM; // only a window at frame 0 finds every track at its first frame or not begun
  if (state_in && state_out) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(state_in), y = reinterpret_cast<uintptr_t>(state_out);
    const uintptr_t bytes = doubles * sizeof(double); // ntracks * nch < 2^60: no wrap for a buffer that exists
    if (x < y ? y - x < bytes : x - y < bytes) return RR_INVPARAM;
  }
  return RR_OK;
}

// RRX_tracks_true_peak_window_device / RRX_debug_tracks_true_peak_window_host: everything that can be refused from the arguments
// alone -- what RRX_tracks_true_peak_device refuses, the three window refusals and the two state rules
int tracks_true_peak_window_args(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *win, size_t win_stride,
                                 size_t row_frames, size_t win_first, size_t win_frames, const double *gain, const double *coefs, int phases,
                                 int taps, const double *state_in, double *state_out, double *true_peak, double *peak,
                                 rsmp::TruePeakWindowArgs &a)
{
  if (!tracks || !win || ntracks < 1 || nch < 1) return RR_INVPARAM;
  if (src_format != RRX_FMT_FLOAT && src_format != RRX_FMT_DOUBLE) return RR_INVPARAM;
  if (!true_peak && !peak) return RR_INVPARAM;
  if (true_peak_filter(coefs, phases, taps, a.f) != RR_OK) return RR_INVPARAM;
  const size_t most = (~size_t(0) >> 4) / size_t(nch); // no buffer has 2^60 samples (RRX_finish_device)
  if (row_frames > most / size_t(ntracks)) return RR_INVPARAM;
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
  if (src_format != RRX_FMT_FLOAT && src_format != RRX_FMT_DOUBLE) return RR_INVPARAM;
  rsmp::LoudnessArgs f;
  if (loudness_filter(coefs, hop, f) != RR_OK) return RR_INVPARAM;
  const size_t most = (~size_t(0) >> 4) / size_t(nch); // no buffer has 2^60 samples (RRX_finish_device)
  if (row_frames > most / size_t(ntracks) || energy_stride > most / size_t(ntracks)) return RR_INVPARAM;
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
// Refusals first.
int RRX_tracks_true_peak_window_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch, int src_format,
                                       const void *d_win, size_t win_stride, size_t row_frames, size_t win_first, size_t win_frames,
                                       const double *d_gain, const double *coefs, int phases, int taps, const double *d_state_in,
                                       double *d_state_out, double *d_true_peak, double *d_peak)
{
  rsmp::TruePeakWindowArgs a;
  const int rc = tracks_true_peak_window_args(d_tracks, ntracks, nch, src_format, d_win, win_stride, row_frames, win_first, win_frames, d_gain,
                                              coefs, phases, taps, d_state_in, d_state_out, d_true_peak, d_peak, a);
  if (rc != RR_OK) return rc;
  if (device < -1) return RR_INVPARAM;
  if (!g_initialized) return RR_EXTUNINIT;
  if (!row_frames || !win_frames) return RR_OK;
  const int dev = check_device(device);
  if (dev != RR_OK) return dev;
  rsmp::DeviceScope on(device); // restores the caller's device on return
  if (!on.ok()) return RR_INTERNAL;
  return rsmp::launch_true_peak_window(static_cast<hipStream_t>(hip_stream), a) == hipSuccess ? RR_OK : RR_INTERNAL;
}

int RRX_debug_tracks_true_peak_window_host(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *win, size_t win_stride,
                                           size_t row_frames, size_t win_first, size_t win_frames, const double *gain, const double *coefs,
                                           int phases, int taps, const double *state_in, double *state_out, double *true_peak, double *peak)
{
  if (!rsmp::knobs().test_hooks) return -1;
  rsmp::TruePeakWindowArgs a;
  const int rc = tracks_true_peak_window_args(tracks, ntracks, nch, src_format, win, win_stride, row_frames, win_first, win_frames, gain, coefs,
                                              phases, taps, state_in, state_out, true_peak, peak, a);
  if (rc != RR_OK) return rc;
  if (row_frames && win_frames) rsmp::true_peak_window_host(a);
  return RR_OK;
}

size_t RRX_tracks_loudness_window_work_doubles(int ntracks, int nch, size_t win_frames, size_t hop)
{
  if (ntracks < 1 || nch < 1 || !hop) return 0;
  return size_t(rsmp::loudness_window_work_doubles(ntracks, nch, win_frames, hop));
}

// RRX_tracks_loudness_device on a window of the output rows, the hop in progress carried per track (measure_window.hip).
// Refusals first.
int RRX_tracks_loudness_window_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch, int src_format,
                                      const void *d_win, size_t win_stride, size_t row_frames, size_t win_first, size_t win_frames,
                                      const double *d_gain, const double *coefs, size_t hop, const double *d_state_in, double *d_state_out,
                                      double *d_energy, size_t energy_stride, unsigned long long *d_hops, double *d_work, size_t work_doubles)
{
  rsmp::LoudnessWindowArgs a;
  const int rc = tracks_loudness_window_args(d_tracks, ntracks, nch, src_format, d_win, win_stride, row_frames, win_first, win_frames, d_gain,
                                             coefs, hop, d_state_in, d_state_out, d_energy, energy_stride, d_hops, d_work, work_doubles, a);
  if (rc != RR_OK) return rc;
  if (device < -1) return RR_INVPARAM;
  if (!g_initialized) return RR_EXTUNINIT;
  if (!row_frames || !win_frames) return RR_OK;
  const int dev = check_device(device);
  if (dev != RR_OK) return dev;
  rsmp::DeviceScope on(device); // restores the caller's device on return
  if (!on.ok()) return RR_INTERNAL;
  return rsmp::launch_loudness_window(static_cast<hipStream_t>(hip_stream), a) == hipSuccess ? RR_OK : RR_INTERNAL;
}

int RRX_debug_tracks_loudness_window_host(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *win, size_t win_stride,
                                          size_t row_frames, size_t win_first, size_t win_frames, const double *gain, const double *coefs,
                                          size_t hop, const double *state_in, double *state_out, double *energy, size_t energy_stride,
                                          unsigned long long *hops, double *work, size_t work_doubles)
{
  if (!rsmp::knobs().test_hooks) return -1;
  rsmp::LoudnessWindowArgs a;
  const int rc = tracks_loudness_window_args(tracks, ntracks, nch, src_format, win, win_stride, row_frames, win_first, win_frames, gain, coefs,
                                             hop, state_in, state_out, energy, energy_stride, hops, work, work_doubles, a);
  if (rc != RR_OK) return rc;
  if (row_frames && win_frames) rsmp::loudness_window_host(a);
  return RR_OK;
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
  if (src_format != RRX_FMT_FLOAT && src_format != RRX_FMT_DOUBLE) return RR_INVPARAM;
  int rc = true_peak_filter(coefs, phases, taps, a.f);
  if (rc != RR_OK) return rc;
  const size_t most = (~size_t(0) >> 4) / size_t(nch); // no buffer has 2^60 samples (RRX_finish_device), and no virtual row either
  if (row_frames > most / size_t(ntracks) || buf_stride > most / size_t(ntracks)) return RR_INVPARAM;
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

// RRX_tracks_limit_device on a window of the rows, from a buffer that holds the window and its halo (limit.hip).  Refusals first.
int RRX_tracks_limit_window_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch, int src_format,
                                   const void *d_buf, size_t buf_stride, size_t buf_first, size_t buf_frames, size_t row_frames,
                                   size_t win_first, size_t win_frames, int dst_format, void *d_dst, size_t dst_stride, const double *d_gain,
                                   double ceiling, const double *coefs, int phases, int taps, size_t lookahead, size_t hold, double *d_reduction,
                                   unsigned long long *d_limited, double *d_work, size_t work_doubles)
{
  rsmp::LimitArgs a;
  rsmp::LimitWindow w;
  int rc = tracks_limit_window_args(d_tracks, ntracks, nch, src_format, d_buf, buf_stride, buf_first, buf_frames, row_frames, win_first,
                                    win_frames, dst_format, d_dst, dst_stride, d_gain, ceiling, coefs, phases, taps, lookahead, hold,
                                    d_reduction, d_limited, d_work, work_doubles, a, w);
  if (rc != RR_OK) return rc;
  if (device < -1) return RR_INVPARAM;
  if (!g_initialized) return RR_EXTUNINIT;
  if (!row_frames || !win_frames) return RR_OK;
  rc = check_device(device);
  if (rc != RR_OK) return rc;
  rsmp::DeviceScope on(device); // restores the caller's device on return
  if (!on.ok()) return RR_INTERNAL;
  return rsmp::launch_limit(static_cast<hipStream_t>(hip_stream), a, &w) == hipSuccess ? RR_OK : RR_INTERNAL;
}

int RRX_debug_tracks_limit_window_host(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *buf, size_t buf_stride,
                                       size_t buf_first, size_t buf_frames, size_t row_frames, size_t win_first, size_t win_frames,
                                       int dst_format, void *dst, size_t dst_stride, const double *gain, double ceiling, const double *coefs,
                                       int phases, int taps, size_t lookahead, size_t hold, double *reduction, unsigned long long *limited,
                                       double *work, size_t work_doubles)
{
  if (!rsmp::knobs().test_hooks) return -1;
  rsmp::LimitArgs a;
  rsmp::LimitWindow w;
  const int rc = tracks_limit_window_args(tracks, ntracks, nch, src_format, buf, buf_stride, buf_first, buf_frames, row_frames, win_first,
                                          win_frames, dst_format, dst, dst_stride, gain, ceiling, coefs, phases, taps, lookahead, hold,
                                          reduction, limited, work, work_doubles, a, w);
  if (rc != RR_OK) return rc;
  if (row_frames && win_frames) rsmp::limit_host(a, &w);
  return RR_OK;
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
// (limit_release_window.hip).  Refusals first.
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
  // (tracks_limit_window_args wants the window call's share of work, which the release's buffer always holds)
  int rc = tracks_limit_window_args(d_tracks, ntracks, nch, src_format, d_buf, buf_stride, buf_first, buf_frames, row_frames, win_first,
                                    win_frames, dst_format, d_dst, dst_stride, d_gain, ceiling, coefs, phases, taps, lookahead, hold,
                                    d_reduction, d_limited, d_work, ~size_t(0), a, w);
  if (rc != RR_OK) return rc;
  rc = tracks_limit_release_window_args(release, block, d_state_in, d_state_out, d_work, work_doubles, a, w, r);
  if (rc != RR_OK) return rc;
  if (device < -1) return RR_INVPARAM;
  if (!g_initialized) return RR_EXTUNINIT;
  if (!row_frames || !win_frames) return RR_OK;
  rc = check_device(device);
  if (rc != RR_OK) return rc;
  rsmp::DeviceScope on(device); // restores the caller's device on return
  if (!on.ok()) return RR_INTERNAL;
  return rsmp::launch_limit_release_window(static_cast<hipStream_t>(hip_stream), a, w, r) == hipSuccess ? RR_OK : RR_INTERNAL;
}

int RRX_debug_tracks_limit_release_window_host(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *buf, size_t buf_stride,
                                               size_t buf_first, size_t buf_frames, size_t row_frames, size_t win_first, size_t win_frames,
                                               int dst_format, void *dst, size_t dst_stride, const double *gain, double ceiling,
                                               const double *coefs, int phases, int taps, size_t lookahead, size_t hold, double release,
                                               size_t block, const double *state_in, double *state_out, double *reduction,
                                               unsigned long long *limited, double *work, size_t work_doubles)
{
  if (!rsmp::knobs().test_hooks) return -1;
  rsmp::LimitArgs a;
  rsmp::LimitWindow w;
  rsmp::LimitReleaseWindowArgs r;
  int rc = tracks_limit_window_args(tracks, ntracks, nch, src_format, buf, buf_stride, buf_first, buf_frames, row_frames, win_first,
                                    win_frames, dst_format, dst, dst_stride, gain, ceiling, coefs, phases, taps, lookahead, hold, reduction,
                                    limited, work, ~size_t(0), a, w);
  if (rc != RR_OK) return rc;
  rc = tracks_limit_release_window_args(release, block, state_in, state_out, work, work_doubles, a, w, r);
  if (rc != RR_OK) return rc;
  if (row_frames && win_frames) rsmp::limit_release_window_host(a, w, r);
  return RR_OK;
}

size_t RRX_isamp_max(const RR_handle *h) { return h ? h->eng->isamp_max() : 0; }
size_t RRX_available(const RR_handle *h) { return h ? h->eng->available() : 0; }
int RRX_channels(const RR_handle *h) { return h ? h->eng->nch() : 0; }
int RRX_streams(const RR_handle *h) { return h ? h->eng->nstreams() : 0; }

int RRX_describe_plan(const RR_config *config, char *buf, size_t cap)
{
  if (!config || !buf || !cap) return -RR_INVPARAM;
  rsmp::ChainPlan plan;
  int rc = rsmp::make_plan(to_config(config), plan);
  if (rc) return -rc;
  std::string s = plan.describe();
  size_t n = s.size() < cap - 1 ? s.size() : cap - 1;
  std::memcpy(buf, s.data(), n);
  buf[n] = 0;
  return int(n);
}

void RRX_plan_cache_clear(void) { rsmp::plan_cache_clear(); }

int RRX_plan_cache_stats(unsigned long long *hits, unsigned long long *misses, int *entries)
{
  rsmp::plan_cache_stats(hits, misses, entries);
  return RR_OK;
}

int RRX_describe_dispatch(const RR_config *config, int nchannels, char *buf, size_t cap)
{
  if (!config || !buf || !cap || nchannels < 1) return -RR_INVPARAM;
  rsmp::ChainPlan plan;
  int rc = rsmp::make_plan(to_config(config), plan);
  if (rc) return -rc;
  int nsub = 0, vs = 0;
  const bool sub = !plan.stages.empty() && rsmp::split_geometry(plan, nchannels, 0, nsub, vs);
  std::string s = "{\"sub_blocked\": ";
  s += sub ? "true" : "false";
  if (sub) {
    const rsmp::DftFilter &f = plan.dft[plan.stages[0].filt];
    const int V = f.N - (f.num_taps - 1), Pref = f.N / 2;
    const bool two = nsub == 1 && vs > rsmp::kSplitVsMax;
    char tmp[256];
    snprintf(tmp, sizeof tmp, ", \"two_round\": %s, \"nsub\": %d, \"Vs\": %d, \"V\": %d, \"taps\": %d, \"N\": %d, \"Pref\": %d, \"sub_blocks\": [",
             two ? "true" : "false", nsub, vs, V, f.num_taps, f.N, Pref);
    s += tmp;
    for (int i = 0; i < nsub; ++i) {
      const rsmp::SubBlock sb = rsmp::sub_block(i, V, vs, Pref);
      snprintf(tmp, sizeof tmp, "%s{\"off\": %d, \"len\": %d, \"win\": %d, \"shift\": %d}", i ? ", " : "", sb.off, sb.len, sb.win, sb.shift);
      s += tmp;
    }
    s += "]";
  }
  s += "}";
  size_t n = s.size() < cap - 1 ? s.size() : cap - 1;
  std::memcpy(buf, s.data(), n);
  buf[n] = 0;
  return int(n);
}

int RRX_plan_table(const RR_config *config, int which, double *out, size_t cap, size_t *count)
{
  if (!config || which < 0 || which > 2) return RR_INVPARAM;
  rsmp::ChainPlan plan;
  int rc = rsmp::make_plan(to_config(config), plan);
  if (rc) return rc;
  const std::vector<double> &t = which == 2 ? plan.poly_table : plan.dft[which].taps;
  if (count) *count = t.size();
  if (out)
    for (size_t i = 0; i < t.size() && i < cap; ++i) out[i] = t[i];
  return RR_OK;
}

} // extern "C"
