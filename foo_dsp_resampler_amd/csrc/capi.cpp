// C ABI: the reference's ratelib.h entry points (rate/rate_uni.c:27-111,210-231) plus the
// device / batch extensions of include/ratelib_amd.h that take a handle or a plan, all thin shims over rsmp::Engine.  The
// handle-free calls (output stage, tracks, meters, limiter) are in capi_stage.cpp.
#include "../../include/ratelib_amd.h"
#include "../../include/ratelib_amd_album.h"

#include "capi_common.hpp"
#include "engine.hpp"
#include "lpc.hpp"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <new>
#include <set>
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

bool rsmp::ratelib_initialized() { return g_initialized != 0; }

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

namespace {

// ceil(s * r2 / r1): the first output instant of the album's grid (multiples of r1 / r2 input frames) at or behind input frame s
size_t album_grid_ceil(size_t s, size_t r1, size_t r2) { return size_t(((unsigned __int128)s * r2 + r1 - 1) / r1); }

} // namespace

// RRX_tracks_plan with albums (include/ratelib_amd_album.h): a row of an album track starts on the album's grid of r1 input frames,
// so that the handle it is pushed to computes the album's output instants, and owns the instants inside its own frames.
int RRX_tracks_plan_album(const RR_config *config, const size_t *frames, const int *group, int ntracks, RRX_track *table, RRX_track_link *links,
                          size_t *row_frames, size_t *out_row_cap, size_t *src_total, size_t *dst_total)
{
  if (!config || !frames || !group || ntracks < 1 || !table || !links || !row_frames || !out_row_cap || !src_total || !dst_total) return RR_INVPARAM;
  try {
    rsmp::ChainPlan plan;
    int rc = rsmp::make_plan(to_config(config), plan);
    if (rc) return rc;
    size_t src = 0, dst = 0, row = 0;
    for (int t = 0; t < ntracks; ++t) // (before any track is walked: a refusal costs nothing)
      if (frames[t] > kTrackFramesMax || (src += frames[t]) < frames[t]) return RR_INVPARAM;
    {
      std::set<int> seen; // albums are consecutive: an id that comes back behind another one is refused
      for (int t = 0; t < ntracks; ++t)
        if (group[t] >= 0 && (t == 0 || group[t] != group[t - 1]) && !seen.insert(group[t]).second) return RR_INVPARAM;
    }
    size_t n_add = 0, n_drop = 0, prime = 0, inbuf = 0;
    if ((rc = RRX_edge_geometry(plan.cfg.in_rate, plan.cfg.out_rate, &n_add, &n_drop, &prime, &inbuf)) != RR_OK) return rc;
    size_t g = plan.cfg.in_rate, b = plan.cfg.out_rate;
    while (b) { const size_t c = g % b; g = b; b = c; }
    const size_t r1 = plan.cfg.in_rate / g, r2 = plan.cfg.out_rate / g;
    src = 0;
    for (int t0 = 0; t0 < ntracks;) {
      int t1 = t0 + 1;
      size_t A = frames[t0];
      if (group[t0] >= 0)
        for (; t1 < ntracks && group[t1] == group[t0]; ++t1) A += frames[t1];
      if (A > kTrackFramesMax) return RR_INVPARAM; // (the album is walked as one track)
      const bool album = group[t0] >= 0 && A > size_t(2 * rsmp::kLpcMaxOrder);
      size_t album_out = 0;
      if (album) {
        size_t lead = 0, ext = 0, out_first = 0;
        if ((rc = track_geometry(plan, A, &lead, &ext, &out_first, &album_out)) != RR_OK) return rc;
      }
      size_t S = 0; // the track's first frame, counted from the album's
      for (int t = t0; t < t1; ++t) {
        size_t lead = 0, ext = 0, out_first = 0, out_frames = 0;
        links[t].back = links[t].ahead = RRX_LINK_NONE;
        if (!album) {
          if ((rc = track_geometry(plan, frames[t], &lead, &ext, &out_first, &out_frames)) != RR_OK) return rc;
        } else {
          const size_t ph = S % r1, at = album_grid_ceil(S, r1, r2);
          lead = n_add + ph;
          ext = frames[t] + 2 * lead;
          out_first = n_drop + album_grid_ceil(ph, r1, r2);
          const size_t end = t + 1 < t1 ? album_grid_ceil(S + frames[t], r1, r2) : album_out;
          out_frames = end > at ? end - at : 0;
          if (CounterChain(plan).drained_total(ext) < out_first + out_frames) return RR_INTERNAL; // the row does not reach its own slice
          if (t > t0) links[t].back = S;
          if (t + 1 < t1) links[t].ahead = A - S - frames[t];
        }
        table[t].src_first = src;
        table[t].frames = frames[t];
        table[t].lead = lead;
        table[t].out_first = out_first;
        table[t].out_frames = out_frames;
        table[t].dst_first = dst;
        src += frames[t];
        S += frames[t];
        if (dst + out_frames < dst) return RR_INVPARAM;
        dst += out_frames;
        row = std::max(row, ext);
      }
      t0 = t1;
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
