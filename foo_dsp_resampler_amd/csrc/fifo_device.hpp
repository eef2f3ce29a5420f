// Device-side fifo accessors shared by the stage kernels (see kernels.hpp for the coordinate convention and the views).
// A FrameView's pointers are untyped; every accessor below casts them once, to the sample type of the view's kind.
#pragma once
#include "kernels.hpp"

namespace rsmp {

struct ChanRef { // per-channel precomputed addressing
  int kind; // AnyView::kind
  // frames: sample 0 of the channel in the ring / the external buffer, consecutive frames nch samples apart
  const void *fring;
  const void *fext;
  long long fmask, ext_begin, ext_end;
  int nch;
  // fp64 ring
  const double *ring64;
  long long mask64;
};

__device__ __forceinline__ ChanRef chan_ref(const AnyView &v, int c)
{
  ChanRef r;
  r.kind = v.kind;
  if (v.kind) {
    const int s = c / v.f.nch, ch = c - s * v.f.nch;
    if (v.kind == kFramesF64) { // (the same element offsets, in doubles)
      r.fring = static_cast<const double *>(v.f.ring) + s * v.f.ring_stream_stride + ch;
      r.fext = v.f.ext ? static_cast<const double *>(v.f.ext) + s * v.f.ext_stream_stride + ch : nullptr;
    } else if (v.kind == kFramesS16) { // (in shorts)
      r.fring = static_cast<const short *>(v.f.ring) + s * v.f.ring_stream_stride + ch;
      r.fext = v.f.ext ? static_cast<const short *>(v.f.ext) + s * v.f.ext_stream_stride + ch : nullptr;
    } else { // (4-byte samples: float or 32-bit PCM)
      r.fring = static_cast<const float *>(v.f.ring) + s * v.f.ring_stream_stride + ch;
      r.fext = v.f.ext ? static_cast<const float *>(v.f.ext) + s * v.f.ext_stream_stride + ch : nullptr;
    }
    r.fmask = v.f.ring_mask;
    r.ext_begin = v.f.ext_begin;
    r.ext_end = v.f.ext_end;
    r.nch = v.f.nch;
    r.ring64 = nullptr;
    r.mask64 = 0;
  } else {
    r.ring64 = v.d.ring + (long long)c * v.d.chan_stride;
    r.mask64 = v.d.mask;
    r.fring = r.fext = nullptr;
    r.fmask = r.ext_begin = r.ext_end = 0;
    r.nch = 1;
  }
  return r;
}

__device__ __forceinline__ double fifo_get(const ChanRef &r, long long a)
{
  if (r.kind == kFramesF64) {
    const double *e = static_cast<const double *>(r.fext), *g = static_cast<const double *>(r.fring);
    if (e && a >= r.ext_begin && a < r.ext_end) return e[(a - r.ext_begin) * r.nch];
    return g[(a & r.fmask) * r.nch];
  }
  if (r.kind >= kFramesS16) { // integer PCM frames: convert on load
    const bool in_ext = r.fext && a >= r.ext_begin && a < r.ext_end;
    const long long i = in_ext ? (a - r.ext_begin) * r.nch : (a & r.fmask) * r.nch;
    const void *base = in_ext ? r.fext : r.fring;
    if (r.kind == kFramesS16) return pcm_in(static_cast<const short *>(base)[i]);
    return pcm_in(static_cast<const int *>(base)[i]);
  }
  if (r.kind) {
    if (r.fext && a >= r.ext_begin && a < r.ext_end) return (double)static_cast<const float *>(r.fext)[(a - r.ext_begin) * r.nch];
    return (double)static_cast<const float *>(r.fring)[(a & r.fmask) * r.nch];
  }
  return r.ring64[a & r.mask64];
}

__device__ __forceinline__ void fifo_put(const ChanRef &r, long long a, double v)
{
  if (r.kind == kFramesF64) {
    double *e = static_cast<double *>(const_cast<void *>(r.fext)), *g = static_cast<double *>(const_cast<void *>(r.fring));
    if (e && a >= r.ext_begin && a < r.ext_end) e[(a - r.ext_begin) * r.nch] = v;
    else g[(a & r.fmask) * r.nch] = v;
  } else if (r.kind >= kFramesS16) { // integer PCM frames: quantise on store
    const bool in_ext = r.fext && a >= r.ext_begin && a < r.ext_end;
    const long long i = in_ext ? (a - r.ext_begin) * r.nch : (a & r.fmask) * r.nch;
    void *base = const_cast<void *>(in_ext ? r.fext : r.fring);
    if (r.kind == kFramesS16) static_cast<short *>(base)[i] = pcm_out16(v);
    else static_cast<int *>(base)[i] = pcm_out32(v);
  } else if (r.kind) {
    if (r.fext && a >= r.ext_begin && a < r.ext_end) static_cast<float *>(const_cast<void *>(r.fext))[(a - r.ext_begin) * r.nch] = (float)v;
    else static_cast<float *>(const_cast<void *>(r.fring))[(a & r.fmask) * r.nch] = (float)v;
  } else
    const_cast<double *>(r.ring64)[a & r.mask64] = v;
}


// `len` consecutive samples of ONE channel starting at absolute index a0, when they lie contiguously in one buffer:
// kind 1 = float32 frames (element i at p32[i * stride32]), kind 2 = the channel's fp64 ring, kind 3 = float64 frames
// (element i at p64[i * stride32]), kind 4 / 5 = 16- / 32-bit PCM frames (element i at p16 / pi32 [i * stride32], through
// get()), kind 0 = split (fifo_get).
struct ChanSpan {
  int kind;
  const float *p32;
  long long stride32;
  const double *p64;
  const short *p16;
  const int *pi32;
  __device__ __forceinline__ double geti(long long i) const // kinds 4 / 5
  {
    return kind == 4 ? pcm_in(p16[i * stride32]) : pcm_in(pi32[i * stride32]);
  }
};
__device__ __forceinline__ ChanSpan chan_span(const AnyView &v, int c, long long a0, long long len)
{
  ChanSpan r = {0, nullptr, 1, nullptr, nullptr, nullptr};
  if (v.kind) {
    const int s = c / v.f.nch, ch = c - s * v.f.nch;
    r.stride32 = v.f.nch;
    long long off = -1; // element offset from the buffer's base
    const void *base = nullptr;
    if (v.f.ext && a0 >= v.f.ext_begin && a0 + len <= v.f.ext_end) {
      base = v.f.ext;
      off = s * v.f.ext_stream_stride + (a0 - v.f.ext_begin) * v.f.nch + ch;
    } else if ((!v.f.ext || a0 + len <= v.f.ext_begin || a0 >= v.f.ext_end) && a0 >= 0 && (a0 & v.f.ring_mask) + len <= v.f.ring_mask + 1) {
      base = v.f.ring;
      off = s * v.f.ring_stream_stride + (a0 & v.f.ring_mask) * v.f.nch + ch;
    }
    if (off >= 0) {
      if (v.kind == kFramesF64) {
        r.kind = 3;
        r.p64 = static_cast<const double *>(base) + off;
      } else if (v.kind == kFramesS16) {
        r.kind = 4;
        r.p16 = static_cast<const short *>(base) + off;
      } else if (v.kind == kFramesS32) {
        r.kind = 5;
        r.pi32 = static_cast<const int *>(base) + off;
      } else {
        r.kind = 1;
        r.p32 = static_cast<const float *>(base) + off;
      }
    }
  } else if (a0 >= 0 && (a0 & v.d.mask) + len <= v.d.mask + 1) {
    r.kind = 2;
    r.p64 = v.d.ring + (long long)c * v.d.chan_stride + (a0 & v.d.mask);
  }
  return r;
}

// Channel pair -> channels.  nchs = 0: pairs run over all C channels of the handle (2p, 2p+1; the last one may be single).
// nchs > 0 (batch handles with an odd channel count per stream): pairs never straddle two streams -- every stream has
// (nchs + 1) / 2 of them and its last channel rides alone with a zero imaginary part, exactly as in a one-stream handle,
// so the bits a stream gets do not depend on its neighbours in the batch.
struct PairCh {
  int ca, cb;
  bool hasb;
};
__device__ __forceinline__ PairCh pair_channels(int pair, int C, int nchs, unsigned pps_magic)
{
  // One branch-free, division-free, wave-uniform form for both cases: with nchs = 0 the whole handle counts as one
  // "stream" of C channels.  pps_magic = ceil(2^32 / pairs per stream) (pair_magic; 0 = one pair per stream): the quotient is exact while pair * pps <= 2^32,
  // which Engine::create sees to for every pair of a handle (pair_division_exact, with the derivation and the one case that needs less).
  const int ncs = nchs > 0 ? nchs : C, pps = (ncs + 1) >> 1;
  const int strm = pps_magic ? (int)__umulhi((unsigned)pair, pps_magic) : pair /* one pair per stream */, pin = pair - strm * pps;
  PairCh r;
  r.ca = __builtin_amdgcn_readfirstlane(strm * ncs + 2 * pin);
  r.cb = r.ca + 1;
  r.hasb = __builtin_amdgcn_readfirstlane(2 * pin + 1 < ncs) != 0;
  return r;
}

// Direct addressing of `len` consecutive samples of channel pair (2*pair, 2*pair+1) starting at absolute index a0,
// when they lie contiguously in one buffer: kind 1 = float32 frames with the two channels side by side (one 8-byte
// word per sample), kind 2 = the two planar fp64 rings, kind 3 = float64 frames (one 16-byte word per sample), kind 4 = 16-bit
// PCM frames (one 4-byte word per sample), kind 5 = 32-bit PCM frames (one 8-byte word), kind 0 = not contiguous (use
// fifo_get / fifo_put).  The pair words of kinds 4 and 5 convert on load and quantise on store (pcm_in / pcm_out*).
struct PairSpan {
  int kind;
  float2 *p2;
  long long fstride; // pair words (float2; kind 3: double2, kind 4: unsigned, kind 5: int2) between consecutive frames
  double *pa, *pb;
  bool hasb;
  double2 *d2;       // kind 3 = float64 frames with the two channels side by side (one 16-byte word per sample)
  unsigned *w16;     // kind 4
  int2 *w32;         // kind 5
  // kinds 4 / 5: pair word i
  __device__ __forceinline__ void geti(long long i, double &x, double &y) const
  {
    if (kind == 4) {
      const unsigned w = w16[i * fstride];
      x = pcm_lo16(w);
      y = pcm_hi16(w);
    } else {
      const int2 w = w32[i * fstride];
      x = pcm_in(w.x);
      y = pcm_in(w.y);
    }
  }
  __device__ __forceinline__ void puti(long long i, double x, double y) const
  {
    if (kind == 4) w16[i * fstride] = pcm_pack16(x, y);
    else w32[i * fstride] = make_int2(pcm_out32(x), pcm_out32(y));
  }
  __device__ __forceinline__ void get(int i, double &x, double &y) const
  {
    if (kind == 1) {
      const float2 f = p2[i * fstride];
      x = (double)f.x;
      y = (double)f.y;
    } else if (kind == 3) {
      const double2 f = d2[i * fstride];
      x = f.x;
      y = f.y;
    } else if (kind >= 4) {
      geti(i, x, y);
    } else {
      x = pa[i];
      y = hasb ? pb[i] : 0.0;
    }
  }
  __device__ __forceinline__ void put(int i, double x, double y) const
  {
    if (kind == 1) p2[i * fstride] = make_float2((float)x, (float)y);
    else if (kind == 3) d2[i * fstride] = make_double2(x, y);
    else if (kind >= 4) puti(i, x, y);
    else {
      pa[i] = x;
      if (hasb) pb[i] = y;
    }
  }
};

// NPTS samples i0, i0 + istride, ... of a contiguous span (kind 1 or 2) into registers, every load issued before any is
// waited for.  (PairSpan::get in an unrolled loop keeps its kind / hasb tests per element, and the compiler then waits for
// each element's loads at the joins: 8-16 memory round trips in a row at the head of a workgroup.)
template <int NPTS, typename CT> __device__ __forceinline__ void span_load(const PairSpan &sp, int i0, int istride, CT (&dst)[NPTS])
{
  if (sp.kind == 1) {
#pragma unroll
    for (int s = 0; s < NPTS; ++s) {
      const float2 f = sp.p2[(i0 + s * istride) * sp.fstride];
      dst[s].x = (double)f.x;
      dst[s].y = (double)f.y;
    }
  } else if (sp.kind == 3) {
#pragma unroll
    for (int s = 0; s < NPTS; ++s) {
      const double2 f = sp.d2[(i0 + s * istride) * sp.fstride];
      dst[s].x = f.x;
      dst[s].y = f.y;
    }
  } else if (sp.kind == 4) { // (the raw words first: every load issues before the first conversion waits)
    unsigned w[NPTS];
#pragma unroll
    for (int s = 0; s < NPTS; ++s) w[s] = sp.w16[(i0 + s * istride) * sp.fstride];
#pragma unroll
    for (int s = 0; s < NPTS; ++s) {
      dst[s].x = pcm_lo16(w[s]);
      dst[s].y = pcm_hi16(w[s]);
    }
  } else if (sp.kind == 5) {
    int2 w[NPTS];
#pragma unroll
    for (int s = 0; s < NPTS; ++s) w[s] = sp.w32[(i0 + s * istride) * sp.fstride];
#pragma unroll
    for (int s = 0; s < NPTS; ++s) {
      dst[s].x = pcm_in(w[s].x);
      dst[s].y = pcm_in(w[s].y);
    }
  } else { // (pair_span sets pb = pa for a one-channel pair: both loads are unconditional)
#pragma unroll
    for (int s = 0; s < NPTS; ++s) {
      dst[s].x = sp.pa[i0 + s * istride];
      dst[s].y = sp.pb[i0 + s * istride];
    }
    if (!sp.hasb) {
#pragma unroll
      for (int s = 0; s < NPTS; ++s) dst[s].y = 0.0;
    }
  }
}

// (__host__ too: the launchers that pick a lean kernel instance ask this very function, not a copy of its predicate)
// INTS = false: for callers that are never handed integer PCM frames (the lean dftx instances; their launcher sees to it) --
// the integer branch is then not even compiled, and the function is instruction for instruction what it was without it.
template <bool INTS = true>
__host__ __device__ __forceinline__ PairSpan pair_span(const AnyView &v, int pair, bool hasb, long long a0, long long len, int ca = -1)
{
  if (ca < 0) ca = 2 * pair; // (pair_channels: differs only with an odd channel count per stream, where float frames are never contiguous pairs)
  PairSpan r;
  r.kind = 0;
  r.p2 = nullptr;
  r.fstride = 1;
  r.pa = r.pb = nullptr;
  r.hasb = hasb;
  r.d2 = nullptr;
  r.w16 = nullptr;
  r.w32 = nullptr;
  if (INTS && v.kind >= kFramesS16) { // as below, in shorts / ints; a pair is aligned as one word (4 / 8 bytes) or not taken
    if (hasb && !(v.f.nch & 1)) {
      const int hp = v.f.nch >> 1, strm = pair / hp, pin = pair - strm * hp, eb = frame_elem_bytes(v.kind);
      const char *ext = static_cast<const char *>(v.f.ext), *ring = static_cast<const char *>(v.f.ring);
      const char *p = nullptr;
      if (ext && a0 >= v.f.ext_begin && a0 + len <= v.f.ext_end)
        p = ext + (strm * v.f.ext_stream_stride + (a0 - v.f.ext_begin) * v.f.nch + 2 * pin) * eb;
      else if ((!ext || a0 + len <= v.f.ext_begin || a0 >= v.f.ext_end) && (a0 & v.f.ring_mask) + len <= v.f.ring_mask + 1)
        p = ring + (strm * v.f.ring_stream_stride + (a0 & v.f.ring_mask) * v.f.nch + 2 * pin) * eb;
      if (p && (reinterpret_cast<unsigned long long>(p) & (2 * eb - 1)) == 0) {
        r.fstride = hp;
        if (v.kind == kFramesS16) {
          r.kind = 4;
          r.w16 = reinterpret_cast<unsigned *>(const_cast<char *>(p));
        } else {
          r.kind = 5;
          r.w32 = reinterpret_cast<int2 *>(const_cast<char *>(p));
        }
      }
    }
  } else if (v.kind == kFramesF64) { // as below, in doubles; a pair is 16-byte aligned or not taken
    if (hasb && !(v.f.nch & 1)) {
      const int hp = v.f.nch >> 1, strm = pair / hp, pin = pair - strm * hp;
      const double *ext = static_cast<const double *>(v.f.ext), *ring = static_cast<const double *>(v.f.ring);
      const double *p = nullptr;
      if (ext && a0 >= v.f.ext_begin && a0 + len <= v.f.ext_end)
        p = ext + strm * v.f.ext_stream_stride + (a0 - v.f.ext_begin) * v.f.nch + 2 * pin;
      else if ((!ext || a0 + len <= v.f.ext_begin || a0 >= v.f.ext_end) && (a0 & v.f.ring_mask) + len <= v.f.ring_mask + 1)
        p = ring + strm * v.f.ring_stream_stride + (a0 & v.f.ring_mask) * v.f.nch + 2 * pin;
      if (p && (reinterpret_cast<unsigned long long>(p) & 15) == 0) {
        r.kind = 3;
        r.d2 = reinterpret_cast<double2 *>(const_cast<double *>(p));
        r.fstride = hp;
      }
    }
  } else if (v.kind) {
    if (hasb && !(v.f.nch & 1)) {
      const int hp = v.f.nch >> 1, strm = pair / hp, pin = pair - strm * hp;
      float *p = nullptr;
      if (v.f.ext && a0 >= v.f.ext_begin && a0 + len <= v.f.ext_end)
        p = static_cast<float *>(v.f.ext) + strm * v.f.ext_stream_stride + (a0 - v.f.ext_begin) * v.f.nch + 2 * pin;
      else if ((!v.f.ext || a0 + len <= v.f.ext_begin || a0 >= v.f.ext_end) && (a0 & v.f.ring_mask) + len <= v.f.ring_mask + 1)
        p = static_cast<float *>(v.f.ring) + strm * v.f.ring_stream_stride + (a0 & v.f.ring_mask) * v.f.nch + 2 * pin;
      if (p && (reinterpret_cast<unsigned long long>(p) & 7) == 0) {
        r.kind = 1;
        r.p2 = reinterpret_cast<float2 *>(p);
        r.fstride = hp;
      }
    }
  } else if ((a0 & v.d.mask) + len <= v.d.mask + 1) {
    r.kind = 2;
    r.pa = v.d.ring + (long long)ca * v.d.chan_stride + (a0 & v.d.mask);
    r.pb = hasb ? r.pa + v.d.chan_stride : r.pa;
  }
  return r;
}

// Work item -> (block, channel pair) for the one-workgroup-per-(block, pair) kernels; `lin` = linear workgroup id.
//
// hp <= 1 (stereo or planar data): pair-fastest order.  Blocks are dealt round-robin over the 8 XCDs, so with
// npairs % 8 == 0 the consecutive blocks of one pair land on the same XCD and their input overlap is an L2 hit.
//
// hp >= 2 (interleaved float frames of 2*hp channels): the hp workgroups of one (block, stream) each touch 8 bytes of
// every frame, i.e. the SAME 128-byte lines.  Spread over the 8 XCDs (each with its own L2) every line would be fetched
// by several L2s and written back in pieces (measured on 8-channel frames: 4.6x the output bytes in WRITE_SIZE).  Here
// they get linear ids lin, lin + 8, ..., lin + 8*(hp-1): same XCD under the observed round-robin placement, dispatched
// together, so the pieces meet in one L2.  Placement is a speed matter only; any placement is correct.
__device__ __forceinline__ bool item_map(int lin, int nblocks, int npairs, int hp, int &bl, int &pair)
{
  if (hp <= 1) {
    bl = lin / npairs;
    pair = lin - bl * npairs;
    return bl < nblocks;
  }
  const int xcd = lin & 7, t = lin >> 3;
  const int slot = t / hp, within = t - slot * hp, g = slot * 8 + xcd;
  const int nstreams = npairs / hp;
  if (g >= nblocks * nstreams) return false;
  bl = g / nstreams;
  pair = (g - bl * nstreams) * hp + within;
  return true;
}
inline int item_grid(int nblocks, int npairs, int hp)
{
  if (hp <= 1) return nblocks * npairs;
  const int ngroups = nblocks * (npairs / hp);
  return (ngroups + 7) / 8 * 8 * hp;
}
// pairs per interleaved frame that share cache lines (0 when the grouping does not apply)
inline int frame_pairs(const AnyView &in, const AnyView &out, int C)
{
  const AnyView *v = in.kind ? &in : out.kind ? &out : nullptr;
  if (!v || (v->f.nch & 1) || v->f.nch < 4 || C % v->f.nch) return 0;
  return v->f.nch / 2;
}

} // namespace rsmp
