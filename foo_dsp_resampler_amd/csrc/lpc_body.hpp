// lpc_extrapolate2 of the reference (lpc/lpc.cpp:25-191) for ONE channel, as the 64 lanes of one workgroup run it: the body that
// lpc.hip's kernel (one workgroup per (stream, channel) of a padded buffer) and tracks.hip's stage kernel (one per (track, channel,
// edge) of a packed source) share, so that the two cannot drift apart.  What fixes the bits is the ORDER of the arithmetic, and
// the order is the reference's everywhere; every file that includes this is compiled with -ffp-contract=off.
// Device code only.
#pragma once
#include "lpc.hpp"

namespace rsmp {

struct LpcShared {
  double r[kLpcMaxOrder + 1]; // autocorrelation, lags 0..order
  double a[kLpcMaxOrder];     // predictor, lpc[] of the reference
  float c[kLpcMaxOrder];      // c[m] = (float)a[31 - m]: the tap of the m-th of the last 32 samples (oldest first)
  int lo;                     // first tap in use: 32 - max_order
  int pad;
};
static_assert(sizeof(LpcShared) % 16 == 0, "the windowed copy behind it stays 16-byte aligned");

// NaN results: a NaN in the base frames comes out as a NaN (it passes the clamp), but its sign and payload are the hardware's.
// IEEE 754 leaves them open, and the reference's are no property of lpc.cpp either: SSE returns its FIRST NaN operand, and which
// operand of a commutative operation comes first is the host compiler's register allocation.

// one tap of lpc_extrapolate_data's inner loop (:172 / :185); falls through to the next younger sample
#define RSMP_LPC_TAP(m) case m: sum -= h[m] * c[m]; [[fallthrough]];
#define RSMP_LPC_TAP8(T, m) T(m) T(m + 1) T(m + 2) T(m + 3) T(m + 4) T(m + 5) T(m + 6) T(m + 7)
#define RSMP_LPC_TAPS(T) switch (lo) { RSMP_LPC_TAP8(T, 0) RSMP_LPC_TAP8(T, 8) RSMP_LPC_TAP8(T, 16) RSMP_LPC_TAP8(T, 24) default: break; }

// lds: LpcShared, then (kLds) room for n floats.  x(i) = base frame i of the channel, 0 <= i < n; put(i, v) stores extrapolated
// frame i, counted from base frame 0: -bk <= i < 0 behind lane 1, n <= i < n + fw behind lane 0.  Every lane of the workgroup
// calls this with the same arguments.
// kLds: the windowed copy of the channel lives in LDS (n <= kLpcLdsFrames); otherwise every use recomputes the window from x (the
// same float operations, so the same bits).
template <bool kLds, class Load, class Store>
__device__ __forceinline__ void lpc_channel(unsigned char *lds, int lane, long long n, float n2, int order, long long bk, long long fw,
                                            Load x, Store put)
{
  LpcShared &sh = *reinterpret_cast<LpcShared *>(lds);
  float *w = reinterpret_cast<float *>(lds + sizeof(LpcShared));

  // apply_window, :80-88 (Welch), on a private copy
  auto windowed = [&](long long i) {
    float k = (float)(int)(i + 1) - n2;
    k = k / n2;
    return x(i) * (1.0f - k * k);
  };
  if (kLds) {
    for (long long i = lane; i < n; i += 64) w[i] = windowed(i);
    __syncthreads();
  }

  // compute_autocorr, :91-105: lane j owns lag j
  if (lane <= order) {
    double d = 0;
    for (long long i = lane; i < n; ++i) {
      const float p = kLds ? w[i] : windowed(i), q = kLds ? w[i - lane] : windowed(i - lane);
      d += (double)p * (double)q;
    }
    sh.r[lane] = d;
  }
  __syncthreads();

  // compute_lpc, :107-160
  if (lane == 0) {
    const double *r = sh.r;
    double *a = sh.a;
    int used = order;
    double err = r[0] * (1. + 1e-10);
    const double eps = 1e-9 * r[0] + 1e-10;
    for (int i = 0; i < order; ++i) {
      if (err < eps) {
        for (int k = i; k < order; ++k) a[k] = 0;
        used = i;
        break;
      }
      double k = -r[i + 1];
      for (int j = 0; j < i; ++j) k -= a[j] * r[i - j];
      k /= err;
      a[i] = k;
      int j;
      for (j = 0; j < i / 2; ++j) {
        const double t = a[j];
        a[j] += k * a[i - 1 - j];
        a[i - 1 - j] += k * t;
      }
      if (i & 1) a[j] += a[j] * k;
      err *= 1.0 - k * k;
    }
    const double g = 0.999; // slightly damp the filter
    double damp = g;
    for (int j = 0; j < used; ++j) {
      a[j] *= damp;
      damp *= g;
    }
    if (used == 0) {
      used = 1;
      a[0] = -1;
    }
    for (int m = 0; m < kLpcMaxOrder; ++m) sh.c[m] = m >= kLpcMaxOrder - used ? (float)a[kLpcMaxOrder - 1 - m] : 0.0f;
    sh.lo = kLpcMaxOrder - used;
  }
  __syncthreads();

  // lpc_extrapolate_data, :162-191: lane 0 forward, lane 1 backward (the forward recursion over the reversed signal), both from
  // the unmodified frames.  h = the last 32 samples of the sequence, oldest first; taps below `lo` are not part of the filter.
  const int lo = __builtin_amdgcn_readfirstlane(sh.lo);
  const bool back = lane == 1;
  const long long extra = lane == 0 ? fw : back ? bk : 0;
  if (extra > 0) {
    float c[kLpcMaxOrder], h[kLpcMaxOrder];
#pragma unroll
    for (int m = 0; m < kLpcMaxOrder; ++m) {
      const long long t = n - kLpcMaxOrder + m;
      c[m] = sh.c[m];
      h[m] = t >= 0 ? x(back ? n - 1 - t : t) : 0.0f;
    }
    for (long long i = 0; i < extra; ++i) {
      float sum = 0.0f;
      RSMP_LPC_TAPS(RSMP_LPC_TAP)
      if (sum > 10.f) sum = 10.f; else if (sum < -10.f) sum = -10.f;
#pragma unroll
      for (int m = 0; m < kLpcMaxOrder - 1; ++m) h[m] = h[m + 1];
      h[kLpcMaxOrder - 1] = sum;
      put(back ? -1 - i : n + i, sum);
    }
  }
}

#undef RSMP_LPC_TAPS
#undef RSMP_LPC_TAP8
#undef RSMP_LPC_TAP

} // namespace rsmp
