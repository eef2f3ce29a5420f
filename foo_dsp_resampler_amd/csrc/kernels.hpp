// Kernel argument blocks and launch entry points (implemented in kernels.hip).
//
// Coordinates: every fifo between stages is addressed by ABSOLUTE sample index since the stream was
// opened (the preload zeros of rate_base.h:417-422 occupy indices [0, preload)).  Rings are powers of
// two, so index -> address is `idx & mask`.  All channels of a handle advance in lock step, which is
// why one set of indices serves every channel.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdint>

#include "knobs.hpp"

namespace rsmp {

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE attribute of a kernel: one process may hold handles on several
// GPUs (RRX_open_batch_on), so "already set" is remembered per (kernel instance, device).  Setting it twice is harmless,
// so a race between two handles' threads needs no lock.
struct DynLdsOnce {
  std::atomic<unsigned long long> mask{0};
  hipError_t set(const void *fn, int bytes)
  {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 64 && ((mask.load(std::memory_order_acquire) >> dev) & 1ull)) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess && dev < 64) mask.fetch_or(1ull << dev, std::memory_order_release);
    return e;
  }
};

// Interleaved frames: the caller-facing end of the chain (stage-0 input or final output).  A frame with absolute index a lives
// in the external buffer when ext != nullptr and ext_begin <= a < ext_end, else in the ring.  This is what lets a device-resident
// push be consumed in place and a device-resident pull be produced in place (no staging copy of bulk data).  The frame kind says
// what a sample is: float, double (RRX_FMT_DOUBLE) or integer PCM (RRX_FMT_S16 / RRX_FMT_S32).  ring / ext address samples of that
// type and every stride counts samples; the integer kinds convert on every load and quantise on every store (pcm_in / pcm_out
// below) around the same fp64 arithmetic.  kRingF64: no frames, the planar fp64 ring between two stages.
enum { kRingF64 = 0, kFramesF32 = 1, kFramesF64 = 2, kFramesS16 = 3, kFramesS32 = 4 };
__host__ __device__ constexpr int frame_elem_bytes(int kind) { return kind == kFramesF64 ? 8 : kind == kFramesS16 ? 2 : 4; } // per sample

// The integer formats' conversions (the ABI contract of include/ratelib_amd.h).  In: s * 2^-bits, exact in fp64.  Out:
// round half to even (v_rndne_f64), saturate to [-2^bits, 2^bits - 1] in fp64, then narrow -- the integer convert never sees
// a value it cannot hold (a NaN saturates to -2^bits: fmax / fmin return their other operand).
__host__ __device__ __forceinline__ double pcm_in(short s) { return (double)s * 0x1p-15; }
__host__ __device__ __forceinline__ double pcm_in(int s) { return (double)s * 0x1p-31; }
__host__ __device__ __forceinline__ short pcm_out16(double y)
{
  return (short)(int)fmin(fmax(rint(y * 32768.0), -32768.0), 32767.0);
}
__host__ __device__ __forceinline__ int pcm_out32(double y)
{
  return (int)fmin(fmax(rint(y * 2147483648.0), -2147483648.0), 2147483647.0);
}
// a channel pair of one S16 frame as one 4-byte word (channel 2p in the low half)
__host__ __device__ __forceinline__ unsigned pcm_pack16(double a, double b)
{
  return (unsigned)(unsigned short)pcm_out16(a) | ((unsigned)(unsigned short)pcm_out16(b) << 16);
}
__host__ __device__ __forceinline__ double pcm_lo16(unsigned w) { return pcm_in((short)(w & 0xffffu)); }
__host__ __device__ __forceinline__ double pcm_hi16(unsigned w) { return pcm_in((short)(w >> 16)); }
struct FrameView {
  void *ring;
  long long ring_mask;          // frames - 1
  long long ring_stream_stride; // samples between streams
  void *ext;
  long long ext_begin, ext_end; // absolute frame range held by ext
  long long ext_stream_stride;  // samples between streams
  int nch;                      // channels per stream
};

// Planar fp64 ring between two stages: [channel][cap].
struct RingView {
  double *ring;
  long long mask;        // items - 1
  long long chan_stride; // items between channels
};

// One fifo end, from the engine (Engine::view) through a launcher to its kernel: kind = a frame kind (the frames `f`) or kRingF64
// (the ring `d`); the half that is not in use is zero.  Read as a truth value, `kind` means "frames".
struct AnyView {
  int kind;
  FrameView f;
  RingView d;
};

struct DftArgs {
  const double2 *G;      // N entries: DFT_N(L * h_placed) / N, natural order, e^{-i} convention
  const double2 *Gr;     // dftx_kernel: [L][N/L] spectra of the filter's polyphase components, DFT_P(L * h_placed[L j + r]) / P
  const double2 *tw_fwd; // twiddle table for the forward size P
  const double2 *tw_inv; // twiddle table for the inverse size Nd
  const double2 *tw_fwd8; // forward size P, 8-points-per-thread plan (fft8_regs)
  const double2 *tw_inv8; // inverse size Nd, 8-points-per-thread plan (frequency-domain decimation by 2)
  long long B0;          // absolute index of the first block of this launch
  long long out_offset;  // preload of the destination fifo (absolute index of stage output 0)
  int nblocks;
  int C;                 // total channels (streams * nch)
  int L;                 // zero-stuffing factor
  int c0;                // initial remL (time-domain stuffing phase)
  int V;                 // N - (taps-1): valid filtered samples per block before decimation
  int Vout;              // outputs kept per block when M == 1 (V, or the frequency-domain decimated count)
  int q;                 // inputs consumed per block (frequency-domain paths)
  int M;                 // time-domain decimation step (1 = none)
  int nchs;              // > 0: channels per stream of a batch handle whose pairs must not straddle streams (pair_channels); else 0
  int npairs;            // pair_count(C, nchs), filled in by the launchers
  unsigned pps_magic;    // ceil(2^32 / pairs per stream) when nchs > 0 (pair_magic), filled in by the launchers
  int hp;                // channel pairs per interleaved float frame whose workgroups are co-located (item_map); 0/1 = none
  long long in_limit;    // input items at absolute index >= in_limit read as zero (unused by the engine: always +inf)
  long long clip_lo, clip_hi; // only stage outputs with absolute index in [clip_lo, clip_hi) are stored (always everything)
  // Sub-blocked fused launch (fused_fast_kernel<.., SPLIT>, fused_fast.hip): every block of the reference is computed as
  // `nsub` sub-blocks of `Vs` valid samples (the last one shorter) on 4096-point component transforms; B0 / nblocks then
  // count SUB-blocks (B0 = Bref0 * nsub) and G holds the two component spectra.  nsub = 0: not sub-blocked.
  int nsub, Vs;
  int two;               // 1: whole 8192-point blocks (nsub = 1, Vs = V), polyphase stage in two rounds (kSplitRaEnd / kSplitRbStart)
  int Pref;              // inputs a reference block spans (N / L)
  long long Bref0;       // first reference block of the launch
};

// Geometry of sub-block `i` of a reference block with V valid samples out of N/L = `Pref` inputs (x2 chains): its `len` valid
// samples start `off` samples into the block's valid range; its 4096-point input window starts `win` inputs into the block's
// input span -- as late as the samples allow, but never so late that it would reach past the block's own inputs -- and its
// first valid sample is element `shift` of each component transform's output.
struct SubBlock { int off, len, win, shift; };
__host__ __device__ inline SubBlock sub_block(int i, int V, int Vs, int Pref)
{
  SubBlock s;
  s.off = i * Vs;
  s.len = V - s.off < Vs ? V - s.off : Vs;
  s.win = (s.off >> 1) < Pref - 4096 ? (s.off >> 1) : Pref - 4096;
  s.shift = (s.off >> 1) - s.win;
  return s;
}

// number of channel pairs (= workgroups per block) of a launch, see pair_channels (fifo_device.hpp)
__host__ __device__ inline int pair_count(int C, int nchs) { return nchs > 0 ? (C / nchs) * ((nchs + 1) >> 1) : (C + 1) >> 1; }

__host__ __device__ inline unsigned pair_magic(int C, int nchs)
{
  const unsigned long long pps = (unsigned long long)(((nchs > 0 ? nchs : C) + 1) >> 1);
  return pps <= 1 ? 0u : (unsigned)(((1ull << 32) + pps - 1) / pps); // 0: one pair per stream, no division
}

// Can pair_channels serve every pair of such a handle?  With magic = ceil(2^32 / pps) = (2^32 + e) / pps, 0 <= e < pps, the
// quotient __umulhi(pair, magic) = floor(pair / pps + pair * e / (pps * 2^32)) is floor(pair / pps) whenever pair * e < 2^32,
// and pair * pps <= 2^32 sees to that for every e.  The pairs of a handle run below npairs, so npairs * pps <= 2^32 is enough.
// One case needs less: with nchs = 0 and an even C every pair lies in "stream" 0 of pps = C / 2 pairs, the quotient is 0 or 1
// (pair * magic < 2^32 + pps), and a quotient of 1 leaves ca = C + 2 * (pair - pps) = 2 * pair and hasb true all the same.  With
// an odd C that slip gives 2 * pair - 1: a one-stream handle of 131 073 channels (pps = 65 537, magic = 65 536) would hand its
// last pair channel 131 071 instead of 131 072.  Engine::create refuses what this function refuses.
inline bool pair_division_exact(int C, int nchs)
{
  if (nchs <= 0 && !(C & 1)) return true;
  const unsigned long long pps = (unsigned long long)(((nchs > 0 ? nchs : C) + 1) >> 1);
  return (unsigned long long)pair_count(C, nchs) * pps <= (1ull << 32);
}

// Long blocks (N = 32768 ... 131072): N = 16 x M four-step transform in three launches through a workspace (dftbig.hip)
struct BigDftArgs {
  DftArgs d;             // tw_fwd / tw_inv: fft_regs tables of the forward / inverse ROW lengths
  const double2 *twN;    // exp(+2 pi i j / N), j < N
  double2 *w1, *w2;      // workspaces [item][16][Mp] and [item][16][Md]
  int log2n, log2mp, log2md; // block length; forward / inverse row lengths (log2 of P/16 and Nd/16)
  int fdomain_in;        // 1: the block is 16*Mp consecutive stage inputs (L = 1, or xL in the frequency domain); 0: zero stuffing
  int item0;             // first (block, pair) item of this launch (filled in by launch_dft_big)
};
bool big_dft_supported(int log2n, int log2p, int log2nd);
hipError_t launch_dft_big(const AnyView &in, const AnyView &out, BigDftArgs a, int ws_items, hipStream_t st);

// per-block output bookkeeping of the fused launch, computed on the host (64-bit divisions stay there)
struct FusedBlock {
  long long i_lo; // first output whose window starts inside the block (absolute output index)
  int cnt;        // number of such outputs whose window also ends inside the block
  int irel_lo;    // i_lo - kk_lo * polyL, kk_lo = i_lo / polyL (first period touched)
  int base_li;    // kk_lo * step - b0: window start of (period kk_lo, residue r) is qr(r) + base_li
  int K;          // periods touched by [i_lo, i_lo + cnt)
  int KA;         // matrix-pipe variant: periods [0, KA) are computed from the first LDS image, the rest from the second
  // lean kernels' tile walk (fused_walk below): bit 31 set = every 16-residue group starts at its OWN first period; bits 0-9
  // the first group whose residues do not all lie below irel_lo (groups in front of it start at period 1), bits 10-19 the
  // first group whose residues all lie at or behind the block's last partial period (its groups end one period early),
  // bits 20-30 the periods (counted from the group's first) that the first LDS image takes.  0 = the uniform walk of KA.
  int walk;
  // seam outputs in front of this block (window straddles blocks B-1 | B): indices [seam_i0, i_lo); output seam_i0 has
  // phase seam_ph0 and its window starts seam_q0 samples into the [tail of B-1 | head of B] image (seam_kernel)
  long long seam_i0;
  int seam_q0, seam_ph0;
};
// Matrix-pipe variant of the fused kernel (N = 4096, 256 threads): the block's samples sit in LDS in two rounds,
// round A = register slots [0, kFusedSA) of the inverse FFT (samples [0, 256*kFusedSA) plus a 32-sample margin),
// round B = slots [kFusedSB0, 16); the two overlap by (kFusedSA - kFusedSB0) * 256 + 32 samples, which every period's
// windows (all residues) must fit into one way or the other.  Sized for three workgroups per CU.
constexpr int kFusedSA = 12, kFusedSB0 = 10, kFusedWaves = 3;

// The lean kernels' tile walk (fused_fast.hip: poly_round).  A tile is one 16-residue group x 4 consecutive periods.  Group g
// owns periods [p0, pend) of the block (counted from kk_lo): p0 = 1 for the groups in front of g_lo, pend = K - 1 for the
// groups from g_hi on.  A round of periods [kb, ke) gives group g the periods [kb + p0, min(ke + p0, pend)), so with
// g_lo = 0 and g_hi = NGRP every group walks [kb, ke): the uniform walk.  The same functions serve the kernel, the block
// table (fused_block_info) and the host-side enumeration behind RRX_debug_tile_walk.
struct FusedWalk { int g_lo, g_hi, ka; }; // ka: the first round is [0, ka), the second [ka, K)
__host__ __device__ inline FusedWalk fused_walk(const FusedBlock &fb, int ngrp)
{
  if (fb.walk >= 0) return FusedWalk{0, ngrp, fb.KA};
  return FusedWalk{fb.walk & 1023, (fb.walk >> 10) & 1023, (fb.walk >> 20) & 2047};
}
__host__ __device__ inline int walk_p0(const FusedWalk &w, int g) { return g < w.g_lo ? 1 : 0; }
// column steps of group g in the round [kb, ke); a group with nothing in the round keeps one (all its lanes are dropped by
// the store's range check), so that the walk never has to jump over a group
__host__ __device__ inline int walk_ncs(const FusedWalk &w, int K, int kb, int ke, int g)
{
  const int p0 = walk_p0(w, g), pend = g >= w.g_hi ? K - 1 : K;
  const int e = ke + p0 < pend ? ke + p0 : pend, n = (e - kb - p0 + 3) >> 2;
  return n > 0 ? n : 1;
}
// A round's tiles in group-major order: the groups form at most three runs of equal column-step count, [0, b1), [b1, b2)
// and [b2, ngrp), which start at tiles 0, T1 and T2 of the round's nt.
// Invariant the kernel's group switch relies on: walk_p0 and walk_ncs are constant inside each run (they depend on g only
// through g < g_lo and g >= g_hi), so poly_round refetches them only when the next group is b1 or b2.
struct WalkRound { int b1, b2, n0, n1, n2, T1, T2, nt; };
__host__ __device__ inline WalkRound walk_round(const FusedWalk &w, int K, int kb, int ke, int ngrp)
{
  WalkRound r;
  const int lo = w.g_lo < ngrp ? w.g_lo : ngrp, hi = w.g_hi < ngrp ? w.g_hi : ngrp;
  r.b1 = lo < hi ? lo : hi;
  r.b2 = lo < hi ? hi : lo;
  r.n0 = walk_ncs(w, K, kb, ke, 0);
  r.n1 = walk_ncs(w, K, kb, ke, r.b1);
  r.n2 = walk_ncs(w, K, kb, ke, r.b2);
  r.T1 = r.b1 * r.n0;
  r.T2 = r.T1 + (r.b2 - r.b1) * r.n1;
  r.nt = r.T2 + (ngrp - r.b2) * r.n2;
  return r;
}
// tile t of the round -> its group and column step (the one integer division of a wave's walk)
__host__ __device__ inline void walk_seek(const WalkRound &r, int t, int &g, int &c)
{
  int gb = 0, tb = 0, n = r.n0;
  if (t >= r.T2) {
    gb = r.b2, tb = r.T2, n = r.n2;
  } else if (t >= r.T1) {
    gb = r.b1, tb = r.T1, n = r.n1;
  }
  const int dg = (t - tb) / n;
  g = gb + dg;
  c = t - tb - dg * n;
}
// A lane's part of a tile's addresses in the round that starts at period kb (lane = 16 hi + 4 bq + jq, rloc = 4 bq + hi): the
// window of (group g, period offset pc) starts at walk_lane_li + q(g, bq) + pc * step, its output is number
// walk_lane_ib + 16 g + pc * polyL of the block, kept when that lies in [0, walk_round_cnt).
__host__ __device__ inline int walk_lane_li(int base_li, int kb, int hi, int jq, int step) { return base_li + hi + (kb + jq) * step; }
__host__ __device__ inline int walk_lane_ib(int irel_lo, int kb, int jq, int rloc, int pl) { return (kb + jq) * pl + rloc - irel_lo; }
// q(g, bq): the window start of the 4-residue block rb = 16 g + 4 bq within its period, (at0 + rb * step) / polyL; an idle block
// of a partial last group (rb >= polyL: all-zero coefficients, any in-range window will do) takes block 0's.  The host table
// (qtab) holds these values for the generic kernel and polymf_kernel.  The lean kernels compute them where a group becomes
// current, with no memory access: the quotient is the high half of numerator x m, shifted right by s (WalkRcp, chosen by
// walk_rcp so that it is exact for every numerator up to nmax, the largest one a launch can form).
__host__ __device__ inline int walk_q_rb(int g, int bq, int pl)
{
  const int rb = 16 * g + 4 * bq;
  return rb >= pl ? 0 : rb;
}
__host__ __device__ inline int walk_q_table(long long at0, int step, int pl, int g, int bq)
{
  return int((at0 + (long long)walk_q_rb(g, bq, pl) * step) / pl);
}
struct WalkRcp { unsigned m; int s; unsigned nmax; };
__host__ __device__ inline int walk_q_rcp(unsigned num, unsigned m, int s) { return int(unsigned(((unsigned long long)num * m) >> 32) >> s); }
// m = ceil(2^(32 + s) / polyL) with the smallest s for which floor(num * m / 2^(32 + s)) = floor(num / polyL) for all num <= nmax:
// num * m / 2^(32 + s) = num / polyL + num * e / (polyL * 2^(32 + s)) with e = m * polyL - 2^(32 + s) in [0, polyL), and the second
// term cannot carry the first over an integer while it is below 1 / polyL, i.e. while nmax * e < 2^(32 + s).  False where no
// 32-bit multiplier does it (polyL = 1 among them: m would be 2^32), or the numerators do not fit 31 bits.
inline bool walk_rcp(long long at0, int step, int pl, WalkRcp &r)
{
  if (at0 < 0 || step < 1 || pl < 2) return false;
  const long long nmax = at0 + (long long)((pl - 1) & ~3) * step;
  if (nmax > 0x7fffffffLL) return false;
  for (int s = 0; s < 31; ++s) {
    const unsigned long long pow = 1ull << (32 + s), m = (pow + pl - 1) / pl, e = m * pl - pow;
    if (m > 0xffffffffull) break;
    if ((unsigned long long)nmax * e < pow) {
      r = WalkRcp{unsigned(m), s, unsigned(nmax)};
      return true;
    }
  }
  return false;
}
// outputs of the block that a round up to period ke may store: the round ends at period ke for the groups that start at 0
// and at ke + 1 for the others (a group that starts at 0 has exact column steps there and never reaches period ke)
__host__ __device__ inline int walk_round_cnt(const FusedBlock &fb, const FusedWalk &w, int ke, int pl)
{
  const int irel_hi = fb.irel_lo + fb.cnt, e = (ke + (w.g_lo > 0 ? 1 : 0)) * pl;
  return (irel_hi < e ? irel_hi : e) - fb.irel_lo;
}
// tiles of a block: both rounds (the second only when the first leaves periods over)
__host__ __device__ inline int fused_walk_tiles(const FusedWalk &w, int K, int ngrp)
{
  return (w.ka > 0 ? walk_round(w, K, 0, w.ka, ngrp).nt : 0) + (w.ka < K ? walk_round(w, K, w.ka, K, ngrp).nt : 0);
}

// Closed forms of a block's bookkeeping; evaluated by fused_prep_kernel on the device (one thread per block of the
// launch) and by the engine for its consistency checks.
struct FusedPrepArgs {
  long long b_offset, B0, at0; // as in FusedArgs / DftArgs
  int V, polyL, step, n, nblocks;
  int two_round, KS, qb_max;   // matrix-pipe variant: split of the periods over its two LDS images
  int ra_end, rb_start;        // ... the first image holds samples [0, ra_end) (+ 32), the second starts at rb_start; 0 = the lean
                               // kernel's kFusedSA * 256 / kFusedSB0 * 256
  int qb_min;                  // (smallest / largest window start of a 4-residue block, relative to its period)
  long long clip_lo, clip_hi;  // only outputs with index in [clip_lo, clip_hi) belong to this launch (standalone stage)
  int nsub, Vs;                // sub-blocked launch (DftArgs::nsub): entry k is sub-block k % nsub of reference block B0 + k / nsub
};
__host__ __device__ inline FusedBlock fused_block_info(const FusedPrepArgs &p, int k)
{
  long long b0 = p.b_offset + (p.B0 + k) * (long long)p.V;
  int V = p.V;
  if (p.nsub > 0) {
    const int kr = k / p.nsub, i = k - kr * p.nsub;
    b0 = p.b_offset + (p.B0 + kr) * (long long)p.V + (long long)i * p.Vs;
    V = p.V - i * p.Vs < p.Vs ? p.V - i * p.Vs : p.Vs;
  }
  const long long nlo = b0 * p.polyL - p.at0, nhi = (b0 + V - p.n + 1) * p.polyL - p.at0;
  long long ilo = nlo <= 0 ? 0 : (nlo + p.step - 1) / p.step, ihi = nhi <= 0 ? 0 : (nhi + p.step - 1) / p.step;
  if (ilo < p.clip_lo) ilo = p.clip_lo;
  if (ihi > p.clip_hi) ihi = p.clip_hi;
  FusedBlock fb;
  fb.i_lo = ilo;
  fb.cnt = ihi > ilo ? int(ihi - ilo) : 0;
  const long long kk_lo = ilo / p.polyL;
  fb.irel_lo = int(ilo - kk_lo * p.polyL);
  fb.base_li = int(kk_lo * p.step - b0);
  fb.K = fb.cnt > 0 ? int((ihi - 1) / p.polyL - kk_lo) + 1 : 0;
  fb.KA = fb.K;
  int fit = fb.K; // periods (from 0) whose windows end inside the first LDS image: all of them unless there are two
  { // first output whose window starts at or behind the previous block's tail: (b0 - (n - 1)) * L - at0 over step, rounded up
    const long long ns = (b0 - (p.n - 1)) * p.polyL - p.at0;
    const long long s0 = ns <= 0 ? 0 : (ns + p.step - 1) / p.step;
    const long long a0 = p.at0 + s0 * p.step, q0 = a0 / p.polyL;
    fb.seam_i0 = s0;
    fb.seam_q0 = int(q0 - (b0 - (p.n - 1)));
    fb.seam_ph0 = int(a0 - q0 * p.polyL);
  }
  const int ra_end = p.ra_end > 0 ? p.ra_end : kFusedSA * 256, rb_start = p.ra_end > 0 ? p.rb_start : kFusedSB0 * 256;
  if (p.two_round && V > ra_end) { // periods whose (padded) windows end inside the first LDS image
    const int a_hi = ra_end + 32 - 4 * p.KS - 3, num = a_hi - fb.base_li - p.qb_max;
    const int ka = num < 0 ? 0 : num / p.step + 1;
    fb.KA = ka < fb.K ? ka : fb.K;
    // a multiple of 4 periods in the first image when the second one can take the rest: the two rounds then need
    // ceil(K / 4) column steps of 4 periods together instead of one more
    const int k4 = fb.KA & ~3;
    if (fb.KA < fb.K && k4 > 0 && fb.base_li + p.qb_min + k4 * p.step >= rb_start) fb.KA = k4;
    fit = ka;
  }
  // Per-group period ranges.  Residues >= irel_lo own periods 0 .., the others 1 ..; residues below (irel_lo + cnt) mod polyL
  // own the last period K - 1, the others end at K - 2: a group whose 16 residues agree needs one column step of 4 periods
  // less than ceil(K / 4) whenever K is one past a multiple of 4 -- the common case, since a block's first output has an
  // arbitrary residue.  With two LDS images the split moves with the group's start, group g's periods [p0_g, p0_g + 4a) go
  // to the first image: the last of them (4a - 1, or 4a where some group starts at 1) must end inside it, and period 4a of
  // a group that starts at 0 must start inside the second -- the conditions of KA above.  Among the a that satisfy both the
  // one with the fewest tiles is taken; where there is none, or the uniform walk has fewer tiles, `walk` stays 0.
  fb.walk = 0;
  const int ngrp = (p.polyL + 15) >> 4;
  if (fb.cnt > 0 && ngrp <= 1023 && fb.K <= 2047) {
    FusedWalk w;
    w.g_lo = fb.irel_lo >> 4;
    w.g_hi = (fb.irel_lo + fb.cnt - 1 - (fb.K - 1) * p.polyL + 16) >> 4;
    w.ka = fb.K;
    const int p1 = w.g_lo > 0 ? 1 : 0;                  // some group starts at period 1
    const int maxlen = w.g_lo < w.g_hi ? fb.K : fb.K - 1; // periods of the longest group
    int best = -1, best_ka = 0;
    if (fit >= fb.K) {
      best = fused_walk_tiles(w, fb.K, ngrp);
      best_ka = fb.K;
    } else {
      for (int a4 = 4; a4 + p1 <= fit; a4 += 4) {
        const bool all = a4 >= maxlen; // nothing left for the second image: one round
        if (!all && fb.base_li + p.qb_min + a4 * p.step < rb_start) continue;
        w.ka = all ? fb.K : a4;
        const int t = fused_walk_tiles(w, fb.K, ngrp);
        if (best < 0 || t < best) {
          best = t;
          best_ka = w.ka;
        }
        if (all) break;
      }
    }
    const FusedWalk u = {0, ngrp, fb.KA};
    if (best >= 0 && best <= fused_walk_tiles(u, fb.K, ngrp))
      fb.walk = int(0x80000000u | unsigned(w.g_lo) | unsigned(w.g_hi) << 10 | unsigned(best_ka) << 20);
  }
  return fb;
}
// Start states of the tile walk, one record per table entry beside its FusedBlock: everything poly_round used to derive from
// the entry, the round and the wave index with ~250 dependent scalar instructions and one division -- behind a barrier, on
// all four waves alike -- evaluated once per block by fused_prep_kernel.  The lean kernels fetch the record with their
// input loads and keep only the per-lane terms (walk_lane_li / walk_lane_ib) on the path between a barrier and its first tile.
// Round 0 = periods [0, ka), round 1 = [ka, K); a round the block does not have, and a wave without tiles, is all zero.
struct WalkStartWave { int n, g, pc, pend; }; // tiles of the wave; its first group, and pc / pend as poly_round counts them
struct WalkStartRound {
  int kb, ke, cnt;      // periods of the round, outputs it may store (walk_round_cnt)
  int b1, b2;           // run boundaries (WalkRound)
  int p0[3], pend[3];   // first period and end (p0 + 4 column steps) of the groups of each run
  int pad;
  WalkStartWave w[4];
};
struct alignas(16) WalkStart { WalkStartRound r[2]; };
static_assert(sizeof(WalkStartRound) == 112 && sizeof(WalkStart) == 224, "WalkStart: fixed layout (the kernels read it as dwords)");
// one round of the record, written in place (fused_prep_kernel: one thread per entry and round, straight into the table)
__host__ __device__ inline void fused_walk_start_round(const FusedBlock &fb, int ngrp, int pl, int round, WalkStartRound &r)
{
  const FusedWalk fw = fused_walk(fb, ngrp);
  const int kb = round ? fw.ka : 0, ke = round ? fb.K : fw.ka;
  const bool have = fb.cnt > 0 && ke > kb;
  WalkRound wr = {0, 0, 0, 0, 0, 0, 0, 0};
  if (have) wr = walk_round(fw, fb.K, kb, ke, ngrp);
  r.kb = have ? kb : 0;
  r.ke = have ? ke : 0;
  r.cnt = have ? walk_round_cnt(fb, fw, ke, pl) : 0;
  r.b1 = wr.b1;
  r.b2 = wr.b2;
  r.pad = 0;
  const int gs[3] = {0, wr.b1, wr.b2};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int p0 = walk_p0(fw, gs[i]);
    r.p0[i] = have ? p0 : 0;
    r.pend[i] = have ? p0 + 4 * walk_ncs(fw, fb.K, kb, ke, gs[i]) : 0;
  }
#pragma unroll
  for (int wave = 0; wave < 4; ++wave) {
    const int t0 = (wr.nt * wave) >> 2, t1 = (wr.nt * (wave + 1)) >> 2; // this wave's tiles, group-major
    WalkStartWave e = {0, 0, 0, 0};
    if (t0 < t1) {
      int g, c;
      walk_seek(wr, t0, g, c);
      const int p0 = walk_p0(fw, g);
      e = WalkStartWave{t1 - t0, g, 4 * c + p0, p0 + 4 * walk_ncs(fw, fb.K, kb, ke, g)};
    }
    r.w[wave] = e;
  }
}
__host__ __device__ inline WalkStart fused_walk_start(const FusedBlock &fb, int ngrp, int pl)
{
  WalkStart s;
  fused_walk_start_round(fb, ngrp, pl, 0, s.r[0]);
  fused_walk_start_round(fb, ngrp, pl, 1, s.r[1]);
  return s;
}
// the group switch of the walk: first period and end of group gnext when it opens a run, else the values it had (runs are
// constant in both, WalkRound); b2 first, so that an empty middle run (b1 == b2) takes the last run's
__host__ __device__ inline void walk_next_group(const WalkStartRound &r, int gnext, int &p0, int &pend)
{
  if (gnext == r.b2) p0 = r.p0[2], pend = r.pend[2];
  else if (gnext == r.b1) p0 = r.p0[1], pend = r.pend[1];
}
constexpr int kFusedMaxBlocks = 1024; // capacity of the per-stage block table in HBM

// dft -> vpoly0 fused launch (fused.hip)
struct FusedArgs {
  DftArgs d;             // the FFT-FIR part (out_offset unused)
  const double *tab;     // polyphase table [phase][tap]
  const double *cft;     // per-thread coefficient tiles [tap < 32][g < 2][thread], shifted + zero padded
  double *seam;          // [slot][channel (C + 1 of them)][head|tail][32] stage-1 samples at block edges
  long long at0;         // absolute initial clock of the poly stage, units 1/polyL
  long long b_offset;    // preload of the stage-1 fifo (absolute index of the first FFT output)
  long long out_offset2; // preload of the fifo after the poly stage
  int seam_mask;         // slots - 1
  int n, polyL, step;    // taps per phase, phases, clock step
  int span;              // n + largest window offset inside a G-tile
  int NG, KC;            // residue groups, period chunks (NG * KC <= threads)
  int kper;              // periods per chunk
  const double *cfm;     // matrix-pipe variant: A operands [16-residue group][k-step][lane]; null = vector variant
  int NGRP, KS;          // 16-residue groups, k-steps (4 taps each) of a 4-residue block's common window
  unsigned long long *stamps; // RSMP_STAMPS: per-phase cycle sums [8] (null in production)
  const FusedBlock *blk; // [nblocks] in HBM, written by fused_prep_kernel ahead of the launch
  const int *qtab;       // matrix-pipe variant: window start (at0 + rb*step)/polyL of every 4-residue block rb = 4*i, [NGRP*4]
  const double2 *cfm2;   // the same A operands two k-steps per 16-byte element: [group][(KS + 1) / 2][lane] (lean kernel)
  const WalkStart *wst = nullptr; // [nblocks] beside blk: the tile walk's start states (lean kernels only)
  unsigned rcp_m = 0;    // lean kernels: the window start of a 4-residue block by multiply-high and shift (WalkRcp); a launch
  int rcp_s = 0;         // of theirs with rcp_m = 0 is refused
};

// Lean fast path of the matrix-pipe variant (fused_fast.hip): both ends are plain interleaved frames in one buffer each
struct FastIo {
  const void *in;             // frame `in_abs0` (absolute input index) of stream 0, channel 0
  const void *in_ring;        // frames below in_abs0 (the tail of the previous push): fifo 0's ring, frame (index & in_ring_mask)
  long long in_ring_mask, in_ring_stream_stride;
  void *out;                  // frame `out_abs0` (absolute index in the output fifo) of stream 0, channel 0
  long long in_abs0, out_abs0;
  long long in_stream_stride, out_stream_stride; // samples between streams
  int nch;                    // channels per stream (even)
  int in_unaligned;           // sub-blocked form only: a channel pair of `in` is not aligned as one word (channels read one sample at a time)
  // sub-blocked form, omode 2: frame with absolute index A is in `out` when out_abs0 <= A < out_end, else in the fifo's ring
  void *out_ring;
  long long out_ring_mask, out_ring_stream_stride, out_end;
  int out_unaligned;          // a channel pair of `out` is not aligned as one word
  // OUT64 instances (the polyphase stage feeds another stage): planar fp64 ring of the destination fifo instead of `out`
  double *out64;              // ring of channel 0
  long long out64_mask, out64_chan_stride; // items - 1, items between channels
  // Sample format of the caller-facing frames, which picks the kernel instance: 0 = float32, 1 = float64 (*_dio_kernel),
  // 2 = 16-bit PCM (*_s16_kernel), 3 = 32-bit PCM (*_s32_kernel).  in / in_ring / out / out_ring address samples of that type,
  // every stride and frame offset above counts samples, and a channel pair is one word of 8 / 16 / 4 / 8 bytes
  int dio;
};
bool fused_fast_supported(int log2n, int log2p, int ksteps);
hipError_t launch_fused_fast(int log2p, const FusedArgs &a, const FastIo &io, hipStream_t st, const char **kname = nullptr);
// the sub-blocked form (fused_split_kernel): x2 stages with 8192- or 16384-point blocks -> vpoly0
constexpr int kSplitVsMax = 5056; // valid samples of a sub-block: (32 + Vs + 32) 16-byte LDS elements, two workgroups per CU
// 8192-point blocks fit ONE pair of component transforms whole (V = 8192 - (taps - 1) samples): one workgroup, the polyphase
// stage in two rounds -- samples [0, kSplitRaEnd) (register slots 0 .. 8 of both components) first, [kSplitRbStart, V) from
// the slots kept in registers (8 .. 15) afterwards
constexpr int kSplitSA = 9, kSplitSB0 = 8, kSplitRaEnd = 2 * kSplitSA * 256, kSplitRbStart = 2 * kSplitSB0 * 256;
bool fused_split_supported(int log2n, int L, int ksteps);
// omode: 0 = float frames straight into FastIo::out (every output of the launch lies inside it, 8-byte aligned), 1 = the next
// fifo's fp64 ring (out64), 2 = float frames wherever the output fifo has them (out / out_ring)
hipError_t launch_fused_split(int omode, const FusedArgs &a, const FastIo &io, hipStream_t st, const char **kname = nullptr);
bool fused_split_two_supported(int V, int taps, int ksteps, int qb_spread); // the whole-block two-round form (8192-point blocks)

struct PolyArgs {
  const double *tab;     // [phase][tap][order+1]
  long long rd;          // absolute index of the stage's read pointer
  long long at;          // clock relative to rd: integer (order 0, units 1/L) or 32.32 fixed point
  long long step;        // same units as `at`
  long long out_abs;     // absolute index (in the destination fifo) of output 0 of this launch
  long long count;       // outputs to produce
  int C, n, L, phase_bits, tile, win;
  int tab_lds;           // order 0: copy the [L][n] table into LDS behind the window (it fits)
  int coop;              // orders 1-3: 8 lanes per output (poly_coop_kernel); needs n % 8 == 0
  int shared_rows;       // orders 1-3: interpolated rows computed once per tile and shared by 16 channels (polyi_kernel);
                         // `win` is then the per-channel window stride in doubles (odd)
};

struct HalfArgs {
  long long rd, out_abs, count;
  int C, ncoef, pre;
  double coef[13];
};

// All launchers return hipSuccess or the launch error; `kname` (optional) receives the name of the kernel instance
// that was picked, as rocprofv3 prints it (static string).
hipError_t launch_dft(int log2n, int log2p, int log2nd, const AnyView &in, const AnyView &out, const DftArgs &a, hipStream_t st,
                      const char **kname = nullptr);
hipError_t launch_poly(int order, const AnyView &in, const AnyView &out, const PolyArgs &a, hipStream_t st, const char **kname = nullptr);
hipError_t launch_half(const AnyView &in, const AnyView &out, const HalfArgs &a, hipStream_t st, const char **kname = nullptr);
bool dft_shape_supported(int log2n, int log2p, int log2nd);
// x4 upsampling on 8192-point blocks as four 2048-point component transforms (dftx.hip); needs DftArgs::Gr
bool dftx_supported(int log2n, int log2p, int log2nd);
hipError_t launch_dftx(int log2n, const AnyView &in, const AnyView &out, const DftArgs &a, hipStream_t st, const char **kname = nullptr);
hipError_t launch_fused(int log2n, int log2p, const AnyView &in, const AnyView &out, const FusedArgs &a, hipStream_t st,
                        const char **kname = nullptr);
// seam_kernel: the outputs whose window straddles two blocks; launch after launch_fused on the same stream
hipError_t launch_seam(const AnyView &out, const FusedArgs &a, hipStream_t st);
bool fused_shape_supported(int log2n, int log2p, int n, int span, int max_seam_outputs);
bool fused_mfma_supported(int log2n, int log2p, int ksteps);
// wst (optional): the lean kernels' WalkStart record of every entry, next to it
hipError_t launch_fused_prep(const FusedPrepArgs &p, FusedBlock *out, hipStream_t st, WalkStart *wst = nullptr);
// host only (test hook): every (round, group, column step, lane) slot of entry k's tile walk in the lean kernels, 7 ints per slot
// (round, group, column step, lane, output index relative to i_lo, 1 if the store's range check keeps it, window start);
// head[13] = i_lo, cnt, K, KA, per-group walk?, g_lo, g_hi, ka, tiles, tiles of the uniform walk, irel_lo, base_li, groups.
// Returns the number of slots (only the first `cap` are written).
size_t fused_walk_enumerate(const FusedPrepArgs &p, int k, long long *head, int *slots, size_t cap);
// host only (test hook): entry k's WalkStart record as 56 ints
void fused_walk_start_host(const FusedPrepArgs &p, int k, int *out56);
// host only (test hook): q(g, bq) as the lean kernels compute it (walk_q_rcp) and as qtab holds it (walk_q_table), with the
// multiplier, shift and largest numerator of walk_rcp in rcp3; false where walk_rcp finds no multiplier
bool fused_window_start_host(long long at0, int step, int pl, int g, int bq, int *arith, int *table, unsigned *rcp3);

// standalone rational polyphase stage on the matrix pipe (polymf.hip)
struct PolyMfArgs {
  const double *cfm;     // A operands [16-residue group][k-step][lane], as in FusedArgs
  const int *qtab;       // window start of every 4-residue block, as in FusedArgs
  const FusedBlock *blk; // per tile: fused_block_info with V = Vt, n = 1, b_offset = 0, clipped to the launch's outputs
  long long B0;          // first tile of the launch: tile B covers stage-input samples [B*Vt, (B+1)*Vt)
  long long at0;         // absolute initial clock of the stage, units 1/polyL
  long long out_offset;  // preload of the destination fifo
  long long in_limit;    // stage-input samples at absolute index >= in_limit are not written yet: read as zero
  int nblocks, C, Vt, n, polyL, step, NGRP;
  int nchs, npairs;      // as DftArgs::nchs / npairs
  unsigned pps_magic;    // as DftArgs::pps_magic
};
bool polymf_supported(int ksteps);
hipError_t launch_polymf(int ksteps, const AnyView &in, const AnyView &out, const PolyMfArgs &a, hipStream_t st,
                         const char **kname = nullptr);
// element-wise copy of absolute range [a0, a1) of every channel from one fifo view to another
// (ring regrow, carrying the unconsumed tail of an in-place push into the ring, device pulls)
hipError_t launch_copy(const AnyView &in, const AnyView &out, long long a0, long long a1, int C, hipStream_t st);

} // namespace rsmp
