// Lean form of the headline kernel: dft(xL, L in {1,2}, N = 4096) -> vpoly0 on the fp64 matrix pipe, for the blocks whose
// input and output are plain interleaved float frames in one buffer each (what a device-resident push / flow of whole
// blocks looks like; rate/dft_filter.h:60-190 followed by rate/rate_filters_generic.h:272-305).
//
// Same mathematics, same summation order and the same two-round LDS sample image as fused_kernel<.., true> (fused.hip);
// what differs is the bookkeeping around it:
//   * no generic fifo addressing: the host hands over one base pointer per side (FastIo) and launches this kernel only
//     for block ranges it has checked (fused_fast_range); other blocks go to fused_kernel;
//   * the polyphase stage walks TILES (16 output residues x 4 periods = one accumulator pair) in group-major order, each
//     wave a contiguous range of them: the coefficient tile changes only when the residue group does (double-buffered,
//     requested one tile ahead of the switch), the window start of a group is a multiply-high by a host-made reciprocal
//     instead of an integer division per lane, every store is issued straight after its tile under a per-lane range test
//     (no deferred-store state, no per-step validity masks, no skip loops);
//   * the next tile's samples are always prefetched (clamped address), so the wait before a tile's MFMA chain is for
//     reads issued one whole tile earlier.
// The old kernel spent ~1200 integer / 1650 scalar instructions per wave and had 1000+ SGPR spill moves in its code;
// this one keeps the scalar state of the tile loop in a dozen registers.
#include "fft_device.hpp"
#include "fifo_device.hpp"
#include "kernels.hpp"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <type_traits>

namespace rsmp {

namespace {
typedef unsigned int rsmp_v2u __attribute__((ext_vector_type(2)));
typedef unsigned int rsmp_v4u __attribute__((ext_vector_type(4)));
// What the lean body needs to know about the sample type E of the caller-facing frames: the word that holds a frame's two
// samples of one channel pair (8 bytes of float32 frames, 16 of float64, 4 of 16-bit PCM, 8 of 32-bit PCM), the conversion of a
// loaded sample to fp64 and of a result to E (integer PCM: scale / round-to-even, saturate, narrow -- pcm_in / pcm_out*).
template <typename E> struct Frame;
template <> struct Frame<float> {
  typedef float2 P;
  static __device__ __forceinline__ double in(float s) { return (double)s; }
  static __device__ __forceinline__ float out(double y) { return (float)y; }
};
template <> struct Frame<double> {
  typedef double2 P;
  static __device__ __forceinline__ double in(double s) { return s; }
  static __device__ __forceinline__ double out(double y) { return y; }
};
template <> struct Frame<short> {
  typedef short2 P;
  static __device__ __forceinline__ double in(short s) { return pcm_in(s); }
  static __device__ __forceinline__ short out(double y) { return pcm_out16(y); }
};
template <> struct Frame<int> {
  typedef int2 P;
  static __device__ __forceinline__ double in(int s) { return pcm_in(s); }
  static __device__ __forceinline__ int out(double y) { return pcm_out32(y); }
};
// a G value (plain load).  It stays a function: written as `Gp[i]` at the call sites the same loads come out of the compiler
// with another register assignment in every instance of this file
__device__ __forceinline__ double2 load_g(const double2 *p) { return *p; }
constexpr int kPad = 32;
constexpr int kSA = kFusedSA, kSB0 = kFusedSB0;
} // namespace

// OUT64: the outputs go to the planar fp64 ring of the next stage's fifo (absolute index & mask: a ring wrap costs nothing)
// instead of interleaved float frames -- chains like 44.1k->192k, whose x2 -> 80/147 pair feeds an x4 stage.
//
// SPLIT (LOG2P = 12; kernel names fused_split_kernel<KS, OMODE> / fused_split2_kernel<KS, OMODE>): the sub-blocked form for x2
// stages whose blocks (8192 ... 32768 points) do not fit a workgroup.
// A block of the reference is nsub workgroups; each computes `len` of the block's valid samples from a 4096-point window of
// the block's inputs: y[2m + r] = IDFT_4096(DFT_4096(x) * G_r)[m], r = 0, 1 -- the block's two polyphase components, the same
// linear convolution as the reference's one long transform, in a different fp64 summation order.  One forward and two inverse
// transforms; component 0 waits in registers while component 1 is computed (256-VGPR budget: two workgroups per CU), then
// both go to ONE LDS image of the whole sub-block and the polyphase stage runs as a single round.  B counts sub-blocks, so the
// seam ring, the block table and seam_kernel work on sub-blocks exactly as they do on blocks.
// OGEN (sub-blocked form only): float frames out, each output wherever the output fifo has it -- the caller's buffer or the
// fifo's ring (RR_push without a destination, outputs beyond the caller's capacity): fifo_put for a channel pair.
// TWO (sub-blocked form, 8192-point blocks): the block is ONE workgroup -- its V samples fit a pair of 4096-point component
// transforms whole -- and the polyphase stage runs in two rounds, the second from the register slots kept across the first.
// E: the sample type of the caller-facing frames (float; double / short / int for the *_dio_kernel / *_s16_kernel / *_s32_kernel
// instances, FastIo::dio): only the frame loads and stores depend on it (Frame<E>), the arithmetic is the same fp64 code.
template <int LOG2P, int KS, bool OUT64, bool SPLIT, bool OGEN, bool TWO = false, typename E = float>
__device__ __forceinline__ void fused_fast_body(const FusedArgs &a, const FastIo &io)
{
  typedef Frame<E> Fr;
  typedef typename Fr::P E2;
  const E *const io_in = static_cast<const E *>(io.in), *const io_in_ring = static_cast<const E *>(io.in_ring);
  E *const io_out = static_cast<E *>(io.out), *const io_out_ring = static_cast<E *>(io.out_ring);
  static_assert(!TWO || SPLIT, "two rounds from registers: sub-blocked form only");
  static_assert(!SPLIT || LOG2P == 12, "sub-blocked form: 4096-point components");
  static_assert(!OGEN || (SPLIT && !OUT64), "generic float output exists for the sub-blocked form only");
  constexpr int LOG2N = 12, N = 1 << LOG2N, P = 1 << LOG2P;
  constexpr int T = N / 16, TF = P / 16;
  extern __shared__ __attribute__((aligned(16))) double lds[];

  const int tid = threadIdx.x;
  const int npairs = a.d.C >> 1; // even channel count (host-checked)
  int bl, pair;
  if (!item_map(blockIdx.x, a.d.nblocks, npairs, a.d.hp, bl, pair)) return; // uniform
  const long long B = a.d.B0 + bl;
  const int hp = io.nch >> 1, strm = pair / hp, pin = pair - strm * hp;
  SubBlock sb = {0, 0, 0, 0};
  long long e0_split = 0;
  if constexpr (SPLIT) { // (the launch starts at sub-block 0 of reference block Bref0)
    const int kr = bl / a.d.nsub;
    sb = sub_block(bl - kr * a.d.nsub, a.d.V, a.d.Vs, a.d.Pref);
    e0_split = (a.d.Bref0 + kr) * a.d.q + sb.win;
  }
  const int V = SPLIT ? sb.len : a.d.V;
  const bool fwd_active = tid < TF;
  // The block's table entry and this wave's start states of both polyphase rounds (kernels.hpp, WalkStart): wave-uniform
  // addresses in memory that no one writes while the kernel runs, so they are scalar loads (constant address space) and the
  // values live in scalar registers.  TAB_AT_START (the x2 instances of 4096-point blocks, the headline among them): requested
  // ahead of the input loads, whose latency covers them, and kept across the transforms.  The other instances have no scalar
  // registers to spare there (their transforms run at 96 - 106 of them): they request the record behind the last transform,
  // under the image writes.
  // EARLY_TILES: each round's first coefficient tile is requested ahead of the barrier(s) in front of its image.  Not in
  // the sub-blocked forms: at 252 - 256 vector registers the tile would spill component 0.
  constexpr bool TAB_AT_START = LOG2P == LOG2N - 1 && !SPLIT, EARLY_TILES = !SPLIT;
  // round A's request: ahead of the image writes where the registers allow it (7 k-steps), else between them and the barrier
  constexpr bool TILES_A_FIRST = TAB_AT_START && EARLY_TILES && KS <= 7;
  typedef const int __attribute__((address_space(4))) *TabPtr;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  struct { long long i_lo; int cnt, irel_lo, base_li; } fb; // (FusedBlock's first five dwords)
  struct RoundStart { int kb, cnt, b1, b2, p01, p02, pe1, pe2, n, g, pc, pend; }; // WalkStartRound without run 0, + this wave's entry
  RoundStart rsA, rsB;
  auto fetch_table = [&] {
    const TabPtr tb = (TabPtr)(const void *)(a.blk + bl), ts = (TabPtr)(const void *)(a.wst + bl);
    fb.i_lo = (long long)(((unsigned long long)(unsigned)tb[1] << 32) | (unsigned)tb[0]);
    fb.cnt = tb[2], fb.irel_lo = tb[3], fb.base_li = tb[4];
    auto round_start = [&](int r) {
      const TabPtr q = ts + r * (int)(sizeof(WalkStartRound) / 4), w = q + 12 + 4 * wave;
      return RoundStart{q[0], q[2], q[3], q[4], q[6], q[7], q[9], q[10], w[0], w[1], w[2], w[3]};
    };
    rsA = round_start(0);
    rsB = round_start(1);
  };
  if constexpr (TAB_AT_START) fetch_table();
  const double2 *__restrict__ Gp = a.d.G;
  double2 *smp = reinterpret_cast<double2 *>(lds) + kPad; // smp[n] = (channel A, channel B) sample n of the block
  const int nm1 = a.n - 1;

  // Builds with -DRSMP_STAMPS_BUILD (tools/build_variant.sh) + RSMP_STAMPS=1 in the environment: per-phase cycle sums of wave 0
  // (s_memtime) in one workgroup of 64, printed when the handle closes.  The product build has no trace of it: the stamp
  // points were branches (and scheduling barriers) in every workgroup.
#ifdef RSMP_STAMPS_BUILD
  const bool stamping = a.stamps && (blockIdx.x & 63) == 5;
  unsigned long long tstamp = stamping ? __builtin_readcyclecounter() : 0;
#define RSMP_STAMP(slot)                                          \
  if (stamping) {                                                  \
    const unsigned long long now = __builtin_readcyclecounter();  \
    if (tid == 0) atomicAdd(a.stamps + (slot), now - tstamp);      \
    tstamp = now;                                                  \
  }
#else
#define RSMP_STAMP(slot)
#endif

  // ---------------------------------------------------------------- load the block (fp32 -> fp64)
  // L = 2 (FWD8): the forward transform has half the points of the inverse one and runs 8 points per thread on ALL
  // waves (fft8_regs_pre); a thread then already holds the 8 distinct spectrum values Zp[tid + (s & 7) * T] its 16
  // inverse-transform inputs need, so the replication exchange disappears.
  constexpr bool FWD8 = LOG2P == LOG2N - 1;
  constexpr int NLD = FWD8 ? 8 : 16, TL = FWD8 ? T : TF; // points per loading thread, loading threads
  c64 v[16];
  c64 u8[8];
  c64 z0[SPLIT ? 16 : 1]; // sub-blocked form: component 0 of the block (samples 2m), component 1 ends up in `v`
  // its twiddles are loaded next to the block's input, G is issued two passes before it is needed
  double2 wf[FWD8 ? fft8_tw_regs(LOG2P) : 1];
  if constexpr (FWD8) fft8_tw_load<LOG2P>(wf, tid, a.d.tw_fwd8); // in flight together with the input loads below
  {
    const long long e0 = SPLIT ? e0_split : B * a.d.q;
    const bool ld_active = FWD8 || fwd_active;
    if (SPLIT && io.in_unaligned) { // (uniform) a caller's buffer that is only 4-byte aligned: the sub-blocked form has no generic
      // kernel to hand such blocks to, so it reads the two channels separately
      const E *pe = io_in + strm * io.in_stream_stride + 2 * pin, *pr = io_in_ring + strm * io.in_ring_stream_stride + 2 * pin;
#pragma unroll
      for (int s = 0; s < NLD; ++s) {
        const long long e = e0 + tid + s * TL;
        const E *f = e >= io.in_abs0 ? pe + (e - io.in_abs0) * io.nch : pr + (e & io.in_ring_mask) * io.nch;
        v[s] = {Fr::in(f[0]), Fr::in(f[1])};
      }
    } else
    if (e0 >= io.in_abs0) { // uniform: the whole block lies in the caller's buffer
      const E2 *p2 = reinterpret_cast<const E2 *>(io_in + strm * io.in_stream_stride + (e0 - io.in_abs0) * io.nch + 2 * pin);
      if (ld_active) {
#pragma unroll
        for (int s = 0; s < NLD; ++s) {
          const E2 f = p2[(unsigned)((tid + s * TL) * hp)]; // (unsigned: scalar base + 32-bit lane offset, no 64-bit address per load)
          (FWD8 ? u8[s & 7] : v[s]) = {Fr::in(f.x), Fr::in(f.y)};
        }
      }
    } else if (ld_active) { // first block of a push: its head is the previous push's tail, kept in fifo 0's ring
      const E *pe = io_in + strm * io.in_stream_stride + 2 * pin, *pr = io_in_ring + strm * io.in_ring_stream_stride + 2 * pin;
#pragma unroll
      for (int s = 0; s < NLD; ++s) {
        const long long e = e0 + tid + s * TL;
        const E2 f = *reinterpret_cast<const E2 *>(e >= io.in_abs0 ? pe + (e - io.in_abs0) * io.nch : pr + (e & io.in_ring_mask) * io.nch);
        (FWD8 ? u8[s & 7] : v[s]) = {Fr::in(f.x), Fr::in(f.y)};
      }
    }
  }
  RSMP_STAMP(0)
  // ---------------------------------------------------------------- FFT-FIR (as fused_kernel)
  if constexpr (FWD8) {
    double2 g[16];
    fft8_regs_pre<LOG2P, -1>(u8, tid, wf, lds, [&](int p) {
      if (p == 1) { // two passes (two LDS round trips) ahead of the multiplication
#pragma unroll
        for (int s = 0; s < 16; ++s) g[s] = load_g(Gp + (unsigned)(tid + s * T));
      }
    });
    RSMP_STAMP(1)
#pragma unroll
    for (int s = 0; s < 16; ++s) v[s] = cmul(u8[s & 7], c64{g[s].x, g[s].y});
    __syncthreads(); // the inverse transform's exchange reuses the LDS the forward one just read
  } else {
  fft_regs<LOG2P, -1, LOG2P == LOG2N ? 2 : 0, kPfFwd>(v, tid, fwd_active, a.d.tw_fwd, lds);
  RSMP_STAMP(1)
  if constexpr (LOG2P < LOG2N) {
    double2 g[16]; // issued before the exchange so the L2 latency overlaps it
#pragma unroll
    for (int s = 0; s < 16; ++s) g[s] = load_g(Gp + tid + s * T);
    double2 *l2 = reinterpret_cast<double2 *>(lds);
    // Z[tid + s*T] = Zp[tid + (s & 7) * T]: a forward thread (tid < TF) already holds those in its even slots; its odd
    // slots are what thread tid + TF needs
    if (fwd_active) {
#pragma unroll
      for (int u = 0; u < 8; ++u) l2[tid + u * TF] = make_double2(v[2 * u + 1].x, v[2 * u + 1].y);
    }
    __syncthreads();
    c64 z[8];
    if (fwd_active) {
#pragma unroll
      for (int u = 0; u < 8; ++u) z[u] = v[2 * u];
    } else {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const double2 q = l2[tid - TF + u * TF];
        z[u] = {q.x, q.y};
      }
    }
#pragma unroll
    for (int s = 0; s < 16; ++s) v[s] = cmul(z[s & 7], c64{g[s].x, g[s].y});
    __syncthreads();
  } else if constexpr (SPLIT) {
    // X = DFT_4096 of the window stays in `xs` for both components; component 0's samples wait in `z0`
    c64 xs[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      xs[s] = v[s];
      const double2 g = load_g(Gp + tid + s * T);
      v[s] = cmul(xs[s], c64{g.x, g.y});
    }
    fft_regs<LOG2N, +1, 2, kPfInv>(v, tid, true, a.d.tw_inv, lds);
    double2 g1[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) g1[s] = load_g(Gp + N + tid + s * T);
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      z0[s] = v[s];
      v[s] = cmul(xs[s], c64{g1[s].x, g1[s].y});
    }
    __syncthreads(); // the second inverse transform's exchange reuses the LDS the first one just read
    fft_regs<LOG2N, +1, 2, kPfInv>(v, tid, true, a.d.tw_inv, lds);
  } else {
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const double2 g = load_g(Gp + tid + s * T);
      v[s] = cmul(v[s], c64{g.x, g.y});
    }
  }
  }
  RSMP_STAMP(2)
  if constexpr (!SPLIT) fft_regs<LOG2N, +1, 2, kPfInv>(v, tid, true, a.d.tw_inv, lds);
  RSMP_STAMP(3)

  // Lane maps of v_mfma_f64_4x4x4 (tools/probe_mfma4.hip): A lane = 16k + 4b + i, B lane = 16k + 4b + j, D lane = 16i + 4b + j:
  // as an A/B lane this lane is (k = hi, block bq, i or j = jq); its D element is (row hi, block bq, period jq).
  const int hi = lane >> 4, bq = (lane >> 2) & 3, jq = lane & 3;
  const int rloc = 4 * bq + hi; // this lane's output residue within a 16-residue group
  const int ngrp = a.NGRP;
  const double2 *const cfm_lane = a.cfm2 + lane;

  // Coefficient tiles: current group, next group (in flight during the current group's last tile).  Nothing else rides on these
  // loads: the window start of a group is arithmetic (window_start below), so the only instructions that wait for a tile are
  // the ones that use its coefficients.
  // (Measured and NOT kept, round 3: two register sets used alternately group by group, all four (set, sample buffer)
  // combinations spelled out so that no set is ever copied and no s_waitcnt vmcnt(0) sits behind the prefetch -- 168 VGPRs
  // with 19 spilled across round A, 2.37 against 1.96 ms.  The kernel has no registers to spare at three workgroups per CU.)
  double cc[KS], cn[KS];
  auto load_tile = [&](int gg, double (&c_)[KS]) {
    constexpr int KSP = (KS + 1) / 2;
    const double2 *cp = cfm_lane + gg * (KSP * 64); // uniform offset; two k-steps per 16-byte load
#pragma unroll
    for (int s2 = 0; s2 < KSP; ++s2) {
      const double2 d = cp[s2 * 64];
      c_[2 * s2] = d.x;
      if (2 * s2 + 1 < KS) c_[2 * s2 + 1] = d.y;
    }
  };
  // EARLY_TILES: a round's first tile is requested AHEAD of the barrier in front of its LDS image: the group comes from the
  // table, the registers are dead there, and only the first `fill` needs the image.  Unconditional (a wave without tiles has g = 0).
  auto request_tiles = [&](const RoundStart &rs) {
    load_tile(rs.g, cc);
  };
  if constexpr (!TAB_AT_START) fetch_table();
  if constexpr (TILES_A_FIRST) request_tiles(rsA); // behind the inverse transform's last exchange, ahead of the image and its barrier


  // ---------------------------------------------------------------- stage-1 samples -> LDS (round A) and seam ring
  const int ca = 2 * pair, cb = ca + 1;
  {
    const int slot = (int)(B & a.seam_mask);
    double *seamA = a.seam + ((long long)(slot * (a.d.C + 1) + ca) * 2) * 32;
    double *seamB = a.seam + ((long long)(slot * (a.d.C + 1) + cb) * 2) * 32;
    // The head of the block goes to the seam ring from registers (slot 0); the tail is picked up from the LDS image below
    // (store_tail), where it is 23 consecutive elements -- out of registers it took per-lane range tests and a pair of
    // conditional global stores in every one of the 16 unrolled slots (V is a run-time value): ~300 scalar and ~150 vector
    // instructions per wave for 46 doubles.
    if constexpr (SPLIT && TWO) {
      __syncthreads(); // the image overlays the exchange area of the last transform
      // first image: samples [0, kSplitRaEnd) + 32 = slots 0 .. kSplitSA - 1 of both components and 16 elements of slot kSplitSA
#pragma unroll
      for (int s = 0; s <= kSplitSA; ++s) {
        const int n = 2 * (tid + s * T);
        if (n < V && (s < kSplitSA || tid < kPad / 2)) {
          smp[n] = make_double2(z0[s].x, z0[s].y);
          smp[n + 1] = make_double2(v[s].x, v[s].y);
        }
      }
      if (tid < kPad) {
        smp[tid - kPad] = make_double2(0.0, 0.0);
        if (V < kSplitRaEnd + kPad) smp[V + tid] = make_double2(0.0, 0.0);
      }
      (void)seamA; (void)seamB;
    } else if constexpr (SPLIT) {
      __syncthreads(); // the image overlays the exchange area of the last transform
      // element m of component r is sample 2 (m - shift) + r of the sub-block; the whole sub-block fits the image
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const int n = 2 * (tid + s * T - sb.shift);
        if (n >= 0 && n < V) { // (V is even)
          smp[n] = make_double2(z0[s].x, z0[s].y);
          smp[n + 1] = make_double2(v[s].x, v[s].y);
        }
      }
      if (tid < kPad) {
        smp[tid - kPad] = make_double2(0.0, 0.0);
        smp[V + tid] = make_double2(0.0, 0.0);
      }
      (void)seamA; (void)seamB;
    } else {
#pragma unroll
    for (int s = 0; s <= kSA; ++s) {
      const int n = tid + s * T;
      const bool whole = (s + 1) * T <= V;                 // every sample of this slot is valid
      if (s < kSA ? (whole || n < V) : (tid < kPad && n < V)) smp[n] = make_double2(v[s].x, v[s].y);
    }
    if (tid < nm1) {
      seamA[tid] = v[0].x;
      seamB[tid] = v[0].y;
    }
    if (tid < kPad) { // finite guard values: padded coefficients are zero, 0 * x must stay 0
      smp[tid - kPad] = make_double2(0.0, 0.0);
      if (V < kSA * T + kPad) smp[V + tid] = make_double2(0.0, 0.0);
    }
    }
  }
  if constexpr (EARLY_TILES && !TILES_A_FIRST) request_tiles(rsA); // (the image writes cover the table's round trip)
  __syncthreads();
  if constexpr (SPLIT) { // the head goes to the seam ring from the image (its register slot depends on the sub-block's shift)
    if (tid < nm1) {
      const int slot = (int)(B & a.seam_mask);
      const double2 t = smp[tid];
      a.seam[((long long)(slot * (a.d.C + 1) + ca) * 2) * 32 + tid] = t.x;
      a.seam[((long long)(slot * (a.d.C + 1) + cb) * 2) * 32 + tid] = t.y;
    }
  }
  // the block's last n-1 samples -> seam ring, read back from whichever LDS image holds them (element 0 of `img` = sample n0)
  const int tail0 = V - nm1;
  auto store_tail = [&](const double2 *img, int n0) {
    if (tid < nm1) {
      const int slot = (int)(B & a.seam_mask);
      const double2 t = img[tail0 + tid - n0];
      a.seam[((long long)(slot * (a.d.C + 1) + ca) * 2 + 1) * 32 + tid] = t.x;
      a.seam[((long long)(slot * (a.d.C + 1) + cb) * 2 + 1) * 32 + tid] = t.y;
    }
  };
  // uniform: else the whole tail lies inside the first image (V <= kSB0 * T + n - 1)
  const bool tail_in_b = TWO ? tail0 >= kSplitRbStart : (!SPLIT && tail0 >= kSB0 * T);
  if (!tail_in_b) store_tail(smp, 0);
  RSMP_STAMP(4)

  // ---------------------------------------------------------------- polyphase FIR on v_mfma_f64_4x4x4, tile by tile
  const int pl = a.polyL, step = a.step;
  const int frame_bytes = io.nch * (int)sizeof(E);
  char *const obytes = (OUT64 || OGEN) ? nullptr
                            : reinterpret_cast<char *>(io_out + strm * io.out_stream_stride + (a.out_offset2 + fb.i_lo - io.out_abs0) * io.nch + 2 * pin);
  // OGEN: absolute index (in the output fifo) of the block's output 0, this pair's slot of a frame in either buffer
  const long long oabs0 = a.out_offset2 + fb.i_lo;
  E *const oext = OGEN ? io_out + strm * io.out_stream_stride + 2 * pin : nullptr;
  E *const oring = OGEN ? io_out_ring + strm * io.out_ring_stream_stride + 2 * pin : nullptr;
  // OUT64: one descriptor per channel over its whole ring; output ib of the block sits at ring slot (o64 + ib) & mask
  const unsigned o64 = OUT64 ? (unsigned)((a.out_offset2 + fb.i_lo) & io.out64_mask) : 0u;
  const unsigned m64 = (unsigned)io.out64_mask;
  __amdgpu_buffer_rsrc_t orsrcA, orsrcB;
  if constexpr (OUT64) {
    double *ra = io.out64 + (long long)(2 * pair) * io.out64_chan_stride;
    orsrcA = __builtin_amdgcn_make_buffer_rsrc(ra, 0, (int)((io.out64_mask + 1) * 8), 0x00020000);
    orsrcB = __builtin_amdgcn_make_buffer_rsrc(ra + io.out64_chan_stride, 0, (int)((io.out64_mask + 1) * 8), 0x00020000);
  }
  // Every group walks its OWN periods (kernels.hpp, FusedWalk): group g starts at period kb + p0_g, p0_g = 1 when all its
  // residues lie in front of the block's first output, and has ncs_g column steps of 4 periods, one less than its neighbours
  // when it ends a period early.  `pc` counts periods from kb: p0_g, p0_g + 4, ... up to `pend` = p0_g + 4 ncs_g.
  // The round's and the wave's start state is the table's (RoundStart, in scalar registers since the kernel began); what is
  // left to do behind the barrier are the per-lane terms and the buffer descriptor.
  auto poly_round = [&](const RoundStart &rs, const double2 *xs, int li_lo, int li_hi) {
    if (rs.n == 0) return; // the round does not exist, or has no tile for this wave
    if constexpr (!EARLY_TILES) request_tiles(rs);
    const int kb = rs.kb;
    int g = rs.g, pc = rs.pc, pend = rs.pend;
    int p0 = pc & 3; // the current group's first period (pc = p0 + 4 column steps, p0 < 2), then the next group's
    // (a first round that stops short of K ends at period ke for the groups that start at 0 and at ke + 1 for the others)
    const int lane_li = walk_lane_li(fb.base_li, kb, hi, jq, step); // window start = lane_li + q(group, block) + pc * step
    const int lane_ib = walk_lane_ib(fb.irel_lo, kb, jq, rloc, pl); // output index relative to i_lo = lane_ib + 16 g + pc * pl
    const int cnt = rs.cnt;
    // raw buffer over this round's outputs [0, cnt) of the block: frame ib at byte ib * frame_bytes, 8 (16) bytes of it are ours
    // (the range check is done by the descriptor: no per-tile compare / branch)
    const __amdgpu_buffer_rsrc_t orsrc =
        __builtin_amdgcn_make_buffer_rsrc(obytes, 0, (!OUT64 && !OGEN && cnt > 0) ? (cnt - 1) * frame_bytes + 2 * (int)sizeof(E) : 0, 0x00020000);
    // store offset of a tile = (this lane's part, once per round) + (the tile's part, scalar): one vector add per tile.  Only the
    // last residue group can hold residues >= polyL (polyL not a multiple of 16): its lanes get the dropped offset there.
    const int lane_off0 = __mul24(lane_ib, frame_bytes); // |lane_ib| < 2^23
    const bool lane_dead_last = 16 * (ngrp - 1) + rloc >= pl;
    // q(group, this lane's block) + lane_li (kernels.hpp, walk_q_table / walk_q_rcp): a handful of 32-bit vector instructions where
    // a group becomes current, no memory access -- as a value that came with the coefficient tile (or from qtab) its use was a
    // wait for every vector-memory operation in flight, the output stores of the tiles before it among them
    auto window_start = [&](int gg) {
      unsigned num = (unsigned)a.at0 + (unsigned)((16 * gg + 4 * bq) * step);
      if (gg == ngrp - 1 && (pl & 15)) num = 16 * gg + 4 * bq >= pl ? (unsigned)a.at0 : num; // uniform: idle blocks of a partial last group
      return walk_q_rcp(num, a.rcp_m, a.rcp_s) + lane_li;
    };

    double2 x0[KS], x1[KS];
    auto fill = [&](double2 (&x)[KS], int q, int pstep) {
      const int li = max(li_lo, min(li_hi, q + pstep * step)); // (q = lane_li + the group's window start)
      const double2 *xp = xs + li;
#pragma unroll
      for (int s = 0; s < KS; ++s) x[s] = xp[4 * s];
    };
    // (lane_li is added where qc changes, at the group switch: one vector add per tile for the window address, as before)
    int qc = window_start(g);
    fill(x0, qc, pc);
    // the round's first tile has arrived before the loop is entered: left to the first use inside the loop, the wait (counted from
    // the loop's entry) stands in every tile, where it counts output stores as if they were this load
    asm volatile("" : "+v"(cc[KS - 1]));

    int left = rs.n;
    // one tile: prefetch the next tile's samples into `xn`, run the two accumulation chains on `xc`, store
    auto tile = [&](const double2 (&xc)[KS], double2 (&xn)[KS]) {
      // (loop control in plain ints: uniform bools that live across blocks came back as v_cndmask / v_readfirstlane pairs)
      // (and every condition is recomputed from them where it is used: carried from one block to the next it takes a trip through
      // a vector register)
      // wrap = 1 when this is its group's last tile (pc + 4 == pend), by arithmetic the optimiser cannot see through: as a compare
      // (+ select) it widens the flag through a vector register (v_cndmask, v_readfirstlane, v_cmp_ne) in every tile
      int wrap;
      asm("s_lshr_b32 %0, %1, 31" : "=s"(wrap) : "s"(pend - 8 - pc));
      const int gnext = g + wrap;
      int pnext = pc + 4, pend_next = pend;
      if (wrap != 0 && left > 1) { // uniform.  Volatile so that it STAYS a branch: as a select the conversion runs in every tile and the
                          // tile right behind a switch waits for the tile load that was just issued
        qc = window_start(gnext);
        asm volatile("" : "+v"(qc)); // (keeps the arithmetic inside the branch)
        // the next group's first period and column steps: they differ from this group's only where a run of groups ends
        // (WalkRound: twice per round at most, never in the uniform walk), so a group switch costs two scalar compares
        // (walk_next_group, on the table's run values)
        if (gnext == rs.b2) p0 = rs.p02, pend_next = rs.pe2;
        else if (gnext == rs.b1) p0 = rs.p01, pend_next = rs.pe1;
        pnext = p0;
        // The next group's coefficient tile, requested at the head of this group's last tile: between the request and the copy at
        // the tile's end lies exactly one output store on every path, so the waits of the copy are counted for the loads alone
        // (vmcnt = the loads still behind + that store).  (`cn` is dead here: the previous switch copied it.  Requested a whole
        // group ahead, behind the copy, the loads had the group's stores behind them, one per tile, which the compiler cannot
        // count: its vmcnt(1) in front of the last copy then waited for every store but the newest.)
        load_tile(gnext, cn);
      }
      fill(xn, qc, left > 1 ? pnext : pc); // after the last tile: a harmless re-read
      double accA = 0.0, accB = 0.0;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        accA = __builtin_amdgcn_mfma_f64_4x4x4f64(cc[s], xc[s].x, accA, 0, 0, 0);
        accB = __builtin_amdgcn_mfma_f64_4x4x4f64(cc[s], xc[s].y, accB, 0, 0, 0);
      }
      (void)x0; // (names `x0` so that it stays among this lambda's captures, behind `cc`: without it the instances with an odd KS
                // get another register assignment)
      const int ib = lane_ib + 16 * g + pc * pl;
      if constexpr (OGEN) {
        if ((unsigned)ib < (unsigned)cnt && 16 * g + rloc < pl) {
          const long long A = oabs0 + ib;
          E *const p = (A >= io.out_abs0 && A < io.out_end) ? oext + (A - io.out_abs0) * io.nch : oring + (A & io.out_ring_mask) * io.nch;
          if (io.out_unaligned) { // (uniform) a caller's buffer that is only aligned for one sample, not for a pair
            p[0] = Fr::out(accA);
            p[1] = Fr::out(accB);
          } else
            *reinterpret_cast<E2 *>(p) = E2{Fr::out(accA), Fr::out(accB)};
        }
      } else if constexpr (OUT64) {
        // (the descriptor spans the ring, so the block's range test is explicit here; lanes that fail it get an offset
        // behind the ring and the hardware drops their stores)
        const bool ok = (unsigned)ib < (unsigned)cnt && 16 * g + rloc < pl;
        const unsigned off = ok ? ((o64 + (unsigned)ib) & m64) * 8u : 0xffffffffu;
        const rsmp_v2u da = {(unsigned)__double2loint(accA), (unsigned)__double2hiint(accA)};
        const rsmp_v2u db = {(unsigned)__double2loint(accB), (unsigned)__double2hiint(accB)};
        __builtin_amdgcn_raw_buffer_store_b64(da, orsrcA, (int)off, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b64(db, orsrcB, (int)off, 0, 0);
      } else {
        // one unconditional buffer store per tile: outputs in front of the block (ib < 0 wraps to a huge offset) and behind
        // the round's last one fail the descriptor's range check and are dropped by the hardware; only the residue test of
        // the last (partial) group needs a select
        unsigned off = (unsigned)(lane_off0 + (16 * g + pc * pl) * frame_bytes);
        if (g == ngrp - 1 && (pl & 15)) { // uniform, and only chains whose polyL is not a multiple of 16 ever take it
          off = lane_dead_last ? 0xffffffffu : off;
          asm volatile("" : "+v"(off)); // (keeps it a branch: as selects it is two more vector instructions in every tile)
        }
        if constexpr (sizeof(E) == 8) { // float64 frames: the pair as one 16-byte store
          const rsmp_v4u d = {(unsigned)__double2loint(accA), (unsigned)__double2hiint(accA), (unsigned)__double2loint(accB),
                              (unsigned)__double2hiint(accB)};
          __builtin_amdgcn_raw_buffer_store_b128(d, orsrc, (int)off, 0, 0);
        } else if constexpr (sizeof(E) == 2) { // 16-bit PCM frames: the pair as one 4-byte store
          __builtin_amdgcn_raw_buffer_store_b32(pcm_pack16(accA, accB), orsrc, (int)off, 0, 0);
        } else if constexpr (std::is_same<E, int>::value) { // 32-bit PCM frames: one 8-byte store
          const rsmp_v2u d = {(unsigned)pcm_out32(accA), (unsigned)pcm_out32(accB)};
          __builtin_amdgcn_raw_buffer_store_b64(d, orsrc, (int)off, 0, 0);
        } else {
          const rsmp_v2u d = {__float_as_uint((float)accA), __float_as_uint((float)accB)};
          __builtin_amdgcn_raw_buffer_store_b64(d, orsrc, (int)off, 0, 0);
        }
      }
      if (wrap != 0 && left > 1) { // uniform: the group switches
#pragma unroll
        for (int s = 0; s < KS; ++s) asm volatile("v_mov_b64 %0, %1" : "=v"(cc[s]) : "v"(cn[s]));
      }
      g = gnext;
      pc = pnext;
      pend = pend_next;
      --left;
    };
    // Pairs of tiles in a loop with ONE exit, an odd last tile behind it.  (With a second exit between the two tiles the compiler
    // routes both through one block that also leads back to the loop's head -- an edge that is never taken, on which the reads
    // into `x1` are still pending: every register it reuses from `x1` for an address in the first tile then costs an
    // s_waitcnt lgkmcnt(0) there, in the middle of the tile's MFMA chain.)
    while (left >= 2) {
      tile(x0, x1);
      tile(x1, x0);
    }
    if (left != 0) tile(x0, x1);
  };

  const bool run = fb.cnt > 0;
  // round A: periods whose windows end inside the samples written above
  if constexpr (SPLIT && TWO) {
    if (run) poly_round(rsA, smp, -kPad, min(V, kSplitRaEnd) + kPad - 4 * KS);
    if constexpr (EARLY_TILES) request_tiles(rsB);
    __syncthreads();
    { // second image: samples [kSplitRbStart, V) from the slots kept in registers, element 0 = sample kSplitRbStart
      double2 *l2 = reinterpret_cast<double2 *>(lds);
#pragma unroll
      for (int s = kSplitSB0; s < 16; ++s) {
        const int n = 2 * (tid + s * T);
        if (n < V) {
          l2[n - kSplitRbStart] = make_double2(z0[s].x, z0[s].y);
          l2[n + 1 - kSplitRbStart] = make_double2(v[s].x, v[s].y);
        }
      }
      if (tid < kPad && V > kSplitRbStart) l2[V - kSplitRbStart + tid] = make_double2(0.0, 0.0);
    }
    __syncthreads();
    if (tail_in_b) store_tail(reinterpret_cast<const double2 *>(lds), kSplitRbStart);
    if (run) poly_round(rsB, reinterpret_cast<const double2 *>(lds) - kSplitRbStart, kSplitRbStart, V + kPad - 4 * KS);
    return;
  } else if constexpr (SPLIT) {
    if (run) poly_round(rsA, smp, -kPad, V + kPad - 4 * KS); // one round over the whole image (the table's first round is [0, K))
    return;
  }
  if (run) poly_round(rsA, smp, -kPad, min(V, kSA * T) + kPad - 4 * KS);
  if constexpr (EARLY_TILES) request_tiles(rsB); // straight after this wave's last tile of round A, ahead of both barriers
  RSMP_STAMP(6)
  __syncthreads();
  // round B: the rest of the block's samples replace the image, element 0 = sample kSB0*T
  {
    double2 *l2 = reinterpret_cast<double2 *>(lds);
#pragma unroll
    for (int s = kSB0; s < 16; ++s) {
      const int n = tid + s * T;
      if (n < V) l2[n - kSB0 * T] = make_double2(v[s].x, v[s].y);
    }
    if (tid < kPad && V > kSB0 * T) l2[V - kSB0 * T + tid] = make_double2(0.0, 0.0);
  }
  __syncthreads();
  if (tail_in_b) store_tail(reinterpret_cast<const double2 *>(lds), kSB0 * T);
  if (run) poly_round(rsB, reinterpret_cast<const double2 *>(lds) - kSB0 * T, kSB0 * T, V + kPad - 4 * KS);
  RSMP_STAMP(5)
#ifdef RSMP_STAMPS_BUILD
  if (stamping && tid == 0) atomicAdd(a.stamps + 7, 1ull);
#endif
#undef RSMP_STAMP
}

// (thin kernels around one body, so that the lean kernel keeps the name its profiles are filed under)
template <int LOG2P, int KS, bool OUT64>
__global__ __launch_bounds__(256, kFusedWaves) void fused_fast_kernel(FusedArgs a, FastIo io)
{
  fused_fast_body<LOG2P, KS, OUT64, false, false>(a, io);
}
// OMODE: 0 = float frames straight into the caller's buffer, 1 = the next fifo's fp64 ring, 2 = float frames via the fifo (OGEN)
template <int KS, int OMODE>
__global__ __launch_bounds__(256, 2) void fused_split_kernel(FusedArgs a, FastIo io)
{
  fused_fast_body<12, KS, OMODE == 1, true, OMODE == 2>(a, io);
}
// whole 8192-point blocks, polyphase stage in two rounds from registers (TWO)
template <int KS, int OMODE>
__global__ __launch_bounds__(256, 2) void fused_split2_kernel(FusedArgs a, FastIo io)
{
  fused_fast_body<12, KS, OMODE == 1, true, OMODE == 2, true>(a, io);
}

// the same three around the float64-frame body (FastIo::dio)
template <int LOG2P, int KS, bool OUT64>
__global__ __launch_bounds__(256, kFusedWaves) void fused_fast_dio_kernel(FusedArgs a, FastIo io)
{
  fused_fast_body<LOG2P, KS, OUT64, false, false, false, double>(a, io);
}
template <int KS, int OMODE>
__global__ __launch_bounds__(256, 2) void fused_split_dio_kernel(FusedArgs a, FastIo io)
{
  fused_fast_body<12, KS, OMODE == 1, true, OMODE == 2, false, double>(a, io);
}
template <int KS, int OMODE>
__global__ __launch_bounds__(256, 2) void fused_split2_dio_kernel(FusedArgs a, FastIo io)
{
  fused_fast_body<12, KS, OMODE == 1, true, OMODE == 2, true, double>(a, io);
}

// and around the integer PCM bodies
#define RSMP_PCM_KERNELS(tag, E)                                                                                          \
  template <int LOG2P, int KS, bool OUT64>                                                                                \
  __global__ __launch_bounds__(256, kFusedWaves) void fused_fast_##tag##_kernel(FusedArgs a, FastIo io)                  \
  {                                                                                                                       \
    fused_fast_body<LOG2P, KS, OUT64, false, false, false, E>(a, io);                                                     \
  }                                                                                                                       \
  template <int KS, int OMODE> __global__ __launch_bounds__(256, 2) void fused_split_##tag##_kernel(FusedArgs a, FastIo io) \
  {                                                                                                                       \
    fused_fast_body<12, KS, OMODE == 1, true, OMODE == 2, false, E>(a, io);                                               \
  }                                                                                                                       \
  template <int KS, int OMODE> __global__ __launch_bounds__(256, 2) void fused_split2_##tag##_kernel(FusedArgs a, FastIo io) \
  {                                                                                                                       \
    fused_fast_body<12, KS, OMODE == 1, true, OMODE == 2, true, E>(a, io);                                                \
  }
RSMP_PCM_KERNELS(s16, short)
RSMP_PCM_KERNELS(s32, int)
#undef RSMP_PCM_KERNELS

typedef void (*FastKernel)(FusedArgs, FastIo);

template <int LOG2P, int KS, bool OUT64> static hipError_t launch_fast_t(const FusedArgs &a, const FastIo &io, hipStream_t st)
{
  constexpr int N = 4096;
  size_t lds_bytes = 8 * size_t(fft_lds_doubles_halves(12));
  if (LOG2P < 12) lds_bytes = std::max(lds_bytes, 8 * size_t(std::max(fft_lds_doubles(LOG2P), fft8_lds_doubles(LOG2P))));
  lds_bytes = std::max(lds_bytes, size_t(kPad + kSA * (N / 16) + kPad) * 16);
  static DynLdsOnce attr[4];
  static const FastKernel fns[4] = {&fused_fast_kernel<LOG2P, KS, OUT64>, &fused_fast_dio_kernel<LOG2P, KS, OUT64>,
                                    &fused_fast_s16_kernel<LOG2P, KS, OUT64>, &fused_fast_s32_kernel<LOG2P, KS, OUT64>};
  if (io.dio < 0 || io.dio > 3) return hipErrorInvalidValue;
  if (hipError_t e = attr[io.dio].set(reinterpret_cast<const void *>(fns[io.dio]), int(lds_bytes)); e != hipSuccess) return e;
  FusedArgs b = a;
  b.d.hp = io.nch >= 4 ? io.nch / 2 : 0;
  dim3 grid(item_grid(a.d.nblocks, a.d.C / 2, b.d.hp)), block(N / 16);
  hipLaunchKernelGGL(fns[io.dio], grid, block, lds_bytes, st, b, io);
  return hipGetLastError();
}

template <int KS, int OMODE, bool TWO> static hipError_t launch_split_t(const FusedArgs &a, const FastIo &io, hipStream_t st)
{
  // the image of the longest sub-block (TWO: the first image, the longer of the two), or the exchange area of the
  // transforms, whichever is larger: <= 80 KB, two per CU
  const size_t lds_max = std::max(size_t(8) * fft_lds_doubles_halves(12), size_t(kPad + (TWO ? kSplitRaEnd : kSplitVsMax) + kPad) * 16);
  const size_t lds_bytes = TWO ? lds_max : std::max(size_t(8) * fft_lds_doubles_halves(12), size_t(kPad + a.d.Vs + kPad) * 16);
  static DynLdsOnce attr[4];
  static const FastKernel fns[4] = {
      TWO ? &fused_split2_kernel<KS, OMODE> : &fused_split_kernel<KS, OMODE>, TWO ? &fused_split2_dio_kernel<KS, OMODE> : &fused_split_dio_kernel<KS, OMODE>,
      TWO ? &fused_split2_s16_kernel<KS, OMODE> : &fused_split_s16_kernel<KS, OMODE>, TWO ? &fused_split2_s32_kernel<KS, OMODE> : &fused_split_s32_kernel<KS, OMODE>};
  if (io.dio < 0 || io.dio > 3) return hipErrorInvalidValue;
  if (hipError_t e = attr[io.dio].set(reinterpret_cast<const void *>(fns[io.dio]), int(lds_max)); e != hipSuccess) return e;
  FusedArgs b = a;
  b.d.hp = io.nch >= 4 ? io.nch / 2 : 0;
  dim3 grid(item_grid(a.d.nblocks, a.d.C / 2, b.d.hp)), block(256);
  hipLaunchKernelGGL(fns[io.dio], grid, block, lds_bytes, st, b, io);
  return hipGetLastError();
}

// V samples of an 8192-point block in two LDS images: the second must reach the block's end, and every 4-residue block's
// windows (spread qb_spread samples) must fit the overlap of the two
bool fused_split_two_supported(int V, int taps, int ksteps, int qb_spread)
{
  return !knobs().no_split2 && !(V & 1) && V == 8192 - (taps - 1) && V > kSplitVsMax && V - kSplitRbStart + kPad <= kSplitRaEnd + kPad &&
         qb_spread + 4 * ksteps + 4 <= kSplitRaEnd - kSplitRbStart + kPad && ksteps >= 7 && ksteps <= 9;
}

bool fused_split_supported(int log2n, int L, int ksteps)
{
  return !knobs().no_fast && !knobs().no_split && L == 2 && log2n >= 13 && log2n <= 15 && ksteps >= 7 && ksteps <= 9;
}

hipError_t launch_fused_split(int omode, const FusedArgs &a, const FastIo &io, hipStream_t st, const char **kname)
{
  // what the kernel's indexing assumes, checked where the launch is made
  if (!a.blk || !a.wst) return hipErrorInvalidValue;
  if (a.d.two) { // whole 8192-point blocks: one "sub-block" per block, two rounds
    if (a.d.nsub != 1 || a.d.Vs != a.d.V || a.d.Pref != 4096 || a.d.V <= kSplitVsMax || a.d.V > 8192 || (a.d.V & 1)) return hipErrorInvalidValue;
  } else if (a.d.Vs > kSplitVsMax) return hipErrorInvalidValue;
  if (a.d.nsub < 1 || a.d.Vs < 64 || (a.d.Vs & 1) || (a.d.V & 1) || a.d.nblocks % a.d.nsub || omode < 0 || omode > 2 ||
      (omode == 1 ? !io.out64 : omode == 2 ? !io.out_ring : !io.out) ||
      (a.d.Pref != 4096 && a.d.Pref != 8192 && a.d.Pref != 16384) || a.d.nsub * a.d.Vs < a.d.V || (a.d.nsub - 1) * a.d.Vs >= a.d.V || (io.nch & 1))
    return hipErrorInvalidValue;
  for (int i = 0; i < a.d.nsub; ++i) { // every sub-block's samples must be free of the component transforms' wrap-around
    const SubBlock sb = sub_block(i, a.d.V, a.d.Vs, a.d.Pref);
    const int ov = 2 * a.d.Pref - a.d.V; // taps - 1
    if (sb.win < 0 || sb.shift < 0 || sb.shift + sb.len / 2 + (ov + 1) / 2 > 4096 || (sb.len & 1) || sb.win + 4096 > a.d.Pref) return hipErrorInvalidValue;
  }
// the instance's name by sample format (FastIo::dio), as rocprofv3 prints it
#define RSMP_IO_NAME(fmt, head, tail) \
  ((fmt) == 1 ? head "_dio_" tail : (fmt) == 2 ? head "_s16_" tail : (fmt) == 3 ? head "_s32_" tail : head "_" tail)
#define RSMP_SPLIT_CASE(ks, om)                                                        \
  if (a.KS == ks && omode == om && !a.d.two) {                                         \
    if (kname) *kname = RSMP_IO_NAME(io.dio, "rsmp::fused_split", "kernel<" #ks ", " #om ">");  \
    return launch_split_t<ks, om, false>(a, io, st);                                   \
  }                                                                                    \
  if (a.KS == ks && omode == om && a.d.two) {                                          \
    if (kname) *kname = RSMP_IO_NAME(io.dio, "rsmp::fused_split2", "kernel<" #ks ", " #om ">"); \
    return launch_split_t<ks, om, true>(a, io, st);                                    \
  }
  // (9 k-steps: 80 phases at step 147, the windows of a 4-residue block spread over 34 samples)
  RSMP_SPLIT_CASE(7, 0) RSMP_SPLIT_CASE(7, 1) RSMP_SPLIT_CASE(7, 2) RSMP_SPLIT_CASE(8, 0) RSMP_SPLIT_CASE(8, 1) RSMP_SPLIT_CASE(8, 2)
  RSMP_SPLIT_CASE(9, 0) RSMP_SPLIT_CASE(9, 1) RSMP_SPLIT_CASE(9, 2)
#undef RSMP_SPLIT_CASE
  return hipErrorInvalidValue;
}

// poly_round's walk restated on the host, slot by slot, for the tile-walk tests (RRX_debug_tile_walk): the block's table
// entry and its start-state record come from the functions fused_prep_kernel uses (fused_block_info, fused_walk_start: each
// round's output count, each wave's first tile and tile count, the runs' values), the group switch is the kernel's
// (walk_next_group), and so are a lane's window start and output index (walk_lane_li, walk_lane_ib); a slot is one lane of
// one tile.
size_t fused_walk_enumerate(const FusedPrepArgs &p, int k, long long *head, int *slots, size_t cap)
{
  const FusedBlock fb = fused_block_info(p, k);
  const int pl = p.polyL, step = p.step, ngrp = (pl + 15) >> 4;
  const FusedWalk fw = fused_walk(fb, ngrp);
  const FusedWalk uni = {0, ngrp, fb.KA};
  const long long h[13] = {fb.i_lo, fb.cnt, fb.K, fb.KA, fb.walk < 0, fw.g_lo, fw.g_hi, fw.ka,
                           fb.cnt > 0 ? fused_walk_tiles(fw, fb.K, ngrp) : 0, fb.cnt > 0 ? fused_walk_tiles(uni, fb.K, ngrp) : 0,
                           fb.irel_lo, fb.base_li, ngrp};
  for (int i = 0; i < 13; ++i) head[i] = h[i];
  size_t n = 0;
  if (fb.cnt <= 0) return 0;
  const WalkStart ws = fused_walk_start(fb, ngrp, pl); // what fused_prep_kernel puts beside the entry, and all the kernels start from
  WalkRcp rcp = {0, 0, 0};
  const bool have_rcp = walk_rcp(p.at0, step, pl, rcp); // (without one the engine refuses the lean kernels: the plain quotient then)
  for (int round = 0; round < 2; ++round) {
    const WalkStartRound &r = ws.r[round];
    const int kb = r.kb, cnt = r.cnt;
    for (int wave = 0; wave < 4; ++wave) {
      int g = r.w[wave].g, pc = r.w[wave].pc, pend = r.w[wave].pend, p0 = pc & 3;
      for (int left = r.w[wave].n; left > 0; --left) { // (the kernel takes them in pairs and an odd last one: the same sequence)
        for (int lane = 0; lane < 64; ++lane) {
          const int hi = lane >> 4, bq = (lane >> 2) & 3, jq = lane & 3, rloc = 4 * bq + hi;
          // window start of the 4-residue block as poly_round's window_start forms it: numerator, multiply-high, shift
          const unsigned num = unsigned(p.at0) + unsigned(walk_q_rb(g, bq, pl) * step);
          const int q = have_rcp ? walk_q_rcp(num, rcp.m, rcp.s) : walk_q_table(p.at0, step, pl, g, bq);
          const int li = walk_lane_li(fb.base_li, kb, hi, jq, step) + q + pc * step;
          const int ib = walk_lane_ib(fb.irel_lo, kb, jq, rloc, pl) + 16 * g + pc * pl;
          if (n < cap) {
            int *o = slots + 7 * n;
            o[0] = round, o[1] = g, o[2] = (pc - p0) >> 2, o[3] = lane, o[4] = ib;
            o[5] = ib >= 0 && ib < cnt && 16 * g + rloc < pl;
            o[6] = li;
          }
          ++n;
        }
        if (pc + 4 == pend) { // the group's last tile: the kernel's group switch
          ++g;
          walk_next_group(r, g, p0, pend);
          pc = p0;
        } else
          pc += 4;
      }
    }
  }
  return n;
}

// the window start of (group, block) both ways: as the lean kernels compute it and as qtab holds it; false = no reciprocal
bool fused_window_start_host(long long at0, int step, int pl, int g, int bq, int *arith, int *table, unsigned *rcp3)
{
  WalkRcp r;
  if (!walk_rcp(at0, step, pl, r)) return false;
  const unsigned num = unsigned(at0) + unsigned(walk_q_rb(g, bq, pl) * step);
  *arith = walk_q_rcp(num, r.m, r.s);
  *table = walk_q_table(at0, step, pl, g, bq);
  rcp3[0] = r.m, rcp3[1] = unsigned(r.s), rcp3[2] = r.nmax;
  return true;
}

void fused_walk_start_host(const FusedPrepArgs &p, int k, int *out56)
{
  static_assert(sizeof(WalkStart) == 56 * sizeof(int), "WalkStart as 56 ints");
  const WalkStart ws = fused_walk_start(fused_block_info(p, k), (p.polyL + 15) >> 4, p.polyL);
  memcpy(out56, &ws, sizeof ws);
}

bool fused_fast_supported(int log2n, int log2p, int ksteps)
{
  return !knobs().no_fast && log2n == 12 && (log2p == 11 || log2p == 12) && (ksteps == 7 || ksteps == 8);
}

#define RSMP_FAST_CASE(p, ks)                                                                        \
  if (log2p == p && a.KS == ks) {                                                                    \
    if (kname) *kname = io.out64 ? RSMP_IO_NAME(io.dio, "rsmp::fused_fast", "kernel<" #p ", " #ks ", true>") \
                                 : RSMP_IO_NAME(io.dio, "rsmp::fused_fast", "kernel<" #p ", " #ks ", false>"); \
    return io.out64 ? launch_fast_t<p, ks, true>(a, io, st) : launch_fast_t<p, ks, false>(a, io, st); \
  }

hipError_t launch_fused_fast(int log2p, const FusedArgs &a, const FastIo &io, hipStream_t st, const char **kname)
{
  if (!a.blk || !a.wst) return hipErrorInvalidValue; // the block table and its start-state records (fused_prep_kernel)
  RSMP_FAST_CASE(11, 7) RSMP_FAST_CASE(12, 7) RSMP_FAST_CASE(11, 8) RSMP_FAST_CASE(12, 8)
  return hipErrorInvalidValue;
}

} // namespace rsmp
