/* ratelib_amd.h -- additive extensions of the ratelib.h C ABI for GPU-resident data and for many
 * independent streams per handle.  Nothing here exists in the reference; the closest reference
 * interfaces are cited so a maintainer can see what each call generalises.
 *
 * A "batch" handle holds `nstreams` independent streams of `nchannels` channels each, all with the
 * same RR_config and all pushed in lock step (the reference would use nstreams separate handles:
 * rate/rate_base.h:533-540 makes every channel an independent rate_t already).  Buffers are laid out
 * [stream][frame][channel]; `*_stride` is the distance between consecutive streams in FRAMES.
 */
#ifndef RATELIB_AMD_H
#define RATELIB_AMD_H

#include "ratelib.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Generalises RR_open (rate/ratelib.h:74) to nstreams lock-stepped streams. RR_push/RR_pull/RR_flow
 * on such a handle use packed host buffers (stride = the frame count of the call).
 * Every stream's output is bit-identical to what a handle of its own produces, for even and odd channel counts
 * alike: the channel pairs that share a complex transform never straddle two streams (with an odd count the last
 * channel of each stream rides alone, exactly as in a one-stream handle).
 * nchannels * nstreams above 524 287 is RR_ENOMEM before anything is allocated.  An odd nchannels is RR_INVPARAM where
 * streams * pairs-per-stream^2 exceeds 2^32 with pairs-per-stream = (nchannels + 1) / 2 (RR_open: 131 073 channels or more). */
int RRX_open_batch(const RR_config *config, int nchannels, int nstreams, RR_handle **const handle);

/* Devices.  A handle lives on ONE HIP device: all of its memory, streams and launches.  Every entry point of both headers
 * selects that device for the duration of the call and restores the caller's afterwards, so a handle may be used from any
 * thread whatever device that thread has current (one thread at a time per handle, as in the reference: SURVEY 8b).
 *   RR_open / RRX_open_batch place the handle on the calling thread's current device, or -- when the environment variable
 *   RATELIB_AMD_DEVICES ("all", or a comma list of device indices) was set at init_ratelib -- deal new handles round-robin
 *   over those devices: the unchanged plugin, one process with one handle per converter thread (chain.h:36), then spreads
 *   over the GPUs of a node by itself (channels / streams are independent, rate/rate_base.h:533-540: no collective).
 *   RRX_open_batch_on names the device explicitly: RR_INVPARAM for an index the process does not have (or < 0),
 *   RR_EXTUNINIT for a device that is not gfx950.
 * Device pointers handed to RRX_*_device must be accessible from the handle's device; RRX_device reports it (-1: NULL). */
int RRX_open_batch_on(const RR_config *config, int nchannels, int nstreams, int device, RR_handle **const handle);
int RRX_device(const RR_handle *h);

/* Device-pointer forms of RR_push / RR_pull / RR_flow (rate/ratelib.h:75-77).  Pointers are HBM
 * addresses valid on the handle's HIP stream; calls only enqueue work (no host synchronisation),
 * the frame counts they return are exact because availability never depends on sample values.
 * RRX_flow_device consumes the input in place and writes new output straight into d_obuf.
 * Ordering is the caller's: whatever filled d_ibuf (or last wrote d_obuf, e.g. a zero fill) on ANOTHER stream must have
 * completed, or be ordered before the handle's stream by an event, when the call is made; work on the handle's own
 * stream (RRX_set_stream) is ordered by the stream itself. */
int RRX_push_device(RR_handle *h, const fb_sample_t *d_ibuf, size_t in_stride, size_t isamp);
int RRX_pull_device(RR_handle *h, fb_sample_t *d_obuf, size_t out_stride, size_t osamp, size_t *ogen);
int RRX_flow_device(RR_handle *h, const fb_sample_t *d_ibuf, size_t in_stride, fb_sample_t *d_obuf, size_t out_stride,
                    size_t isamp, size_t osamp, size_t *iused, size_t *ogen);

/* Host-pointer forms with an explicit stream stride (batch handles). */
int RRX_push_strided(RR_handle *h, const fb_sample_t *ibuf, size_t in_stride, size_t isamp);
int RRX_pull_strided(RR_handle *h, fb_sample_t *obuf, size_t out_stride, size_t osamp, size_t *ogen);

/* Use the caller's hipStream_t (passed as void*) for all work of this handle from now on.  NULL is the device's default
 * stream, as in every HIP call (it is also what PyTorch's default stream is); RRX_STREAM_OWN restores the stream the
 * handle created for itself at RR_open, which is what a handle uses until this is called.  The caller keeps ownership of
 * its stream: RR_close never destroys it, but waits on it, so a caller-owned stream must outlive RR_close.  Work already
 * queued on the previous stream is ordered before the work queued after the switch.  RRX_sync blocks until everything
 * enqueued so far has finished. */
#define RRX_STREAM_OWN ((void *)(~(size_t)0))
int RRX_set_stream(RR_handle *h, void *hip_stream);
int RRX_sync(RR_handle *h);

/* Back to the just-opened state, so that one handle serves track after track (the reference has no such call: it closes and
 * opens, chain.h:26-29).  After RRX_reset the handle behaves as one just returned by the open call that made it -- same config,
 * channels, streams, device and sample format -- and for any sequence of data calls every sample it produces equals, bit for bit,
 * what a fresh handle produces for that sequence, in all four handle formats, through host and device calls.  The counters are
 * fresh as well: RRX_available is 0, RRX_isamp_max is unchanged, a later drain yields round(total_in * out_rate / in_rate), and
 * the wrap of the counters by whole seconds behaves as on a fresh handle; RRX_track_geometry and RRX_tracks_plan therefore
 * describe a reset handle unchanged.
 *   Discarded: frames pushed and not pulled (those still in the page-locked host mirror of an RR_push included), partial blocks,
 *   seam state, and the drained state.
 *   Kept: the stream set by RRX_set_stream, the profiling switch and its records, and every allocation -- rings keep the capacity
 *   they have grown to, which is what makes a reset cheaper than RR_close + RR_open.
 * The call only enqueues: no allocation, no host synchronisation.  All clearing is ordered on the handle's stream behind
 * everything queued so far, so output buffers of earlier *_device pulls are untouched and receive what was queued for them; the
 * stream-ordering contract is that of the *_device calls.
 * Returns RR_NULLHANDLE for NULL.  A poisoned handle (RRX_debug_fail_alloc) returns RR_INTERNAL and stays poisoned, like every
 * data call.  A reset of a fresh handle, or a second reset in a row, is RR_OK and changes nothing observable. */
int RRX_reset(RR_handle *h);

/* Per-kernel timing for benchmarks: while enabled, every stage launch is bracketed by HIP events on the
 * handle's stream.  RRX_profile_read synchronises, returns the summed duration and launch count of the
 * chain's dominant kernel ("hot": the fused dft->polyphase kernel, or the dft stage) and of all other
 * stage kernels, and clears the records. */
int RRX_profile(RR_handle *h, int enable);
int RRX_profile_read(RR_handle *h, double *hot_ms, long long *hot_launches, double *other_ms, long long *other_launches);
/* The same records per kernel instance, as JSON text: [{"kernel": "rsmp::fused_kernel<12, 11, 2, 7, true>", "hot": 1,
 * "launches": n, "ms": t}, ...] with the names rocprofv3 prints, so a benchmark line can say which variant the
 * engine's dispatch picked.  Synchronises and clears the records.  Returns the length written (text is truncated
 * to cap-1 bytes) or the negated RR_error. */
int RRX_profile_report(RR_handle *h, char *buf, size_t cap);

/* Test hook (fault injection), inert unless the process was started with RSMP_TEST_HOOKS set in its environment (read once,
 * at init_ratelib): the nth device allocation from now on, counted process-wide, fails as if the GPU were
 * out of memory (RR_ENOMEM + the init_ratelib handler, rate/xmalloc.c:38-43); 0 disarms.  A failure in the middle of a
 * push or drain poisons the handle: every later data call returns RR_INTERNAL until it is closed (its counters no
 * longer describe the device fifos; the reference has no recovery path either, chain.h:26-29 tears the chain down). */
void RRX_debug_fail_alloc(int nth);

/* Test hook (host only, needs no device), refused with -1 unless RSMP_TEST_HOOKS is set as above: the tile walk of the lean
 * fused kernels' polyphase stage for block `k` of a launch that starts at block B0, from the same closed forms the kernels
 * and their block table use.  Geometry: the polyphase stage (polyL phases of n taps, clock step `step`, initial clock at0,
 * preload b_offset of its input fifo), V valid samples per block, KS k-steps of 4 taps, window starts of the 4-residue
 * blocks within [qb_min, qb_max]; two_round = 1 with the two LDS images [0, ra_end) and [rb_start, V) (ra_end = 0: the lean
 * kernel's own 3072 / 2560); nsub > 0: sub-blocks of Vs samples.  slots receives 7 ints per (round, group, column step,
 * lane): those four, the output index relative to head[0], whether the store keeps it, and the window's first sample;
 * head[13] = i_lo, cnt, K, KA, per-group walk (1) or uniform (0), g_lo, g_hi, periods of the first round, tiles, tiles of
 * the uniform walk, irel_lo, base_li, groups.  Returns the number of slots of the block (at most cap are written). */
typedef struct RRX_walk_geom {
  long long at0, b_offset, B0;
  int V, polyL, step, n, KS, qb_min, qb_max, two_round, ra_end, rb_start, nsub, Vs;
} RRX_walk_geom;
long long RRX_debug_tile_walk(const RRX_walk_geom *geom, int k, long long *head, int *slots, size_t cap);

/* Test hook, as above (-1 unless RSMP_TEST_HOOKS is set, else 0): the start states of block `k`'s tile walk, the record that the
 * block table holds beside the entry and that the lean kernels begin from, evaluated on the host by the same function.
 * round[0] covers periods [0, ka), round[1] [ka, K): periods [kb, ke), the outputs the round may store (cnt), the boundaries
 * b1 <= b2 of its three runs of groups with each run's first period p0 and end pend = p0 + 4 x column steps, and for every
 * wave its number of tiles n, its first group g, and pc = p0 + 4 x (first column step) with that group's pend.  A round the
 * block does not have, and a wave without tiles, is all zero. */
typedef struct RRX_walk_start {
  struct {
    int kb, ke, cnt, b1, b2, p0[3], pend[3], pad;
    struct { int n, g, pc, pend; } wave[4];
  } round[2];
} RRX_walk_start;
int RRX_debug_walk_start(const RRX_walk_geom *geom, int k, RRX_walk_start *out);

/* Test hook, as above (-1 unless RSMP_TEST_HOOKS is set): the window start of the 4-residue block `bq` (0 .. 3) of 16-residue
 * group `group` within its period, both ways.  *arith is what the lean fused kernels compute where a group becomes current:
 * the numerator at0 + rb * step (rb = 16 group + 4 bq, 0 for an idle block rb >= polyL), multiplied high by rcp[0] and shifted
 * right by rcp[1]; *table is the entry of the host table that the other kernels read, the plain quotient by polyL.  rcp[2] is
 * the largest numerator a launch of this geometry can form; the multiplier and shift are chosen to be exact up to it.  Only
 * at0, polyL and step of the geometry are used.  Returns 0, or -2 where no such multiplier exists (the engine then refuses
 * the lean kernels with RR_INTERNAL) or group / bq lie outside the stage's groups. */
int RRX_debug_window_start(const RRX_walk_geom *geom, int group, int bq, int *arith, int *table, unsigned rcp[3]);

/* Sample formats.  A handle gets its format when it is opened and keeps it: every handle opened by the calls above is
 * RRX_FMT_FLOAT (interleaved float32, fb_sample_t).  An RRX_FMT_DOUBLE handle takes and gives interleaved float64 frames
 * at both ends; the chain in between is the same fp64 arithmetic, stage kernels and geometry as on a float handle of the
 * same config, so its output rounded to float32 equals the float handle's bit for bit, and nothing is rounded to 24 bits
 * on the way in or out.
 * A data call whose format does not match the handle's -- RR_push / RR_pull / RR_flow, RRX_*_device and RRX_*_strided on a
 * double handle, a *_double call on a float handle -- returns RR_INVPARAM and leaves the handle as it was (not poisoned,
 * counters unchanged).  Format-free calls (RR_drain, RR_close, RRX_sync, RRX_set_stream, profiling, introspection) work on
 * both kinds of handle. */
#define RRX_FMT_FLOAT  0   /* interleaved float32: what every other data call uses */
#define RRX_FMT_DOUBLE 1   /* interleaved float64 */
/* RRX_open_batch / RRX_open_batch_on with a sample format: device = -1 is RRX_open_batch's placement (the current device,
 * or round-robin under RATELIB_AMD_DEVICES), any other value is RRX_open_batch_on's.  An unknown format returns
 * RR_INVPARAM before any device is touched.  (RRX_FMT_S16 / RRX_FMT_S32: below.) */
int RRX_open_batch_fmt(const RR_config *config, int nchannels, int nstreams, int device, int format, RR_handle **const handle);
int RRX_format(const RR_handle *h); /* RRX_FMT_*, or -1 for NULL */

/* The double forms mirror RR_push / RR_pull / RR_flow (host memory, packed: the stride is ignored on one-stream handles
 * exactly as RRX_push_strided / RRX_pull_strided use it on batches) and RRX_push_device / RRX_pull_device /
 * RRX_flow_device (HBM pointers, the stream-ordering contract above) word for word: units are frames, isamp is clamped
 * to RRX_isamp_max, availability and drain totals are the float ones.  A float64 pointer need only be 8-byte aligned. */
int RRX_push_double(RR_handle *h, const double *ibuf, size_t in_stride, size_t isamp);                   /* RRX_push_strided */
int RRX_pull_double(RR_handle *h, double *obuf, size_t out_stride, size_t osamp, size_t *ogen);         /* RRX_pull_strided */
int RRX_flow_double(RR_handle *h, const double *ibuf, size_t in_stride, double *obuf, size_t out_stride, /* RR_flow, strided */
                    size_t isamp, size_t osamp, size_t *iused, size_t *ogen);
int RRX_push_device_double(RR_handle *h, const double *d_ibuf, size_t in_stride, size_t isamp);          /* RRX_push_device */
int RRX_pull_device_double(RR_handle *h, double *d_obuf, size_t out_stride, size_t osamp, size_t *ogen); /* RRX_pull_device */
int RRX_flow_device_double(RR_handle *h, const double *d_ibuf, size_t in_stride, double *d_obuf,        /* RRX_flow_device */
                           size_t out_stride, size_t isamp, size_t osamp, size_t *iused, size_t *ogen);

/* Integer PCM formats: audio at rest.  A handle opened with one of them takes and gives interleaved signed integer frames at
 * both ends; the conversions below are part of this ABI, the chain in between is the same fp64 arithmetic, stage kernels and
 * geometry as on a float handle of the same config (availability, the RRX_isamp_max clamp and drain totals are the float ones).
 *   in :  x = (double)s * 2^-15 (S16) or (double)s * 2^-31 (S32); both are exact in fp64.
 *   out:  q = rint(y * 2^bits), bits = 15 or 31, round half to even; saturated IN FP64 to [-2^bits, 2^bits - 1]; then narrowed
 *         to the integer type.  No wrap-around, no dither, no clipped-sample counter (RRX_finish_device, below, has both
 *         for the frames of a float or double handle).
 * So an integer handle's output equals, bit for bit, the output of an RRX_FMT_DOUBLE handle fed s * 2^-bits, quantised by the
 * rule above.  24-bit audio travels left-justified in RRX_FMT_S32 (sample << 8).
 * Any format value other than these four makes RRX_open_batch_fmt return RR_INVPARAM before any device is touched. */
#define RRX_FMT_S16 16   /* interleaved signed 16-bit PCM */
#define RRX_FMT_S32 32   /* interleaved signed 32-bit PCM (24-bit audio left-justified in it) */

/* One format-tagged set of data calls for all four formats.  `format` is the RRX_FMT_* the caller believes the buffers hold
 * and must equal the handle's: otherwise the call returns RR_INVPARAM and leaves the handle as it was (not poisoned, counters
 * unchanged).  Units (frames), strides (frames between streams; ignored by the host calls on one-stream handles), NULL and
 * zero-count handling, the RRX_isamp_max clamp and the stream-ordering contract of the device calls are those of the
 * *_double and *_strided / *_device calls above, word for word; on float and double handles these ARE those calls' code path.
 * The typed calls (RR_push / RR_pull / RR_flow, RRX_*_device, RRX_*_strided, RRX_*_double) return RR_INVPARAM on an S16 or
 * S32 handle.
 * Alignment: host and device pointers need only the alignment of one sample (2 bytes for S16, 4 for S32, 4 / 8 for float /
 * double).  A channel pair that is aligned as a pair (4 or 8 bytes for S16 / S32) takes the kernels' pair-word path, anything
 * else is read and written one sample at a time; the result is the same bits either way. */
int RRX_push_samples(RR_handle *h, int format, const void *ibuf, size_t in_stride, size_t isamp);
int RRX_pull_samples(RR_handle *h, int format, void *obuf, size_t out_stride, size_t osamp, size_t *ogen);
int RRX_flow_samples(RR_handle *h, int format, const void *ibuf, size_t in_stride, void *obuf, size_t out_stride,
                     size_t isamp, size_t osamp, size_t *iused, size_t *ogen);
int RRX_push_device_samples(RR_handle *h, int format, const void *d_ibuf, size_t in_stride, size_t isamp);
int RRX_pull_device_samples(RR_handle *h, int format, void *d_obuf, size_t out_stride, size_t osamp, size_t *ogen);
int RRX_flow_device_samples(RR_handle *h, int format, const void *d_ibuf, size_t in_stride, void *d_obuf, size_t out_stride,
                            size_t isamp, size_t osamp, size_t *iused, size_t *ogen);

/* Edge treatment for device-resident tracks.  The plugin never resamples a bare track: dsp_rate::on_chunk and flushwrite
 * (foo_dsp_rate.cpp:154-168, 241-312) extend the first and the last buffer by N_samples_to_add frames of linear-prediction
 * extrapolation (lpc/lpc.cpp), resample the extended signal and cut the resampled image of the extension (N_samples_to_drop
 * frames at each end) away again, which keeps the long filters from ringing against a hard track edge.  These two calls give a
 * caller whose frames are in HBM the same pieces; neither needs a handle.  (The drop-in plugin path keeps its own host lpc/:
 * its data is on the host anyway.)
 *
 * RRX_lpc_extrapolate_device is lpc_extrapolate2(data, data_len, nch, lpc_order, extra_bkwd, extra_fwd) of lpc/lpc.h:27 for every
 * stream of a [stream][frame][channel] float32 buffer in one call: d_data is frame 0 of stream 0's data_len base frames,
 * stream_stride the distance between streams in frames.  Per (stream, channel) it reads the base frames, writes extra_fwd frames
 * behind them and extra_bkwd frames in front of them (so d_data must have that many frames of room on either side) and touches
 * nothing else; the base frames are unchanged.  The result is bit-identical to the reference's: Welch window in float
 * (lpc.cpp:80-88), autocorrelation as serial ascending fp64 sums (:91-105), Levinson-Durbin in fp64 with the early stop and the
 * 0.999^k damping (:107-160), float recursion with the +-10 clamp, through which a NaN passes (:162-191).
 *   device: -1 is the calling thread's current device; any other value is checked as RRX_open_batch_on checks it (RR_INVPARAM for
 *   an index the process does not have, RR_EXTUNINIT for a device that is not gfx950).  The caller's device is restored on return.
 *   hip_stream: a hipStream_t as in RRX_set_stream (NULL = the device's default stream).  The call only enqueues: no allocation,
 *   no host synchronisation.  Ordering is the caller's, exactly as for the *_device calls above: whatever filled the base frames
 *   (or last wrote the frames around them) on ANOTHER stream must have completed, or be ordered before hip_stream by an event,
 *   when the call is made; work on hip_stream itself is ordered by the stream.
 * Returns RR_INVPARAM, before any device is touched, for NULL data, nstreams < 1, nch < 1, lpc_order outside 1..32,
 * data_len <= lpc_order, or nstreams > 1 with stream_stride < extra_bkwd + data_len + extra_fwd; RR_EXTUNINIT before
 * init_ratelib; RR_INTERNAL for a failed launch.  extra_bkwd == extra_fwd == 0 is RR_OK and does nothing.
 * Float32 frames only (the reference arithmetic is float32): double and integer buffers have no such call. */
int RRX_lpc_extrapolate_device(int device, void *hip_stream, fb_sample_t *d_data, size_t stream_stride, int nstreams,
                               size_t data_len, int nch, int lpc_order, size_t extra_bkwd, size_t extra_fwd);

/* Output stage for device-resident tracks: the counterpart of RRX_lpc_extrapolate_device at the other end.  One pass over the
 * float32 or float64 frames a handle produced ([stream][frame][channel], strides in frames between streams, ignored when
 * nstreams == 1) applies a per-stream gain, adds deterministic TPDF dither, quantises to integer PCM and takes the peak and the
 * number of clipped samples per (stream, channel).  It needs no handle, and no existing handle, format or kernel changes: an
 * integer handle keeps quantising by its own rule above, which is this one without gain and dither.
 *
 * The arithmetic is part of this ABI.  For sample x of stream s, channel ch, frame i of the call (all fp64, every operation
 * rounded on its own; 64-bit integers wrap):
 *   c = s * nch + ch;   g = (double)x * d_gain[s]   (d_gain NULL: g = x);   a = fabs(g);   t = g * 2^bits, bits = 15 / 23 / 31
 *   if dither:  z = seed + (first_frame + i) * 0x9E3779B97F4A7C15 + c * 0xBF58476D1CE4E5B9
 *               z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;   z = (z ^ (z >> 27)) * 0x94D049BB133111EB;   z = z ^ (z >> 31)
 *               t = t + ((double)(z >> 32) - (double)(z & 0xffffffff)) * 2^-32        triangular on (-1, 1) LSB
 *   q = rint(t), round half to even;   clip = !(-2^bits <= q <= 2^bits - 1), true for a NaN;   q saturates to that range in
 *   fp64 (a NaN to -2^bits) and is narrowed.
 * With dither = 0 and d_gain = NULL the S16 / S32 result is the integer handles' rule bit for bit.  The noise of a sample
 * depends on (seed, stream, channel, first_frame + i) alone: a track finished in chunks, with first_frame = the frames done so
 * far, gets the bits of one call.
 *   src_format: RRX_FMT_FLOAT or RRX_FMT_DOUBLE.
 *   dst_format: RRX_FMT_S16, RRX_FMT_S32, or RRX_FMT_S24_3: three bytes a sample, little endian, two's complement (WAV's packed
 *   24 bit).  RRX_FMT_S24_3 is a buffer format (here, in RRX_tracks_finish_device and as a source of
 *   RRX_tracks_stage_device_samples), never a handle format: RRX_open_batch_fmt refuses it.
 *   d_dst NULL: measure only -- nothing is written, dst_format and dst_stride are ignored, and the statistics are those of the
 *   RRX_FMT_S32 quantiser (bits = 31).
 *   d_peak (double) / d_clipped: [nstreams * nch] each, on the device, either may be NULL.  The call ACCUMULATES into what they
 *   hold -- peak = max(peak, every a), by an unsigned 64-bit maximum on the bit pattern (so a NaN sample leaves a NaN);
 *   clipped += the count of clip -- so the caller zeroes them, and chunked calls over one track sum up.  Both are independent of
 *   the order of the samples, hence deterministic.
 *   Pointers need only the alignment of one sample (1 byte for RRX_FMT_S24_3); no byte outside the frames * nch samples of each
 *   destination row is touched.
 *   device, hip_stream: as in RRX_lpc_extrapolate_device, with the same stream-ordering contract; the call only enqueues (no
 *   allocation, no host synchronisation) and restores the caller's device on return.
 * Returns RR_INVPARAM, before any device is touched, for a NULL source, nstreams < 1, nch < 1, an unknown source format, an
 * unknown destination format (d_dst not NULL), nstreams > 1 with a stride below frames, d_dst, d_peak and d_clipped all NULL,
 * first_frame + frames overflowing 64 bits, a size no buffer has -- frames * nch, or with nstreams > 1 nstreams * src_stride * nch
 * (nstreams * dst_stride * nch when d_dst is not NULL), of 2^60 samples or more, so that no offset the call computes can wrap --
 * or device < -1; RR_EXTUNINIT before init_ratelib; RR_INVPARAM for a device index the process does not have; RR_INTERNAL for
 * a failed launch.  frames == 0 is RR_OK and does nothing.  Noise shaping is RRX_finish_shaped_device's, below; integer or planar
 * sources and float destinations are not offered. */
#define RRX_FMT_S24_3 24   /* packed 3-byte signed 24-bit PCM: RRX_finish_device's destination only, and a source format of RRX_tracks_stage_device_samples and of the packed meter calls (RRX_tracks_true_peak_packed_device) */
int RRX_finish_device(int device, void *hip_stream, int src_format, const void *d_src, size_t src_stride,
                      int dst_format, void *d_dst, size_t dst_stride, int nstreams, size_t frames, int nch,
                      const double *d_gain, int dither, unsigned long long seed, unsigned long long first_frame,
                      double *d_peak, unsigned long long *d_clipped);
/* Test hook (host only, needs no device), refused with -1 unless RSMP_TEST_HOOKS is set as above: RRX_finish_device on HOST
 * pointers, as one serial loop over the very per-sample function the kernel calls.  Same refusals, same results. */
int RRX_debug_finish_host(int src_format, const void *src, size_t src_stride, int dst_format, void *dst, size_t dst_stride,
                          int nstreams, size_t frames, int nch, const double *gain, int dither, unsigned long long seed,
                          unsigned long long first_frame, double *peak, unsigned long long *clipped);

/* RRX_finish_device with noise-shaped dither: the requantisation error of a channel's previous 1..order frames is fed back through
 * an FIR filter, which moves the noise out of the band the filter was designed to spare.  The recursion contains a rint, so a
 * channel is a serial chain; to give the device independent chains the restart of the error history is PART OF THIS ABI: the
 * history of every channel is cleared at every absolute frame that is a multiple of `segment`.  The quantised sample is then a
 * function of (seed, stream, channel, absolute frame, and the samples of its own segment up to it).
 *
 * The arithmetic.  Everything is fp64 and every operation is rounded on its own (no fused multiply-add); 64-bit integers wrap.
 * For stream s, channel ch and frame i of the call:  F = first_frame + i,  c = s * nch + ch,  bits = 15 / 23 / 31.
 *   gain and scale   g = (double)x * d_gain[s]  (d_gain NULL: g = x);  a = fabs(g);  t = g * 2^bits   -- RRX_finish_device's
 *   history          e[1..order] are the errors of the channel's previous 1..order frames; all of them are +0.0 when
 *                    segment != 0 && F % segment == 0, or when F == 0
 *   feedback         acc = +0.0;  for k = order down to 1:  acc = acc + coefs[k-1] * e[k];   w = t - acc
 *                    (a descending sum: the newest error is added last)
 *   dither           u = dither ? w + d(seed, F, c) : w,   d = RRX_finish_device's dither of (seed, first_frame + i, c), unchanged
 *   quantise         q = rint(u), round half to even;  clip = !(-2^bits <= q <= 2^bits - 1);  the stored sample is
 *                    (int)fmin(fmax(q, -2^bits), 2^bits - 1): a NaN stores -2^bits and counts as clipped
 *   error            err = q - w, from the UNSATURATED q, so a clipped passage does not wind the filter up;
 *                    if (!(fabs(err) <= 2.0)) err = 0.0.  A finite sample gives |err| < 1.5; only +-inf or a NaN gives anything
 *                    else, and it then leaves no trace in the history
 *   shift            e[k+1] = e[k],  e[1] = err
 * Consequences:
 *   - with order = 1 and coefs[0] = 0.0 the bytes, peaks and clip counts are RRX_finish_device's, bit for bit, with and without
 *     dither, and for NaN, +-inf and -0.0 alike;
 *   - padding the coefficients with zeros at the high end changes no bit: acc starts at +0.0 and +0.0 + (+-0.0) = +0.0.  The kernel
 *     rounds order up to a compile-time size on that ground and keeps the history in registers.
 *   coefs: a HOST pointer to `order` doubles, copied into the launch arguments; order is 1..RRX_SHAPE_MAX_ORDER and every
 *   coefficient finite.  The call designs no filter: published 44.1 kHz designs are in the Python binding (NOISE_SHAPES).
 *   segment: in frames; any value >= 1, or 0 for "never restart" (one lane per channel: the textbook serial form).
 *   d_dst NULL: measure only -- nothing is written, dst_stride is ignored, but dst_format must still be valid and its bits are
 *   used: the shaped noise is tens of LSB of the target format, and a caller who measures first and then writes must see the clip
 *   count the write will produce.
 *   State: [nstreams * nch][RRX_SHAPE_MAX_ORDER] doubles on the device; entry k-1 of a channel is e[k], entries at `order` and
 *   beyond are 0.  d_state_in NULL: the call must begin a segment (first_frame % segment == 0, or first_frame == 0 for
 *   segment 0), else RR_INVPARAM.  d_state_in not NULL is read only when the call begins inside a segment.  d_state_out not NULL
 *   receives, for every channel, the history as it stands after the call's last frame.  The two must not overlap (RR_INVPARAM,
 *   equal pointers included): the lane that reads the state and the lane that writes it are unordered within one launch, so a
 *   caller ping-pongs two buffers.  Contiguous ascending calls that hand the state on leave the bytes and statistics of one call,
 *   for any cut positions.
 *   Everything else -- src_format, dst_format, layouts and strides, the alignment of one sample and "no byte outside the
 *   frames * nch samples of each destination row is touched", d_peak / d_clipped and their accumulation, device and hip_stream
 *   with the stream-ordering contract, "only enqueues: no allocation, no host synchronisation" -- is RRX_finish_device's.
 * Returns RR_INVPARAM, before any device is touched, for every argument RRX_finish_device refuses, and further for an unknown
 * dst_format (d_dst NULL included), coefs NULL, order outside 1..RRX_SHAPE_MAX_ORDER, a non-finite coefficient, and the state
 * rules above; RR_EXTUNINIT before init_ratelib; RR_INTERNAL for a failed launch.  frames == 0 is RR_OK and touches nothing, the
 * state included. */
#define RRX_SHAPE_MAX_ORDER 16
int RRX_finish_shaped_device(int device, void *hip_stream, int src_format, const void *d_src, size_t src_stride,
                             int dst_format, void *d_dst, size_t dst_stride, int nstreams, size_t frames, int nch,
                             const double *d_gain, int dither, unsigned long long seed, unsigned long long first_frame,
                             const double *coefs, int order, size_t segment,
                             const double *d_state_in, double *d_state_out,
                             double *d_peak, unsigned long long *d_clipped);
/* Test hook (host only, needs no device), refused with -1 unless RSMP_TEST_HOOKS is set as above: RRX_finish_shaped_device on
 * HOST pointers, as one serial loop per channel over the very per-sample functions the kernel calls.  Same refusals, same results. */
int RRX_debug_finish_shaped_host(int src_format, const void *src, size_t src_stride, int dst_format, void *dst, size_t dst_stride,
                                 int nstreams, size_t frames, int nch, const double *gain, int dither, unsigned long long seed,
                                 unsigned long long first_frame, const double *coefs, int order, size_t segment,
                                 const double *state_in, double *state_out, double *peak, unsigned long long *clipped);

/* True peak: the peak of the gained frames oversampled by a polyphase filter (ITU-R BS.1770-4 Annex 2 with a 4 x 12 filter, in
 * dBTP once the caller takes 20 log10), beside the sample peak, per (stream, channel), in one pass over device-resident frames.  A
 * track normalised to a SAMPLE peak of 0 dBFS can overshoot between the samples by several dB; the gain that normalises a track
 * comes from max(true peak, sample peak) -- both, because a filter whose centre tap is below 1 can put the true peak under the
 * sample peak.  The call needs no handle and writes no sample.
 *
 * The arithmetic is part of this ABI.  Everything is fp64 and every operation is rounded on its own (no fused multiply-add).  The
 * filter has `phases` (1..RRX_TP_MAX_PHASES) x `taps` (1..RRX_TP_MAX_TAPS) coefficients, phase-major.  For stream s, channel ch
 * and frame i of the call:  F = first_frame + i,  c = s * nch + ch.
 *   gain        g[F] = (double)x * d_gain[s]  (d_gain NULL: g = x);  a = fabs(g[F])                     -- RRX_finish_device's
 *   history     g[F-k], k = 1..taps-1, are the channel's previous gained samples; frames before absolute frame 0 are +0.0, frames
 *               before the call's first frame come from d_state_in
 *   phases      for p in 0..phases-1:  acc = +0.0;  for k = taps-1 down to 0:  acc = acc + coefs[p*taps + k] * g[F-k];   y_p = acc
 *               (a descending sum: the newest sample is added last)
 *   true peak   tp[F] = max over p of fabs(y_p), as an unsigned 64-bit maximum on the bit patterns (a NaN lies above +inf and stays)
 * Results: d_true_peak[c] = max(what it holds, every tp[F]) and d_peak[c] = max(what it holds, every a), both by the unsigned
 * 64-bit atomic maximum of RRX_finish_device, [nstreams * nch] doubles each on the device.  Either may be NULL, not both.  Both
 * ACCUMULATE: the caller zeroes them, and chunked calls add up.  On the same frames and gain d_peak is RRX_finish_device's
 * measure-only peak, bit for bit.
 *   coefs: a HOST pointer to phases * taps finite doubles, copied into the launch arguments as they are.  The call designs no
 *   filter; the BS.1770 table is in the Python binding (TRUE_PEAK_FILTERS).  The coefficients are never padded with zeros to a
 *   fixed size: 0 * inf is a NaN, so a padded sum would differ for non-finite samples.
 *   flush != 0: taps - 1 further frames of g = +0.0 are evaluated behind the call's last frame -- the filter's tail, where the
 *   intersample peak of a track's last samples lies.  They enter d_true_peak only, neither d_peak nor the state.
 *   State: [nstreams * nch][RRX_TP_MAX_TAPS] doubles on the device; entry j of a channel is the gained sample j + 1 frames before
 *   the next frame to come, entries at taps - 1 and beyond are 0.  d_state_in NULL needs first_frame == 0, else RR_INVPARAM;
 *   d_state_in not NULL is read only when first_frame > 0.  d_state_out not NULL receives, for every channel, the history after
 *   the call's last real frame; with frames < taps - 1 it mixes new and old entries.  The two must not overlap (RR_INVPARAM, equal
 *   pointers included), for the reason RRX_finish_shaped_device gives.  Contiguous ascending calls that hand the state on, with
 *   flush on the last one only, leave the bits of one call with flush, for any cut positions.
 *   Everything else -- src_format (RRX_FMT_FLOAT or RRX_FMT_DOUBLE), layouts and strides, the alignment of one sample, device and
 *   hip_stream with the stream-ordering contract, "only enqueues: no allocation, no host synchronisation" -- is
 *   RRX_finish_device's.
 * Returns RR_INVPARAM, before any device is touched, for every size, stride and overflow RRX_finish_device refuses, and further
 * for coefs NULL, phases or taps out of range, a non-finite coefficient, d_true_peak and d_peak both NULL, and the state rules
 * above; RR_EXTUNINIT before init_ratelib; RR_INTERNAL for a failed launch.  frames == 0 is RR_OK and touches nothing, even with
 * flush. */
#define RRX_TP_MAX_PHASES 8
#define RRX_TP_MAX_TAPS 16
int RRX_true_peak_device(int device, void *hip_stream, int src_format, const void *d_src, size_t src_stride, int nstreams,
                         size_t frames, int nch, const double *d_gain, unsigned long long first_frame,
                         const double *coefs, int phases, int taps, int flush,
                         const double *d_state_in, double *d_state_out, double *d_true_peak, double *d_peak);
/* Test hook (host only, needs no device), refused with -1 unless RSMP_TEST_HOOKS is set as above: RRX_true_peak_device on HOST
 * pointers, as one serial loop per channel over the very per-frame function the kernels call.  Same refusals, same results. */
int RRX_debug_true_peak_host(int src_format, const void *src, size_t src_stride, int nstreams, size_t frames, int nch,
                             const double *gain, unsigned long long first_frame, const double *coefs, int phases, int taps, int flush,
                             const double *state_in, double *state_out, double *true_peak, double *peak);

/* Host-only (no GPU needed): the plugin's edge geometry for a rate pair (dsp_rate::reinit, foo_dsp_rate.cpp:96-101).
 * *n_add / *n_drop = samples_len(in_rate, out_rate, 20, 8192) of util.h:38-48: frames to extrapolate at each end of the input
 * and frames to cut from each end of the output, the same duration at the two rates (n_add * out_rate == n_drop * in_rate);
 * *prime_len = max(clamp(in_rate / 20, 1024, 16384), 65): the base frames the extrapolator looks at (PRIME_LEN_);
 * *inbuf = clamp(in_rate / 10, 2048, 65536): the plugin's staging buffer (INBUF_SIZE_).  RR_INVPARAM for a zero rate or a NULL
 * output. */
int RRX_edge_geometry(size_t in_rate, size_t out_rate, size_t *n_add, size_t *n_drop, size_t *prime_len, size_t *inbuf);

/* Ragged track batches: whole tracks of UNEQUAL length through one batch handle.  A batch handle's streams run in lock step, so
 * the rows it is pushed from all have one length; a shorter track is followed by zeros up to the longest row.  Those zeros are
 * what RR_drain would have fed a handle of its own, and the engine's output does not depend on how its input is cut into pushes,
 * so over its own output range the track gets the bits of a one-stream handle that was drained after it.  What differs per
 * track is where it lies: in the packed source, in its row (behind its own LPC extension), in its output row (behind the
 * resampled image of that extension) and in the packed destination.  RRX_track says so, RRX_tracks_plan fills a table of them on
 * the host, and the two device calls read that table from device memory.  All fields are in FRAMES. */
typedef struct RRX_track {
  unsigned long long src_first;  /* first frame of the track in the packed source            */
  unsigned long long frames;     /* its length                                               */
  unsigned long long lead;       /* where its frame 0 sits in its row: n_add, or 0           */
  unsigned long long out_first;  /* first frame of its output in its output row: n_drop or 0 */
  unsigned long long out_frames; /* frames of output it owns                                 */
  unsigned long long dst_first;  /* first frame of its output in the packed destination      */
} RRX_track;

/* Host-only (no GPU needed): what the whole-track path does with ONE track of `frames` frames on a handle of its own
 * (dsp_rate::on_chunk / flushwrite, foo_dsp_rate.cpp:154-168, 218-313).  More than 2 * LPC_ORDER = 64 frames: *lead = n_add frames
 * of extrapolation in front of it and as many behind it, *ext_frames = frames + 2 * n_add, *out_first = n_drop (RRX_edge_geometry).
 * Up to 64 frames (zero included): *lead = 0, *ext_frames = frames, *out_first = 0.  *out_frames = max(T - 2 * *out_first, 0), where
 * T is what a handle yields in all for *ext_frames frames pushed in RRX_isamp_max pieces and drained -- computed from the handle's
 * own counter arithmetic, the wrap of rate_input's counters by whole seconds included (rate_base.h:436-441, 454-468), not from a
 * closed form.  A zero-length track owns no output.
 * Returns RR_INVPARAM for a NULL argument, a config the planner refuses, or frames above 2^36 (the call walks the track's pushes). */
int RRX_track_geometry(const RR_config *config, size_t frames, size_t *lead, size_t *ext_frames, size_t *out_first,
                       size_t *out_frames);
/* Host-only: the table for `ntracks` tracks of frames[t] frames, packed in that order.  table[t] is RRX_track_geometry's answer for
 * frames[t]; src_first and dst_first are the running sums of frames and out_frames.  *row_frames = the largest ext_frames: the
 * length of the rows the handle is pushed from.  *out_row_cap = *row_frames * out_rate / in_rate + 2: output frames a row can
 * give, the pitch to allocate for the output rows.  *src_total / *dst_total = frames of the packed source / destination.
 * Returns RR_INVPARAM for a NULL argument, ntracks < 1, a config the planner refuses, a track above 2^36 frames, or sums that
 * overflow. */
int RRX_tracks_plan(const RR_config *config, const size_t *frames, int ntracks, RRX_track *table, size_t *row_frames,
                    size_t *out_row_cap, size_t *src_total, size_t *dst_total);

/* Host-only (no GPU needed): a library of `ntracks` tracks as the batches of a handle of `nstreams` streams.  A batch handle
 * resamples nstreams rows of its longest track's length whatever the other tracks hold, so tracks of like length belong together.
 *   order[ntracks]: the track indices sorted by frames descending, ties by index ascending (ext_frames is monotonic in frames,
 *   so this is also descending in row length).
 *   Batch b is order[b * nstreams, min((b + 1) * nstreams, ntracks)); *nbatches = ceil(ntracks / nstreams).
 *   row_frames[b] (NULL, or room for *nbatches entries): what RRX_tracks_plan returns for batch b.
 *   *resampled = sum over b of nstreams * row_frames[b], the frames the handle resamples (it has nstreams streams whatever the
 *   last batch holds); *useful = sum over t of ext_frames[t].  Either may be NULL.  1 - useful / resampled is the padding share.
 * This split minimises sum_b row_frames[b], and with it *resampled, over every partition of the tracks into batches of at most
 * nstreams tracks: some batch must hold the longest track and costs its row; filling that batch with the next longest tracks
 * leaves a remainder whose k-th longest track is no longer than under any other choice, and no partition has fewer batches.
 * Returns RR_INVPARAM for NULL config, frames, order or nbatches, ntracks < 1, nstreams < 1, and whatever RRX_tracks_plan
 * refuses (a config the planner refuses, a track above 2^36 frames, sums that overflow). */
int RRX_tracks_batches(const RR_config *config, const size_t *frames, int ntracks, int nstreams, int *order, size_t *row_frames,
                       int *nbatches, unsigned long long *resampled, unsigned long long *useful);

/* One pass from the packed tracks (d_packed: [src_total][nch] float32) to the rows a batch handle is pushed from (d_rows:
 * [ntracks][row_frames][nch]).  Row t receives, with ext = lead + frames + lead:
 *   [lead, lead + frames)        the track, copied;
 *   [0, lead)                    RRX_lpc_extrapolate_device's backward extension from its first min(frames, prime_len) frames;
 *   [lead + frames, ext)         its forward extension from the track's last min(frames, prime_len) frames -- both with
 *                                lpc_order 32 and bit for bit what that call writes (the kernels share one body);
 *   [ext, row_frames)            zeros.
 * Every frame of every row is written exactly once, nothing outside the rows is written, and d_packed is only read.  in_rate and
 * out_rate fix prime_len (RRX_edge_geometry).
 * d_tracks is DEVICE memory (a copy of RRX_tracks_plan's table) and a call that never synchronises cannot validate it.  So the
 * kernels clamp instead: what a track reads is clamped to [0, src_total) (frames past it read as zeros) and what it writes to its
 * own row (lead, frames and the extension are cut to row_frames).  A wrong table gives wrong samples, never an access outside
 * the buffers.
 * device, hip_stream, stream ordering: RRX_lpc_extrapolate_device's, word for word.  The call only enqueues (no allocation, no
 * host synchronisation) and restores the caller's device on return.
 * Returns RR_INVPARAM, before any device is touched, for a NULL pointer, ntracks < 1, nch < 1, a zero rate, row_frames == 0,
 * ntracks * nch of 2^30 or more, a size no buffer has (src_total * nch or ntracks * row_frames * nch of 2^60 samples or more) or
 * device < -1; RR_EXTUNINIT before init_ratelib or for a device that is not gfx950; RR_INVPARAM for a device index the process does
 * not have; RR_INTERNAL for a failed launch.  Float32 sources only: this is the RRX_FMT_FLOAT case of
 * RRX_tracks_stage_device_samples, below, and the same code path. */
int RRX_tracks_stage_device(int device, void *hip_stream, size_t in_rate, size_t out_rate, const RRX_track *d_tracks, int ntracks,
                            int nch, const fb_sample_t *d_packed, size_t src_total, fb_sample_t *d_rows, size_t row_frames);

/* RRX_tracks_stage_device from a packed source of integer PCM, audio as it is stored: the stage pass converts on load, so no
 * float32 copy of the source is ever written.  src_format is RRX_FMT_FLOAT (d_packed: [src_total][nch] float32, RRX_tracks_stage_device
 * itself), RRX_FMT_S16, RRX_FMT_S32, or RRX_FMT_S24_3 (three bytes a sample, little endian, two's complement, sign-extended:
 * [src_total][nch * 3] bytes).  The rows are float32 whatever the source is -- the LPC arithmetic is float32, and so are the handles
 * they are pushed to -- which is why RRX_FMT_DOUBLE is no source format of this call.
 * The conversion is part of this ABI.  For a source sample s, with bits = 15 (S16), 23 (S24_3) or 31 (S32):
 *   x = (float)((double)s * 2^-bits)        one rounding, to nearest even
 * which is exact for S16 and S24_3; S32 is rounded to float32's 24 bits, and INT32_MAX becomes 1.0f.  ((float)s rounded to nearest
 * even and then scaled by the power of two gives the same bits.)  Copied frames and the base frames of both LPC extensions are
 * converted by this one rule, so the rows equal, bit for bit, those of RRX_tracks_stage_device on the converted source.
 * Reads: d_packed needs the alignment of one sample (2 bytes for S16, 1 byte for S24_3, 4 for S32 and float32).  Tracks are adjacent,
 * so a track begins at any sample, for S24_3 at any byte offset.  No byte outside [d_packed, d_packed + src_total * nch * bytes) is
 * relied on; the copy kernel loads whole aligned dwords, so it may READ the aligned dword that holds the first byte of the source and
 * the one that holds its last byte in full (up to 3 bytes on either side, in the same page: this cannot fault), and nothing further
 * out.  The table clamps are RRX_tracks_stage_device's: frames past src_total read as zeros.
 * Everything else -- what row t receives, "every frame of every row is written exactly once, nothing outside the rows is written,
 * d_packed is only read", the unvalidated device table, device, hip_stream, stream ordering, "only enqueues", every refusal and
 * return value -- is RRX_tracks_stage_device's, word for word; an src_format other than those four (RRX_FMT_DOUBLE included)
 * returns RR_INVPARAM before any device is touched. */
int RRX_tracks_stage_device_samples(int device, void *hip_stream, size_t in_rate, size_t out_rate, const RRX_track *d_tracks,
                                    int ntracks, int nch, int src_format, const void *d_packed, size_t src_total,
                                    fb_sample_t *d_rows, size_t row_frames);
/* Test hook (host only, needs no device), refused with -1 unless RSMP_TEST_HOOKS is set as above: the conversion above for samples
 * [first_sample, first_sample + count) of a HOST buffer of src_format, as one serial loop over the very per-sample function the
 * kernels call.  RR_INVPARAM for an unknown format or a NULL pointer. */
int RRX_debug_tracks_load_host(int src_format, const void *src, size_t first_sample, size_t count, float *out);

/* RRX_finish_device per track in one call.  Track t takes frames [out_first, out_first + out_frames) of row t of d_rows
 * ([ntracks][row_frames][nch], float32 or float64: row_frames is here the pitch of the OUTPUT rows, RRX_tracks_plan's
 * out_row_cap) to frames [dst_first, dst_first + out_frames) of the packed destination d_dst ([dst_total][nch] of RRX_FMT_S16,
 * RRX_FMT_S24_3 or RRX_FMT_S32).  The arithmetic is RRX_finish_device's with stream s = t, first_frame = 0 and frame i counted
 * from the track's own first output frame; d_gain [ntracks], d_peak and d_clipped [ntracks * nch] are per track as they are per
 * stream there, and accumulate as there.  So track t's bytes and statistics are those of a one-stream RRX_finish_device call on
 * its slice with seed + t * nch * 0xBF58476D1CE4E5B9 (mod 2^64) for seed.  The statistics cover the track's own frames and
 * nothing else of its row.  d_dst NULL measures only (dst_format and dst_total are ignored).  Tracks are adjacent in the
 * destination, at any byte offset; no byte of a neighbouring track and no byte beyond dst_total frames is touched.
 * d_tracks is device memory and is clamped as in RRX_tracks_stage_device: a track's slice is cut to its row and (when written)
 * to the destination, so a wrong table gives wrong samples, never an access outside the buffers.
 * device, hip_stream, refusals: RRX_finish_device's -- RR_INVPARAM, before any device is touched, for a NULL table or source,
 * ntracks < 1, nch < 1, an unknown source format, an unknown destination format (d_dst not NULL), d_dst, d_peak and d_clipped
 * all NULL, ntracks * row_frames * nch or (d_dst not NULL) dst_total * nch of 2^60 samples or more, or device < -1.
 * row_frames == 0 is RR_OK and does nothing. */
int RRX_tracks_finish_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch, int src_format,
                             const void *d_rows, size_t row_frames, int dst_format, void *d_dst, size_t dst_total,
                             const double *d_gain, int dither, unsigned long long seed, double *d_peak,
                             unsigned long long *d_clipped);

/* RRX_finish_shaped_device per track in one call: RRX_tracks_finish_device with noise-shaped dither.  Tables, rows, the packed
 * destination, gains, statistics, clamps (a wrong table gives wrong samples, never an access outside the buffers), device,
 * hip_stream and refusals are RRX_tracks_finish_device's; coefs, order and segment are RRX_finish_shaped_device's, refused as
 * there, and as there dst_format must be valid when d_dst is NULL too (its bits are used).  Frame i and the segments are counted
 * from the track's own first output frame, and there is no state: whole rows only (RRX_tracks_finish_shaped_window_device, below,
 * is the form by windows, with a state per track).  Track t gets the bytes and statistics of a
 * one-stream RRX_finish_shaped_device call on its slice with seed + t * nch * 0xBF58476D1CE4E5B9 (mod 2^64) for seed,
 * first_frame = 0 and no state.  row_frames == 0 is RR_OK and does nothing. */
int RRX_tracks_finish_shaped_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch,
                                    int src_format, const void *d_rows, size_t row_frames, int dst_format, void *d_dst,
                                    size_t dst_total, const double *d_gain, int dither, unsigned long long seed,
                                    const double *coefs, int order, size_t segment,
                                    double *d_peak, unsigned long long *d_clipped);

/* RRX_true_peak_device per track in one call: how a caller finds the gain that normalises each track of a ragged batch to a true
 * peak.  Tables, rows and their clamping are RRX_tracks_finish_device's in its measure-only form: track t's slice is frames
 * [out_first, out_first + out_frames) of row t of d_rows ([ntracks][row_frames][nch], float32 or float64), clamped to the row.
 * Track t gets the results of a one-stream RRX_true_peak_device call on that slice with first_frame = 0, no state, flush = 1 and
 * d_gain[t] (d_gain NULL: unity), into d_true_peak / d_peak [ntracks * nch], accumulated as there.  The frames of the row in front
 * of the slice -- the resampled image of the LPC extension -- are NOT history: the written file does not hold them, so the filter
 * starts from +0.0 at the track's first output frame.  A wrong table gives wrong numbers, never an access outside the rows.
 * Refusals: RR_INVPARAM, before any device is touched, for a NULL table or source, ntracks < 1, nch < 1, an unknown source format,
 * both result pointers NULL, the filter refusals of RRX_true_peak_device, ntracks * row_frames * nch of 2^60 samples or more, or
 * device < -1; the rest as there.  row_frames == 0 is RR_OK and does nothing.  The form by windows, with the history
 * carried per track, is RRX_tracks_true_peak_window_device. */
int RRX_tracks_true_peak_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch,
                                int src_format, const void *d_rows, size_t row_frames, const double *d_gain,
                                const double *coefs, int phases, int taps, double *d_true_peak, double *d_peak);

/* RRX_true_peak_device per track of a library AT REST: the tracks lie end to end in d_packed as [src_total][nch] samples of
 * src_format, the packed source of RRX_tracks_stage_device_samples -- RRX_FMT_FLOAT, RRX_FMT_S16, RRX_FMT_S24_3 (three bytes,
 * little endian, two's complement) or RRX_FMT_S32; a sample is aligned to its own size, for S24_3 one byte.  No float copy, no
 * rows padded to the longest track, no handle and no rate pair: what a ReplayGain 2.0 / EBU R 128 scan needs.
 * Track t uses only the input side of its RRX_track entry, clamped:
 *   first  = min(src_first, src_total)
 *   frames = min(frames, src_total - first, max_frames)
 * so a wrong table gives wrong numbers, never a read outside d_packed.  max_frames plays the part row_frames plays in the row
 * forms: it bounds the grid, and a track longer than max_frames is measured up to max_frames.  (A table of RRX_tracks_plan works,
 * and so does one with src_first as prefix sums, frames as lengths and zeros elsewhere.)
 * The sample value is part of this ABI: v = (double)s * 2^-15 (S16), 2^-23 (S24_3) or 2^-31 (S32), and (double)x for float32,
 * exact for all four.  For S32 this is deliberately NOT the value of the stage pass, which rounds to float32: a meter measures
 * what the file holds, so INT32_MAX has the peak 1 - 2^-31 and not 1.0, and INT32_MIN and -32768 have 1.0.  The gained sample is
 * d_gain ? v * d_gain[t] : v.  From there on nothing is new: track t gets, bit for bit, the results of a one-stream
 * RRX_true_peak_device call on a float64 buffer holding its v, with first_frame = 0, no state and flush = 1, into d_true_peak /
 * d_peak [ntracks * nch], accumulated as in RRX_tracks_true_peak_device.
 * Reads: exactly the bytes of the samples of the clamped tracks.  device, hip_stream, "only enqueues": as there.
 * Refusals: RR_INVPARAM, before any device is touched, for a NULL table or source, ntracks < 1, nch < 1, a format outside the four
 * above (RRX_FMT_DOUBLE included), the filter refusals of RRX_true_peak_device, both result pointers NULL, src_total * nch or
 * ntracks * max_frames * nch of 2^60 or more, or device < -1; the rest as there.  max_frames == 0 or src_total == 0 is RR_OK and
 * does nothing. */
int RRX_tracks_true_peak_packed_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch,
                                       int src_format, const void *d_packed, size_t src_total, size_t max_frames,
                                       const double *d_gain, const double *coefs, int phases, int taps, double *d_true_peak,
                                       double *d_peak);
/* Test hook (host only, needs no device), refused with -1 unless RSMP_TEST_HOOKS is set as above: the call above on HOST
 * pointers, as a serial loop over the same clamp, the same one-sample load and the same per-frame function as the kernels. */
int RRX_debug_tracks_true_peak_packed_host(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *packed,
                                           size_t src_total, size_t max_frames, const double *gain, const double *coefs,
                                           int phases, int taps, double *true_peak, double *peak);

/* True-peak limiter: one gain per frame, linked across a stream's channels, that holds the gained frames under a ceiling where a
 * static gain would pull the whole track down for a few transients.  The detector is RRX_true_peak_device's; the gain is a window
 * minimum of the demanded reductions smoothed by a box of `lookahead` frames.  Nothing in it is recursive (there is no one-pole
 * release), so every frame is independent work.  The call needs no handle.
 *
 * The arithmetic is part of this ABI.  Everything is fp64 and every operation is rounded on its own (no fused multiply-add).  Per
 * stream s, with N = frames, the filter of phases x taps as in RRX_true_peak_device, D = taps - 1, c = ceiling, L = lookahead and
 * H = hold:
 *   g[n][ch]  = (double)x * d_gain[s]  (d_gain NULL: g = x)                                            -- RRX_finish_device's
 *   tp[F][ch] for F in [0, N + D): RRX_true_peak_device's tp[F] on the history g[F-k], k < taps, with +0.0 before frame 0 and
 *             behind frame N-1 (first_frame = 0, no state, flush = 1)
 *   a[F][ch]  = fabs(g[F][ch]) for F < N, +0.0 for F >= N
 *   lev[F]    = max over ch of max(tp[F][ch], a[F][ch]), as an unsigned 64-bit maximum on the bit patterns (a NaN lies above +inf)
 *   r[F]      = lev[F] > c ? c / lev[F] : 1.0   (the division correctly rounded; a NaN level fails the comparison: 1.0; +inf gives
 *             +0.0);  r[F] = 1.0 for F < 0 and F >= N + D
 *   m[k]      = min of r[F] over F in [k - H, k + L - 1 + D],  for k in [-(L-1), N)        (a minimum: the order does not matter)
 *   acc       = +0.0;  for i = L-1 down to 0:  acc = acc + m[n - i]
 *   s[n]      = fmin(acc * invL, m[n]),   invL = 1.0 / (double)L computed once on the host
 *   y[n][ch]  = g[n][ch] * s[n], stored as a double (RRX_FMT_DOUBLE) or rounded once to float32 (RRX_FMT_FLOAT)
 * What holds, and what does not.  Every m[n-i], 0 <= i < L, covers [n, n + D], so s[n] <= r[F] for every detector frame F whose
 * filter window contains sample n, and a[n] enters lev[n]: for finite input |y| <= c * (1 + 2^-51) in fp64, the slack being the
 * rounding of c / lev times lev.  The fmin keeps the serial sum's rounding from lifting s[n] above m[n].  The gain starts to fall
 * L + D frames before a peak, is fully down D frames before it, stays down H frames behind it and returns over L frames.  The
 * TRUE peak of y is NOT strictly bounded by c: a gain that varies inside the filter's window is not a scalar factor of the
 * filter's sum.  The overshoot that remains shrinks with L (a few percent at L = 1, below one percent at L = 72, DESIGN.md 10,
 * "Limiter"); a caller who needs the bound measures y with RRX_true_peak_device and trims with a static gain, as
 * convert_tracks_to_pcm_loudness_limited of the Python binding does.
 * Results per stream, both ACCUMULATED: d_reduction[s] (double, [nstreams] on the device; the caller presets it to 1.0) takes
 * min(what it holds, every s[n]) by an unsigned 64-bit atomic minimum on the bit pattern (s >= +0.0 and never a NaN);
 * d_limited[s] (unsigned 64-bit, [nstreams]; the caller zeroes it) counts the frames with s[n] < 1.0.  Either may be NULL.
 *   A NaN sample passes through as a NaN and demands no reduction where it poisons the level; +-inf demands r = +0.0 around it
 *   (and inf * 0 leaves a NaN in its own place).  Neither faults, and the other streams are exact.
 *   src_format and dst_format are RRX_FMT_FLOAT or RRX_FMT_DOUBLE, each on its own; integer sources are not offered.  d_dst has
 *   the source's geometry with dst_stride.  d_dst may be exactly d_src (in place), with equal formats and equal strides only; any
 *   other overlap of the two extents is RR_INVPARAM.
 *   d_work: at least RRX_limit_work_doubles(nstreams, frames, taps, lookahead) doubles on the device, which is
 *   nstreams * 2 * (frames + taps + lookahead) -- r and m, generously -- or 0 for arguments the call would refuse and for a
 *   product of 2^60 or more (host only).  Its content after the call is unspecified.
 *   Launches: the detector (one lane per frame F, the gained samples staged in LDS), the window minimum (LDS tiles of r),
 *   smoothing and product (an LDS tile of m, four frames to a lane), each split over chunks of 32768 streams.  The call only enqueues: no
 *   allocation, no host synchronisation.  coefs (a HOST pointer), layouts, the alignment of one sample, device and hip_stream with
 *   the stream-ordering contract are RRX_true_peak_device's.
 * Returns RR_INVPARAM, before any device is touched, for everything RRX_true_peak_device refuses of the shared arguments (source,
 * strides, sizes, filter, device < -1), and further for d_dst NULL, an unknown dst_format, a dst_stride below frames or beyond
 * 2^60 samples, a ceiling that is not finite or not > 0, lookahead outside 1..RRX_LIMIT_MAX_LOOKAHEAD, hold above
 * RRX_LIMIT_MAX_HOLD, d_work NULL or work_doubles too small, and the overlap rule; RR_EXTUNINIT before init_ratelib; RR_INTERNAL for
 * a failed launch.  frames == 0 is RR_OK and touches nothing. */
#define RRX_LIMIT_MAX_LOOKAHEAD 1024
#define RRX_LIMIT_MAX_HOLD      4096
size_t RRX_limit_work_doubles(int nstreams, size_t frames, int taps, size_t lookahead);
int RRX_limit_device(int device, void *hip_stream, int src_format, const void *d_src, size_t src_stride,
                     int dst_format, void *d_dst, size_t dst_stride, int nstreams, size_t frames, int nch,
                     const double *d_gain, double ceiling, const double *coefs, int phases, int taps,
                     size_t lookahead, size_t hold, double *d_reduction, unsigned long long *d_limited,
                     double *d_work, size_t work_doubles);
/* RRX_limit_device per track of a ragged batch in one call.  Tables, rows and their clamping are RRX_tracks_true_peak_device's:
 * track t is frames [out_first, out_first + out_frames) of row t of d_rows ([ntracks][row_frames][nch]), clamped to the row, and is
 * limited as a one-stream RRX_limit_device call on that slice under d_gain[t] -- the history in front of the slice is +0.0, not the
 * row.  The result goes to the same frames of row t of d_dst_rows, which has the same geometry and may be d_rows (then with
 * dst_format == src_format; any other overlap is RR_INVPARAM).  Frames of the rows outside the slices are not written.
 * d_reduction and d_limited are [ntracks].  d_work: RRX_limit_work_doubles(ntracks, row_frames, taps, lookahead) doubles.  A wrong
 * table gives wrong samples, never an access outside the rows or d_work.  Refusals: RR_INVPARAM, before any device is touched, for
 * a NULL table, source or destination, ntracks < 1, nch < 1, an unknown format, ntracks * row_frames * nch of 2^60 samples or
 * more, and the filter, ceiling, lookahead, hold, work and overlap refusals of RRX_limit_device; the rest as there.
 * row_frames == 0 is RR_OK and does nothing. */
int RRX_tracks_limit_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch,
                            int src_format, const void *d_rows, int dst_format, void *d_dst_rows, size_t row_frames,
                            const double *d_gain, double ceiling, const double *coefs, int phases, int taps,
                            size_t lookahead, size_t hold, double *d_reduction, unsigned long long *d_limited,
                            double *d_work, size_t work_doubles);
/* Test hook (host only, needs no device), refused with -1 unless RSMP_TEST_HOOKS is set as above: RRX_limit_device on HOST
 * pointers, as serial loops over the very per-frame functions the kernels call.  Same refusals, same results. */
int RRX_debug_limit_host(int src_format, const void *src, size_t src_stride, int dst_format, void *dst, size_t dst_stride,
                         int nstreams, size_t frames, int nch, const double *gain, double ceiling,
                         const double *coefs, int phases, int taps, size_t lookahead, size_t hold,
                         double *reduction, unsigned long long *limited, double *work, size_t work_doubles);

/* The limiter with an exponential RELEASE: RRX_limit_device with a one-pole recursion between the window minimum and the box, so
 * that after a transient the gain recovers along an exponential of tens to hundreds of milliseconds instead of a ramp of L frames.
 * One step of a release is the map x -> min(t, a*x + u), and such maps are closed under composition,
 *   min(t2, a2*min(t1, a1*x + u1) + u2) = min(min(t2, a2*t1 + u2), a2*a1*x + (a2*u1 + u2)),
 * so a block of frames collapses into three numbers and the recursion runs as a block scan: every block summarised from nothing,
 * a short serial carry over the summaries, every block run again from its true start state.
 *
 * The arithmetic is part of this ABI, the block decomposition included: fp64, every operation rounded on its own, no fused
 * multiply-add.  g, tp, a[F], lev, r and m[k] are RRX_limit_device's, word for word.  Index the entries of m as v[j] = m[j - (L-1)],
 * j in [0, J), J = N + L - 1.  `release` is the per-frame pole a in [0, 1) (exp(-1 / (seconds * rate)) for a time constant),
 * b = 1.0 - a computed once on the host, and `block` the entries of a block, RRX_LIMIT_RELEASE_MIN_BLOCK..MAX_BLOCK, not
 * necessarily a power of two.  Block i holds the entries [i*block, min((i+1)*block, J)), nb = ceil(J / block) blocks:
 *   summary of block i with entries v_0 .. v_{n-1}:
 *       C = v_0;  A = a;  B = b * v_0
 *       for t = 1 .. n-1:  u = b * v_t;  C = fmin(v_t, a * C + u);  A = a * A;  B = a * B + u
 *   carry:  S_0 = 1.0;  S_{i+1} = fmin(C_i, A_i * S_i + B_i)            (blocks ascending)
 *   run of block i:  p = S_i;  for t = 0 .. n-1:  u = b * v_t;  p = fmin(v_t, a * p + u);  q[i*block + t] = p
 * The start state of block i+1 is the carry's S_{i+1}, NOT the last p of block i: the two differ in rounding.  The rest is
 * RRX_limit_device's with q in place of m: acc sums q[n - i] for i = L-1 down to 0 (as entries: q[n + L-1 - i]),
 * s[n] = fmin(acc * invL, q[n]), y = g * s, and the statistics are as there.
 * What holds.  q[j] <= v[j] always, so s[n] <= m[n]: the sample-peak bound |y| <= c * (1 + 2^-51) of RRX_limit_device holds
 * unchanged, and what is said there of the TRUE peak holds too.  m is never a NaN, so q is never a NaN.  The release is towards
 * the target, a*p + b*v, not towards 1.0: the gain recovers from the +0.0 that an infinite sample demands.  With release == 0.0
 * the call leaves RRX_limit_device's bytes and statistics exactly (b = 1 and fmin(v, 0*p + v) = v).  The blocked form is NOT bit-equal
 * to the plain serial recursion p = fmin(v_j, a*p + b*v_j) run from 1.0: over the cases of tests/test_limit_release_api.py the
 * largest relative difference of q between the two is 6.8e-13, where the gain recovers from +0.0 and q is small against the sums it is read from ("Limiter: release"); it is zero wherever a minimum
 * takes v_j, which forgets the state.  A_i + B_i need not round to 1.0 where nothing demands a reduction: behind the first block
 * a gain can sit one rounding below 1.0, and d_limited counts such frames too (it is not below RRX_limit_device's count).
 *   d_work: at least RRX_limit_release_work_doubles(nstreams, frames, taps, lookahead, block) doubles on the device, which is
 *   nstreams * (2 * (frames + taps + lookahead) + 4 * (ceil((frames + lookahead - 1) / block) + 1)) -- r, m and the blocks' C, A, B, S
 *   per stream -- or 0 for arguments the call would refuse and for a total of 2^60 doubles or more (host only).  Its content after
 *   the call is unspecified.
 *   Launches: RRX_limit_device's detector and window minimum, then summary (one lane per (stream, block), walking its block in
 *   register tiles), carry (one lane per stream) and run (the summary's lanes, q over m in place), then RRX_limit_device's
 *   smoothing and product.  The call only enqueues: no allocation, no host synchronisation; nothing outside the rows' frames of the
 *   destination, the work buffer and the two result arrays is written.
 * Everything else -- formats, strides, in place, d_gain, coefs, d_reduction, d_limited, device, hip_stream -- is RRX_limit_device's.
 * Returns RR_INVPARAM, before any device is touched, for everything RRX_limit_device refuses, a release that is a NaN, below 0 or
 * not below 1, a block outside its range, and d_work NULL or work_doubles too small; RR_EXTUNINIT before init_ratelib; RR_INTERNAL
 * for a failed launch.  frames == 0 is RR_OK and touches nothing. */
#define RRX_LIMIT_RELEASE_MIN_BLOCK 64
#define RRX_LIMIT_RELEASE_MAX_BLOCK 65536
size_t RRX_limit_release_work_doubles(int nstreams, size_t frames, int taps, size_t lookahead, size_t block);
int RRX_limit_release_device(int device, void *hip_stream, int src_format, const void *d_src, size_t src_stride,
                             int dst_format, void *d_dst, size_t dst_stride, int nstreams, size_t frames, int nch,
                             const double *d_gain, double ceiling, const double *coefs, int phases, int taps,
                             size_t lookahead, size_t hold, double release, size_t block, double *d_reduction,
                             unsigned long long *d_limited, double *d_work, size_t work_doubles);
/* RRX_limit_release_device per track of a ragged batch in one call, as RRX_tracks_limit_device is to RRX_limit_device: every
 * track's slice is limited as a one-stream call of its own -- blocks count from the slice's own entry j = 0, the state 1.0 is in
 * front of it -- and the table is clamped as there: a wrong table gives wrong samples, never an access outside the rows or d_work.
 * d_work: RRX_limit_release_work_doubles(ntracks, row_frames, taps, lookahead, block) doubles.  Refusals: RRX_tracks_limit_device's
 * and those of release, block and the work buffer above.  row_frames == 0 is RR_OK and does nothing. */
int RRX_tracks_limit_release_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch,
                                    int src_format, const void *d_rows, int dst_format, void *d_dst_rows, size_t row_frames,
                                    const double *d_gain, double ceiling, const double *coefs, int phases, int taps,
                                    size_t lookahead, size_t hold, double release, size_t block, double *d_reduction,
                                    unsigned long long *d_limited, double *d_work, size_t work_doubles);
/* Test hook (host only, needs no device), refused with -1 unless RSMP_TEST_HOOKS is set as above: RRX_limit_release_device on HOST
 * pointers, as serial loops over the very per-step functions the kernels call.  Same refusals, same results. */
int RRX_debug_limit_release_host(int src_format, const void *src, size_t src_stride, int dst_format, void *dst, size_t dst_stride,
                                 int nstreams, size_t frames, int nch, const double *gain, double ceiling,
                                 const double *coefs, int phases, int taps, size_t lookahead, size_t hold, double release,
                                 size_t block, double *reduction, unsigned long long *limited, double *work, size_t work_doubles);

/* Programme loudness (ITU-R BS.1770-4, EBU R 128): K-weighted energies of 100 ms hops per (stream, channel) of device-resident
 * frames, from which RRX_loudness_gate_device below takes the gated mean; in LUFS once the caller takes -0.691 + 10 log10.  The
 * call needs no handle and writes no sample.
 *
 * K-weighting is two biquads, an IIR recursion: a channel is one serial chain from its first frame, and restarting the state on a
 * grid would falsify the measurement (the 38 Hz high-pass has a pole radius of 0.995 at 48 kHz).  To give the device independent
 * chains all the same, the arithmetic that is part of this ABI is an exact BLOCK DECOMPOSITION by linear superposition, not the
 * serial filter; it agrees with the serial filter to rounding ("Loudness").  Everything is fp64, every operation is
 * rounded on its own, and there is no fused multiply-add.
 *   coefs: a HOST pointer to 10 finite doubles, copied into the launch arguments: stage A is c0..c4 = b0, b1, b2, a1, a2, stage B
 *   is c5..c9, both in transposed direct form II.  The call designs no filter (the Python binding has k_weighting(rate)).
 *   step        per channel, with state s[0..3] and g = (double)x * d_gain[s]  (d_gain NULL: g = x), as in RRX_finish_device:
 *                 y = c0*g + s0;   s0' = (c1*g - c3*y) + s1;   s1' = c2*g - c4*y;
 *                 v = c5*y + s2;   s2' = (c6*y - c8*v) + s3;   s3' = c7*y - c9*v;          E = E + v*v
 *   hop         the 100 ms piece, rate / 10 frames; any value >= 1 is accepted.  Hop k of a channel covers the absolute frames
 *               [k*hop, (k+1)*hop).
 *   The decomposition, with S_k the state at the start of hop k and S_0 = +0.0:
 *     z_k       the state after running the step over hop k from an all-zero state.
 *     A         the 4x4 matrix whose column i is one step with g = 0 from the unit state e_i, computed by the very step above.
 *     M = A^hop computed on the host by square-and-multiply over the bits of hop from the most significant one: R = A; then for
 *               every lower bit R = R R and, where the bit is set, R = R A.  Each entry of a product X Y is the ascending-k sum
 *               acc = +0.0; acc = acc + X[i][k]*Y[k][j], products and sums rounded separately.
 *     carry     S_{k+1}[i] = (((M[i][0]*S_k[0] + M[i][1]*S_k[1]) + M[i][2]*S_k[2]) + M[i][3]*S_k[3]) + z_k[i].
 *     energy[k] the serial ascending sum E from +0.0, over hop k, of the step started from S_k.
 *   Launches: one lane per (stream, channel, hop) computes z_k into d_work; one lane per (stream, channel) walks k ascending and
 *   turns d_work into S_k in place; the first layout again reruns every hop from S_k and writes its energy.  M travels in the
 *   launch arguments.  The call only enqueues -- no allocation, no host synchronisation -- hence the caller's d_work: at least
 *   RRX_loudness_work_doubles(nstreams, nch, frames, hop) doubles on the device (nstreams * nch * (frames / hop) * 4; host only,
 *   0 for arguments the call would refuse), whose content after the call is unspecified.
 *   Only whole hops are processed: n = frames / hop.  The frames behind the last whole hop are not read into anything; a chunked
 *   caller feeds them again.  first_frame % hop != 0 is RR_INVPARAM.
 *   State: [nstreams * nch][4] doubles on the device, s[0..3] of every channel.  d_state_in is required when first_frame > 0 and
 *   is not read at first_frame == 0.  d_state_out, when not NULL, receives S after the call's last whole hop; with n == 0 it
 *   receives a copy of d_state_in, or zeros when that is NULL or not read.  The two must not overlap (RR_INVPARAM, equal pointers
 *   included).  Contiguous calls cut at hop multiples that hand the state on leave the bits of one call.
 *   d_energy: hop first_frame / hop + j of channel c = s * nch + ch is WRITTEN, not accumulated, at
 *   d_energy[c * energy_stride + first_frame / hop + j], j < n.  Nothing else in d_energy is touched.
 *   A NaN or +-inf sample poisons its channel's state and with it every later energy of that channel (the gate then skips the
 *   blocks they enter); it never faults, and the other channels are exact.
 *   Everything else -- src_format (RRX_FMT_FLOAT or RRX_FMT_DOUBLE; integer sources are not offered), layouts and strides, the
 *   alignment of one sample, device and hip_stream with the stream-ordering contract -- is RRX_finish_device's.
 * Returns RR_INVPARAM, before any device is touched, for every source, stride, size and overflow RRX_finish_device refuses, and
 * further for coefs NULL, a non-finite coefficient, hop == 0, d_energy NULL, first_frame / hop + n > energy_stride, nstreams * nch *
 * energy_stride of 2^60 doubles or more, work_doubles below RRX_loudness_work_doubles(...) (or d_work NULL where that is not 0),
 * and the state rules above; RR_EXTUNINIT before init_ratelib; RR_INTERNAL for a failed launch.  frames == 0 is RR_OK and touches
 * nothing, the state included. */
int RRX_loudness_device(int device, void *hip_stream, int src_format, const void *d_src, size_t src_stride, int nstreams,
                        size_t frames, int nch, const double *d_gain, unsigned long long first_frame,
                        const double *coefs, size_t hop, const double *d_state_in, double *d_state_out,
                        double *d_energy, size_t energy_stride, double *d_work, size_t work_doubles);
size_t RRX_loudness_work_doubles(int nstreams, int nch, size_t frames, size_t hop);
/* Test hook (host only, needs no device), refused with -1 unless RSMP_TEST_HOOKS is set as above: RRX_loudness_device on HOST
 * pointers, as serial loops over the very step, carry and matrix functions the kernels use.  Same refusals, same results. */
int RRX_debug_loudness_host(int src_format, const void *src, size_t src_stride, int nstreams, size_t frames, int nch,
                            const double *gain, unsigned long long first_frame, const double *coefs, size_t hop,
                            const double *state_in, double *state_out, double *energy, size_t energy_stride,
                            double *work, size_t work_doubles);

/* RRX_loudness_device per track of a ragged batch in one call.  Tables, rows and their clamping are RRX_tracks_true_peak_device's:
 * track t's slice is frames [out_first, out_first + out_frames) of row t of d_rows ([ntracks][row_frames][nch], float32 or
 * float64), clamped to the row.  Track t is measured as a one-stream RRX_loudness_device call on that slice with first_frame = 0,
 * no state and d_gain[t] (d_gain NULL: unity): its hops go to d_energy[(t * nch + ch) * energy_stride + j], and d_hops[t]
 * (unsigned 64-bit, [ntracks], on the device, WRITTEN) is their number, the clamped out_frames / hop, itself clamped to
 * energy_stride.  Energies at index d_hops[t] and beyond are left untouched.  The row in front of the slice is not history.
 * d_work: at least RRX_loudness_work_doubles(ntracks, nch, row_frames, hop) doubles.  A wrong table gives wrong numbers, never an
 * access outside the rows, d_energy or d_work.
 * Refusals: RR_INVPARAM, before any device is touched, for a NULL table, source, d_energy or d_hops, ntracks < 1, nch < 1, an
 * unknown source format, the filter and work refusals of RRX_loudness_device, ntracks * row_frames * nch or ntracks * nch *
 * energy_stride of 2^60 or more, or device < -1; the rest as there.  row_frames == 0 is RR_OK and does nothing.  The form by
 * windows, with the hop in progress carried per track, is RRX_tracks_loudness_window_device. */
int RRX_tracks_loudness_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch, int src_format,
                               const void *d_rows, size_t row_frames, const double *d_gain, const double *coefs, size_t hop,
                               double *d_energy, size_t energy_stride, unsigned long long *d_hops,
                               double *d_work, size_t work_doubles);

/* RRX_loudness_device per track of a library at rest.  The packed source, its four formats, the clamp of the table (first, frames,
 * max_frames) and the exact sample value v are RRX_tracks_true_peak_packed_device's, word for word.  Track t is measured as a
 * one-stream RRX_loudness_device call on a float64 buffer holding its v, with first_frame = 0, no state and d_gain[t] (d_gain
 * NULL: unity): its hops go to d_energy[(t * nch + ch) * energy_stride + j], bit for bit, and d_hops[t] (unsigned 64-bit,
 * [ntracks], on the device, WRITTEN) = min(frames / hop, energy_stride) with the clamped frames.  Energies at index d_hops[t] and
 * beyond are left untouched.  d_work: at least RRX_loudness_work_doubles(ntracks, nch, max_frames, hop) doubles.  A wrong table
 * gives wrong numbers, never an access outside d_packed, d_energy or d_work.  Reads: an S24_3 source of one or two channels is
 * loaded as the aligned dwords that cover the samples, so the pass may READ, as RRX_tracks_stage_device_samples may, the aligned
 * dword that holds the first byte of the source and the one that holds its last byte in full (up to 3 bytes on either side, in
 * the same page: this cannot fault) and nothing further out; every other source is read by exactly its samples' bytes.  The meter calls (RRX_loudness_blocks_device and the
 * two group calls) read only hop energies and take these as they take RRX_tracks_loudness_device's.
 * Refusals: RR_INVPARAM, before any device is touched, for a NULL table, source, d_energy or d_hops, ntracks < 1, nch < 1, a format
 * outside the four (RRX_FMT_DOUBLE included), the filter, hop and work refusals of RRX_loudness_device, src_total * nch, ntracks *
 * max_frames * nch or ntracks * nch * energy_stride of 2^60 or more, or device < -1; the rest as there.  max_frames == 0 or
 * src_total == 0 is RR_OK and does nothing. */
int RRX_tracks_loudness_packed_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch,
                                      int src_format, const void *d_packed, size_t src_total, size_t max_frames,
                                      const double *d_gain, const double *coefs, size_t hop, double *d_energy,
                                      size_t energy_stride, unsigned long long *d_hops, double *d_work, size_t work_doubles);
/* Test hook (host only, needs no device), refused with -1 unless RSMP_TEST_HOOKS is set as above: the call above on HOST
 * pointers, as serial loops over the same clamp, the same one-sample load and the same per-frame functions as the kernels. */
int RRX_debug_tracks_loudness_packed_host(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *packed,
                                          size_t src_total, size_t max_frames, const double *gain, const double *coefs,
                                          size_t hop, double *energy, size_t energy_stride, unsigned long long *hops,
                                          double *work, size_t work_doubles);

/* The two-stage gate of BS.1770-4 over the hop energies of RRX_loudness_device / RRX_tracks_loudness_device: 400 ms blocks of
 * four hops, overlapping by 75 %.  The arithmetic is part of this ABI (fp64, every operation rounded on its own).  Stream s has
 * n = nhops hops, or min(d_hops[s], nhops) when d_hops (device, [nstreams]) is not NULL; its channel ch has its hops at
 * e = d_energy + (s * nch + ch) * energy_stride.  Block j runs over [0, n - 3); nothing passes if n < 4.
 *   per channel   q = ((e[j] + e[j+1]) + e[j+2]) + e[j+3]
 *   block         acc = +0.0, then ascending channels acc = acc + w[ch]*q (d_weights NULL: acc = acc + q);  z_j = acc * inv,
 *                 inv = 1.0 / (4.0 * (double)hop), computed once on the host
 *   pass A        j ascending and serial, over the blocks with z_j > abs_threshold: S1 (sum) and N1 (count)
 *   threshold     T = rel_factor * (S1 / N1), the division correctly rounded
 *   pass B        S2 and N2 over the blocks with z_j > abs_threshold && z_j > T
 *   d_result[s] = {S2, (double)N2, S1, (double)N1}, [nstreams][4] doubles on the device, written.
 * A NaN z_j fails every comparison and is skipped.  The caller takes -0.691 + 10 log10(S2 / N2); BS.1770's gates are
 * abs_threshold = 10^((-70 + 0.691) / 10) and rel_factor = 10^(-10 / 10).  No libm runs on the device.
 * Returns RR_INVPARAM, before any device is touched, for d_energy or d_result NULL, nstreams < 1, nch < 1, hop == 0,
 * nhops > energy_stride, nstreams * nch * energy_stride of 2^60 or more, a NaN threshold or factor, or device < -1; the rest as
 * RRX_finish_device.  The call only enqueues. */
int RRX_loudness_gate_device(int device, void *hip_stream, const double *d_energy, size_t energy_stride, int nstreams, int nch,
                             size_t nhops, const unsigned long long *d_hops, const double *d_weights, size_t hop,
                             double abs_threshold, double rel_factor, double *d_result);
/* Test hook (host only, needs no device), refused with -1 unless RSMP_TEST_HOOKS is set as above: the gate on HOST pointers, as a
 * serial loop over the very block function the kernel calls. */
int RRX_debug_loudness_gate_host(const double *energy, size_t energy_stride, int nstreams, int nch, size_t nhops,
                                 const unsigned long long *hops, const double *weights, size_t hop,
                                 double abs_threshold, double rel_factor, double *result);

/* The loudness meter: what EBU R 128 and ReplayGain 2.0 ask for beyond the integrated loudness of one stream, from the same hop
 * energies.  Three calls; all fp64, every operation rounded on its own, part of this ABI.  All only enqueue -- no allocation, no
 * host synchronisation, work buffers from the caller -- and take device and hip_stream with RRX_finish_device's contract.  No libm
 * runs on the device: the caller takes the logarithms.
 *
 * RRX_loudness_blocks_device: sliding block powers of L = block_hops hops every P = step_hops hops, and their maximum.  Energies,
 * strides, d_hops, d_weights and hop as in RRX_loudness_gate_device.  Stream s with n = min(d_hops[s], nhops) valid hops has
 *   nb = 0 if n < L, else (n - L) / P + 1, clamped to blocks_stride when d_blocks is given;   d_nblocks[s] = nb
 *   block j begins at hop j*P:   per channel   q = e[jP], then q = q + e[jP+i] for i = 1 .. L-1 ascending
 *                                block         acc = +0.0, then ascending channels acc = acc + w[ch]*q (d_weights NULL: acc + q);
 *                                              z_j = acc * inv,  inv = 1.0 / ((double)L * (double)hop), computed once on the host
 *   d_blocks[s * blocks_stride + j] = z_j for j < nb; nothing else of d_blocks is touched
 *   d_max[s]: m = +0.0, then if (z_j > m) m = z_j over all j < nb.  A NaN fails the comparison and is skipped; the result does not
 *   depend on the order and is reduced in parallel.  No block gives +0.0, which is -inf LUFS.
 * With L = 4 and P = 1 the z_j have the bits of RRX_loudness_gate_device's blocks.  (4, 1) is momentary loudness, (30, 1)
 * short-term; (30, 10) are the 3 s blocks every 1 s that loudness range is commonly computed on.  d_blocks ([nstreams][blocks_stride]
 * doubles), d_nblocks ([nstreams] unsigned 64-bit) and d_max ([nstreams] doubles) may each be NULL, not all three.
 * Returns RR_INVPARAM, before any device is touched, for what RRX_loudness_gate_device refuses of these arguments, and for
 * block_hops == 0, step_hops == 0, all three outputs NULL, blocks_stride == 0 with d_blocks given, or nstreams * blocks_stride of
 * 2^60 or more; RR_EXTUNINIT before init_ratelib; RR_INTERNAL for a failed launch. */
int RRX_loudness_blocks_device(int device, void *hip_stream, const double *d_energy, size_t energy_stride, int nstreams, int nch,
                               size_t nhops, const unsigned long long *d_hops, const double *d_weights, size_t hop,
                               size_t block_hops, size_t step_hops, double *d_blocks, size_t blocks_stride,
                               unsigned long long *d_nblocks, double *d_max);

/* RRX_loudness_gate_groups_device: the two-stage gate of BS.1770-4 over the POOLED blocks of groups of streams -- the album gain of
 * ReplayGain 2.0.  d_blocks, blocks_stride and d_nblocks (required, read clamped to blocks_stride) are what the call above left;
 * they may have been collected from several batches.  d_group ([nstreams] int32 on the device) gives stream s's group in
 * [0, ngroups); any other value means "in no group", and never faults.  The arithmetic is defined by this structure, not by the
 * launch geometry:
 *   per stream   j ascending and serial, from +0.0 and 0: S1_s and N1_s over the blocks with z > abs_threshold
 *   per group    member streams in ascending s, serial, from +0.0: S1 = S1 + S1_s, N1 += N1_s;  T = rel_factor * (S1 / N1)
 *   per stream   S2_s and N2_s over the blocks with z > abs_threshold && z > T, T its group's
 *   per group    S2 and N2 the same way
 *   d_result[g] = {S2, (double)N2, S1, (double)N1}, [ngroups][4] doubles on the device, written; the counts are exact integers.
 * An empty group gives {+0.0, 0, +0.0, 0}; its T is NaN, as in RRX_loudness_gate_device with N1 = 0.
 * A group of exactly ONE stream, over (4, 1) blocks, has the bits of RRX_loudness_gate_device on that stream: +0.0 + x is x for
 * the non-negative sums.  Streams run in parallel: a whole library in one group costs its longest stream's serial walk, not the
 * library's.
 * d_work: at least RRX_loudness_groups_work_doubles(nstreams, ngroups) doubles on the device (host only; 0 for refused arguments;
 * it depends on the two counts only, never on the blocks), content unspecified after the call.
 * Returns RR_INVPARAM, before any device is touched, for d_blocks, d_nblocks, d_group, d_result or d_work NULL, nstreams < 1,
 * ngroups < 1, nstreams * blocks_stride of 2^60 or more, a NaN threshold or factor, work_doubles too small, or device < -1; the
 * rest as above. */
size_t RRX_loudness_groups_work_doubles(int nstreams, int ngroups);
int RRX_loudness_gate_groups_device(int device, void *hip_stream, const double *d_blocks, size_t blocks_stride, int nstreams,
                                    const unsigned long long *d_nblocks, const int *d_group, int ngroups,
                                    double abs_threshold, double rel_factor, double *d_result, double *d_work, size_t work_doubles);

/* RRX_loudness_range_groups_device: gated percentiles per group by exact selection -- loudness range (EBU Tech 3342) is
 * 10 log10(P_high / P_low) on the caller's side.  Arguments as in the call above.  T, and the multiset G of the group's blocks
 * with z > abs_threshold && z > T, are exactly that call's.  With n = |G| and G sorted ascending by value:
 *   P_low = G[((n-1)*pct_low + 50) / 100],  P_high = G[((n-1)*pct_high + 50) / 100]     (integer arithmetic, 0-based: Tech 3342's
 *   round((n-1)*p/100 + 1), 1-based)
 *   d_result[g] = {P_low, P_high, (double)n, T};  n == 0 gives {+0.0, +0.0, 0, T}.
 * abs_threshold < 0 is refused: every element of G is then a positive double or +inf, whose order is the order of its bit pattern
 * as an unsigned 64-bit integer, and equal values have equal bits, so the result is unique.  The device finds it by a radix
 * select on those patterns, one workgroup per group: most significant byte first, a histogram per pass in LDS (integer counts
 * do not depend on the order of arrival), both ranks carried through the same eight passes, the stream list walked per pass -- no
 * sort, no buffer proportional to the block count, no limit on n; the counts are 64-bit.  Tech 3342 uses
 * abs_threshold = 10^((-70 + 0.691) / 10), rel_factor = 10^(-20 / 10) and the percentiles 10 and 95.
 * Refusals: those of the call above, and pct_low or pct_high outside 0..100 or abs_threshold < 0. */
int RRX_loudness_range_groups_device(int device, void *hip_stream, const double *d_blocks, size_t blocks_stride, int nstreams,
                                     const unsigned long long *d_nblocks, const int *d_group, int ngroups,
                                     double abs_threshold, double rel_factor, int pct_low, int pct_high,
                                     double *d_result, double *d_work, size_t work_doubles);
/* Test hooks (host only, need no device), refused with -1 unless RSMP_TEST_HOOKS is set as above: the three calls on HOST pointers,
 * as serial loops over the very functions the kernels call (the range twin sorts).  Same refusals, same results. */
int RRX_debug_loudness_blocks_host(const double *energy, size_t energy_stride, int nstreams, int nch, size_t nhops,
                                   const unsigned long long *hops, const double *weights, size_t hop,
                                   size_t block_hops, size_t step_hops, double *blocks, size_t blocks_stride,
                                   unsigned long long *nblocks, double *max);
int RRX_debug_loudness_gate_groups_host(const double *blocks, size_t blocks_stride, int nstreams, const unsigned long long *nblocks,
                                        const int *group, int ngroups, double abs_threshold, double rel_factor,
                                        double *result, double *work, size_t work_doubles);
int RRX_debug_loudness_range_groups_host(const double *blocks, size_t blocks_stride, int nstreams, const unsigned long long *nblocks,
                                         const int *group, int ngroups, double abs_threshold, double rel_factor,
                                         int pct_low, int pct_high, double *result, double *work, size_t work_doubles);

/* Windows: the two passes above on frames [win_first, win_first + win_frames) of the rows, so that a ragged batch runs in memory
 * proportional to ntracks * window instead of ntracks * longest track.  The rows themselves are VIRTUAL: row_frames is their
 * length, and no buffer of that size exists.  A handle's output does not depend on how its input is cut into pushes, and dither,
 * peak and clip count are functions of the absolute frame, so staging window after window into one buffer, pushing it, pulling into
 * a second one and finishing that at the running output position gives the bytes and statistics of the whole-row calls.
 *
 * RRX_tracks_stage_window_device: d_win is [ntracks][win_stride][nch] float32.  For j in [0, win_frames), d_win[t][j] receives, bit
 * for bit, frame win_first + j of row t as RRX_tracks_stage_device_samples writes it for the same table, source and row_frames: the
 * copied track, both LPC extensions, the zeros behind ext, and the clamps under a wrong table.  Every frame of the window is written
 * exactly once; frames [win_frames, win_stride) of each window row and everything outside d_win are untouched; d_packed is only
 * read, under the read contract of RRX_tracks_stage_device_samples (whole aligned dwords at the two ends of the source, nothing
 * further out), in all four source formats.  An LPC extension is a serial recursion from the track's edge outwards, so a window that
 * begins inside one recomputes it from its start: split rows into windows of thousands of frames, not dozens.
 * device, hip_stream, stream ordering, "only enqueues", refusals and return values: RRX_tracks_stage_device_samples's (with d_win
 * for d_rows), and RR_INVPARAM, before any device is touched, also for win_first + win_frames above row_frames (or wrapping),
 * win_stride < win_frames, or ntracks * win_stride * nch of 2^60 samples or more.  win_frames == 0 is RR_OK and does nothing. */
int RRX_tracks_stage_window_device(int device, void *hip_stream, size_t in_rate, size_t out_rate, const RRX_track *d_tracks,
                                   int ntracks, int nch, int src_format, const void *d_packed, size_t src_total, size_t row_frames,
                                   size_t win_first, size_t win_frames, fb_sample_t *d_win, size_t win_stride);

/* RRX_tracks_finish_window_device: d_win ([ntracks][win_stride][nch], float32 or float64) holds, at d_win[t][j], frame win_first + j
 * of output row t; row_frames is the virtual pitch the whole-row call clamps to.  Of track t's slice [out_first, out_first +
 * out_frames), clamped exactly as RRX_tracks_finish_device clamps it, the frames inside the window are processed: frame r of the row
 * has dither index i = r - out_first -- counted from the track's own first output frame, not from the window -- and goes to frame
 * dst_first + i of the destination.  d_peak and d_clipped accumulate.  So any set of disjoint windows that covers [0, row_frames),
 * in any order, leaves the bytes and statistics of one RRX_tracks_finish_device call.  Exactly the bytes of the processed samples
 * are written: a window may begin or end at any byte offset of the packed destination, and the neighbouring sample of the same
 * track may belong to another window's call.  d_dst NULL measures only.
 * Refusals: RRX_tracks_finish_device's (with d_win for d_rows) and the three window refusals above.  row_frames == 0 or
 * win_frames == 0 is RR_OK and does nothing. */
int RRX_tracks_finish_window_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch, int src_format,
                                    const void *d_win, size_t win_stride, size_t row_frames, size_t win_first, size_t win_frames,
                                    int dst_format, void *d_dst, size_t dst_total, const double *d_gain, int dither,
                                    unsigned long long seed, double *d_peak, unsigned long long *d_clipped);
/* RRX_tracks_finish_shaped_device by windows: RRX_tracks_finish_window_device with noise-shaped dither.  The error history of a
 * channel runs on from one window into the next, so the call takes and returns a per-(track, channel) STATE, and -- unlike the
 * unshaped window call -- it depends on the order of the calls.
 *   Frames taken.  d_win, win_stride, row_frames, win_first, win_frames and the clamps under a wrong table are
 *   RRX_tracks_finish_window_device's, through the same function: of track t's slice [out_first, out_first + out_frames), clamped
 *   as there, the frames inside the window are processed.  They are frames index, index + 1, ... of the slice (index = the first
 *   one's row frame - out_first) and go to frames dst_first + index, ... of the destination.  Exactly the bytes of the processed
 *   samples are written, at any byte offset; d_peak and d_clipped accumulate.
 *   Arithmetic.  Track t's processed frames get the bytes and statistics of a one-stream RRX_finish_shaped_device call on them
 *   with first_frame = index, seed + t * nch * 0xBF58476D1CE4E5B9 (mod 2^64) for seed, d_gain[t], the same coefs, order, segment,
 *   dither and dst_format, and track t's entries of d_state_in as the incoming state.  Segments and the dither index are counted
 *   from the track's own first output frame, never from the window: the history of a channel is all +0.0 at index == 0 and at
 *   every index % segment == 0 (segment != 0), so a window cuts every track's segments at a different place.
 *   State.  d_state_in and d_state_out are [ntracks * nch][RRX_SHAPE_MAX_ORDER] doubles on the device; entry k-1 of a channel is
 *   e[k], entries at `order` and beyond are 0.  d_state_in is read for a track only when that track's first processed frame of
 *   this call lies inside a segment.  Every call with win_frames > 0 and row_frames > 0 writes EVERY entry of d_state_out (when
 *   it is not NULL): for a track with processed frames in this window the history after its last one; for a track with none (not
 *   begun, already ended, zero length) a copy of its d_state_in entries, or zeros when d_state_in is NULL.  A caller therefore
 *   ping-pongs two buffers without knowing which tracks a window touched.  d_state_in NULL is allowed only with win_first == 0 --
 *   no track can have begun earlier -- and is RR_INVPARAM otherwise; the table is device memory, so this is the only check the
 *   host can make.  The two buffers must not overlap over ntracks * nch * 16 doubles (RR_INVPARAM, equal pointers included), for
 *   the reason RRX_finish_shaped_device gives.  d_state_out may be NULL.
 *   Order of calls.  The promise "the bytes and statistics of one RRX_tracks_finish_shaped_device call, bit for bit, for any cut
 *   positions" holds ONLY when the windows partition [0, row_frames), are processed in ascending, contiguous order, and each
 *   call's d_state_out is the next call's d_state_in.  Anything else -- windows out of order, a gap, an overlap, a state from
 *   somewhere else -- gives other samples, never an access outside the buffers.
 *   Identities.  With order = 1 and coefs[0] = 0.0 it is RRX_tracks_finish_window_device, bit for bit, with and without dither.
 *   d_dst NULL measures only; as in the other shaped calls dst_format must still be valid and its bits are used.
 * Returns RR_INVPARAM, before any device is touched, for everything RRX_tracks_finish_window_device refuses (the three window
 * refusals included), everything RRX_tracks_finish_shaped_device adds (coefs NULL, order outside 1..RRX_SHAPE_MAX_ORDER, a
 * non-finite coefficient, an unknown dst_format even with d_dst NULL) and the two state rules above.  row_frames == 0 or
 * win_frames == 0 is RR_OK and touches nothing, the state included.  The call only enqueues (no allocation, no host
 * synchronisation); device, hip_stream and stream ordering are the sibling calls'. */
int RRX_tracks_finish_shaped_window_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch,
                                           int src_format, const void *d_win, size_t win_stride, size_t row_frames,
                                           size_t win_first, size_t win_frames, int dst_format, void *d_dst, size_t dst_total,
                                           const double *d_gain, int dither, unsigned long long seed,
                                           const double *coefs, int order, size_t segment,
                                           const double *d_state_in, double *d_state_out,
                                           double *d_peak, unsigned long long *d_clipped);
/* Test hook (host only, needs no device), refused with -1 unless RSMP_TEST_HOOKS is set as above:
 * RRX_tracks_finish_shaped_window_device on HOST pointers and a HOST table, as one serial loop per (track, channel) over the very
 * functions the kernel calls for the cut and for every sample.  Same refusals, same results. */
int RRX_debug_tracks_finish_shaped_window_host(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *win,
                                               size_t win_stride, size_t row_frames, size_t win_first, size_t win_frames,
                                               int dst_format, void *dst, size_t dst_total, const double *gain, int dither,
                                               unsigned long long seed, const double *coefs, int order, size_t segment,
                                               const double *state_in, double *state_out, double *peak,
                                               unsigned long long *clipped);

/* RRX_tracks_true_peak_device by windows: the true peak and the sample peak of every track of a ragged batch, measured a window
 * of the output rows at a time.  The filter's history of a channel runs on from one window into the next, so the call takes and
 * returns a per-(track, channel) STATE and depends on the order of the calls, as RRX_tracks_finish_shaped_window_device does.
 *   Frames taken.  d_win, win_stride, row_frames, win_first, win_frames and the clamps under a wrong table are
 *   RRX_tracks_finish_window_device's in its measure-only form, through the same function: of track t's clamped slice the frames
 *   inside the window are processed; they are frames index, index + 1, ... of the slice.
 *   Arithmetic.  Track t's processed frames get the results of a one-stream RRX_true_peak_device call on them with
 *   first_frame = index, d_gain[t], the same filter, track t's entries of d_state_in as the history (read only when index > 0; at
 *   index == 0 the history is +0.0, whatever the row holds in front of the slice), and flush = 1 exactly when the window holds
 *   the slice's last frame.  The results accumulate into d_true_peak / d_peak [ntracks * nch] by the same unsigned 64-bit
 *   maximum; the flushed taps - 1 frames enter the true peak only, neither the sample peak nor the state.
 *   State.  d_state_in and d_state_out are [ntracks * nch][RRX_TP_MAX_TAPS] doubles on the device, laid out as in
 *   RRX_true_peak_device.  Every call with win_frames > 0 and row_frames > 0 writes EVERY entry of d_state_out (when it is not
 *   NULL): for a track with processed frames the history after its last processed real frame -- with fewer processed frames than
 *   taps - 1 a mix of new and incoming entries, entries at taps - 1 and beyond 0 --; for a track with none (not begun, already
 *   ended, zero length) a copy of its d_state_in entries, or zeros when d_state_in is NULL.  d_state_in NULL is allowed only with
 *   win_first == 0 and is RR_INVPARAM otherwise.  The two buffers must not overlap over ntracks * nch * 16 doubles (RR_INVPARAM,
 *   equal pointers included).  d_state_out may be NULL.
 *   Order of calls.  Windows that partition [0, row_frames), taken in ascending contiguous order, each given the state of the one
 *   before, leave the bits of ONE RRX_tracks_true_peak_device call in d_true_peak and d_peak, for any cut positions.  Anything
 *   else gives other numbers, never an access outside the buffers.
 * Returns RR_INVPARAM, before any device is touched, for everything RRX_tracks_true_peak_device refuses (with d_win for d_rows),
 * the three window refusals of RRX_tracks_stage_window_device and the two state rules above.  row_frames == 0 or win_frames == 0
 * is RR_OK and touches nothing, the state included.  The call only enqueues (no allocation, no host synchronisation): the LDS
 * form where nch * taps <= 4096 and nch <= 1024, the direct form otherwise, as RRX_true_peak_device. */
int RRX_tracks_true_peak_window_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch,
                                       int src_format, const void *d_win, size_t win_stride, size_t row_frames, size_t win_first,
                                       size_t win_frames, const double *d_gain, const double *coefs, int phases, int taps,
                                       const double *d_state_in, double *d_state_out, double *d_true_peak, double *d_peak);
/* RRX_tracks_loudness_device by windows: the K-weighted hop energies of every track of a ragged batch, measured a window of the
 * output rows at a time.  Hops are counted from each track's own first output frame, so a window cuts every track's hops at a
 * different place, usually mid-hop, and may be shorter than a hop; the state therefore carries a partial hop.
 *   Geometry.  With n = min(slice frames / hop, energy_stride) -- RRX_tracks_loudness_device's hop count -- the processed range of
 *   track t is the window's cut of its slice (as in RRX_tracks_true_peak_window_device) intersected with slice frames
 *   [0, n * hop): frames behind the last whole hop are never read.  With index the slice frame of the first processed one,
 *   k0 = index / hop and r0 = index % hop, the range meets the "pieces" hop k0 + j intersected with the range, j = 0, 1, ...; the
 *   first may begin mid-hop, the last may end mid-hop, and a range of m frames meets at most m / hop + 2 of them.
 *   State.  [ntracks * nch][RRX_LOUDNESS_WIN_STATE] doubles: [0..3] = S, the true filter state at the start of the hop in
 *   progress; [4..7] = Z, the state of the zero-started run after the r0 frames of that hop seen so far; [8..11] = C, the state of
 *   the run started from S after those frames; [12] = E, the partial energy of that run; [13..15] = +0.0.  On a hop boundary
 *   Z = 0, C = S and E = +0.0.  The state is read for a track only when index > 0.  Every call with win_frames > 0 and
 *   row_frames > 0 writes every entry of d_state_out (when not NULL); a track without a processed frame gets a copy of its
 *   d_state_in entries, or zeros when d_state_in is NULL.  d_state_in NULL only with win_first == 0, and no overlap of the two
 *   buffers over ntracks * nch * 16 doubles (RR_INVPARAM, equal pointers included).
 *   Arithmetic.  Three launches, RRX_loudness_device's block decomposition operation by operation.  (1) Every piece is run from
 *   Z of the state (a first piece with r0 > 0) or from zeros, its end state z left in d_work.  (2) Per (track, channel) the pieces
 *   are walked ascending from S of the state (+0.0 at index == 0): each piece's z is replaced by the start state of its hop,
 *   S = M S + z is applied for every hop that completes in this window, and S and the z of an unfinished last piece go to the
 *   state; d_hops[t] = n is written.  (3) Every piece is run again, a first piece with r0 > 0 from C and E of the state, every
 *   other from its S_k and E = +0.0; a piece whose hop completes WRITES d_energy[(t * nch + ch) * energy_stride + k0 + j], an
 *   unfinished last piece writes C and E to the state.  A serial sum cut in two gives the bits of the uncut sum, so under the
 *   order rule of RRX_tracks_true_peak_window_device the energies and d_hops are RRX_tracks_loudness_device's bit for bit, for any
 *   cut positions.  Energies of hops that did not complete in this call are left untouched.
 *   d_work: RRX_tracks_loudness_window_work_doubles(ntracks, nch, win_frames, hop) = ntracks * nch * (win_frames / hop + 2) * 4
 *   doubles of scratch (0 for ntracks < 1, nch < 1 or hop == 0).
 * Returns RR_INVPARAM, before any device is touched, for everything RRX_tracks_loudness_device refuses (with d_win for d_rows;
 * its work rule replaced by: work_doubles below the function above, or d_work NULL), the three window refusals and the two state
 * rules.  row_frames == 0 or win_frames == 0 is RR_OK and touches nothing, the state included.  The call only enqueues. */
#define RRX_LOUDNESS_WIN_STATE 16
size_t RRX_tracks_loudness_window_work_doubles(int ntracks, int nch, size_t win_frames, size_t hop);
int RRX_tracks_loudness_window_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch,
                                      int src_format, const void *d_win, size_t win_stride, size_t row_frames, size_t win_first,
                                      size_t win_frames, const double *d_gain, const double *coefs, size_t hop,
                                      const double *d_state_in, double *d_state_out, double *d_energy, size_t energy_stride,
                                      unsigned long long *d_hops, double *d_work, size_t work_doubles);
/* Test hooks (host only, need no device), refused with -1 unless RSMP_TEST_HOOKS is set as above: the two calls above on HOST
 * pointers and a HOST table, each as one serial loop per (track, channel) over the very functions the kernels call for the cut
 * and for every sample.  Same refusals, same results. */
int RRX_debug_tracks_true_peak_window_host(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *win,
                                           size_t win_stride, size_t row_frames, size_t win_first, size_t win_frames,
                                           const double *gain, const double *coefs, int phases, int taps, const double *state_in,
                                           double *state_out, double *true_peak, double *peak);
int RRX_debug_tracks_loudness_window_host(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *win,
                                          size_t win_stride, size_t row_frames, size_t win_first, size_t win_frames,
                                          const double *gain, const double *coefs, size_t hop, const double *state_in,
                                          double *state_out, double *energy, size_t energy_stride, unsigned long long *hops,
                                          double *work, size_t work_doubles);

/* RRX_tracks_limit_device by windows.  The limiter has nothing recursive in it, so a window needs no state from the one before,
 * only a HALO of input: the gain s[n] of RRX_limit_device depends on the samples of the frames [n - back, n + ahead] and on
 * nothing else, with
 *   back  = (L - 1) + H + D,   ahead = (L - 1) + D            (L = lookahead, H = hold, D = taps - 1)
 * because m[n - i], i < L, covers r[F] for F in [n - (L - 1) - H, n + L - 1 + D], and r[F] reads g[F - D .. F].
 * RRX_limit_window_reach (host only) gives the two numbers: RR_INVPARAM for a NULL pointer, taps outside 1..RRX_TP_MAX_TAPS,
 * lookahead outside 1..RRX_LIMIT_MAX_LOOKAHEAD or hold above RRX_LIMIT_MAX_HOLD.
 *
 * Geometry.  The rows are virtual, of row_frames frames, as in the other window calls; track t is its slice [out_first, out_first
 * + out_frames) of row t, clamped to the row as in RRX_tracks_limit_device.  d_buf, [ntracks][buf_stride][nch] of src_format,
 * holds the frames [buf_first, buf_first + buf_frames) of every row; d_dst is [ntracks][dst_stride][nch] of dst_format, and
 * d_dst[t][j] receives frame win_first + j.  Of every slice the frames inside [win_first, win_first + win_frames) are emitted.
 * Arithmetic.  The emitted frames are those of a one-stream RRX_limit_device call on the WHOLE slice under d_gain[t], restricted
 * to those frames: the history in front of the slice and behind it is +0.0, not what the buffer holds there.  Nothing else of
 * d_dst is written; d_buf is only read.  d_reduction and d_limited ([ntracks]) accumulate over the emitted frames as in the
 * whole-row call.  So any set of disjoint windows that covers [0, row_frames), in ANY order, each given the same d_reduction and
 * d_limited, leaves in the emitted frames the bits of one RRX_tracks_limit_device call, with the same two statistics.  The price
 * is that every window evaluates the detector on back + ahead frames more than it emits.
 * Coverage.  The buffer must hold the window and its halo as far as the row goes:
 *   buf_first <= max(0, win_first - back),   buf_first + buf_frames >= min(row_frames, win_first + win_frames + ahead),
 *   buf_first + buf_frames <= row_frames (and no wrap),   buf_stride >= buf_frames,   dst_stride >= win_frames.
 * In place is not offered -- the back halo of the next window must be unlimited input -- so any overlap of the extents of d_dst
 * and d_buf is refused.
 * d_work: at least RRX_tracks_limit_window_work_doubles(ntracks, win_frames, taps, lookahead, hold) doubles, which is
 * ntracks * 2 * (win_frames + 2 * lookahead + hold + 2 * taps) -- r needs win_frames + 2 L - 2 + H + D entries, m needs
 * win_frames + L - 1 -- or 0 for arguments the call refuses and for a product of 2^60 or more (host only).
 * A wrong table gives wrong samples, never an access outside d_buf, d_dst or d_work; a sample the arithmetic asks for that lies
 * outside the buffer reads as +0.0.  Three launches as in RRX_limit_device, each on the sub-range the window needs and split over
 * chunks of 32768 tracks.  The call only enqueues: no allocation, no host synchronisation; coefs, device and hip_stream as in
 * RRX_limit_device.
 * Returns RR_INVPARAM, before any device is touched, for a NULL table, buffer or destination, ntracks < 1, nch < 1, an unknown
 * format, ntracks * row_frames * nch or either buffer of 2^60 samples or more, a window that wraps or does not lie inside the
 * rows, a violation of the coverage rule, the overlap of d_dst and d_buf, and the filter, ceiling, lookahead, hold and work
 * refusals of RRX_limit_device (the work rule being the function above); the rest as there.  win_frames == 0 or row_frames == 0
 * is RR_OK and touches nothing. */
int RRX_limit_window_reach(int taps, size_t lookahead, size_t hold, size_t *back, size_t *ahead);
size_t RRX_tracks_limit_window_work_doubles(int ntracks, size_t win_frames, int taps, size_t lookahead, size_t hold);
int RRX_tracks_limit_window_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch,
                                   int src_format, const void *d_buf, size_t buf_stride, size_t buf_first, size_t buf_frames,
                                   size_t row_frames, size_t win_first, size_t win_frames, int dst_format, void *d_dst,
                                   size_t dst_stride, const double *d_gain, double ceiling, const double *coefs, int phases,
                                   int taps, size_t lookahead, size_t hold, double *d_reduction, unsigned long long *d_limited,
                                   double *d_work, size_t work_doubles);
/* Test hook (host only, needs no device), refused with -1 unless RSMP_TEST_HOOKS is set as above: the call above on HOST pointers
 * and a HOST table, as one serial loop per track over the very functions the kernels call.  Same refusals, same results. */
int RRX_debug_tracks_limit_window_host(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *buf,
                                       size_t buf_stride, size_t buf_first, size_t buf_frames, size_t row_frames,
                                       size_t win_first, size_t win_frames, int dst_format, void *dst, size_t dst_stride,
                                       const double *gain, double ceiling, const double *coefs, int phases, int taps,
                                       size_t lookahead, size_t hold, double *reduction, unsigned long long *limited,
                                       double *work, size_t work_doubles);

/* RRX_tracks_limit_release_device by windows: RRX_tracks_limit_window_device with the exponential release of
 * RRX_limit_release_device between the window minimum and the box.  The release is a recursion, so unlike the plain window call
 * this one takes and returns a per-track STATE and depends on the order of the calls.  The ABI of the release is its block
 * decomposition, and blocks are counted from each slice's own entry j = 0: a window cuts every track at a different place of its
 * block grid, usually mid-block.  The call keeps the track's ABSOLUTE block grid and carries the scan's intermediate state across
 * the cut, so that it leaves the bits of the whole-row call.
 *   Entries.  As in RRX_limit_release_device: v[j] = m[j - (L-1)], j in [0, J), J = N + L - 1 for a slice of N frames; the gain of
 *   slice frame n reads q[n .. n + L-1].  A call processes the slice frames [e0, e1) of track t, the window's cut of the clamped
 *   slice as in the other window calls (e0 is their `index`), and computes q on the entries [e0, e1 + L-1).
 *   State.  d_state_in and d_state_out are [ntracks][RRX_LIMIT_RELEASE_WIN_STATE] doubles on the device -- per track, not per
 *   channel: the limiter links channels.  A state describes the scan AT AN ENTRY e; it is read at e0 and written at e1.  With
 *   i = e / block and r = e % block:
 *     [0]    = S, the carry's S_i (1.0 at e = 0);
 *     [1..3] = C, A, B, the summary of the entries [i*block, e), built by the first-entry step and the extension step of
 *              RRX_limit_release_device in order; +0.0 when r == 0;
 *     [4]    = p, q[e - 1] run from S_i; S when r == 0;
 *     [5..7] = +0.0.
 *   Pieces.  The pieces of a call are the absolute blocks intersected with [e0, e1 + L-1).  A first piece with r0 = e0 % block > 0
 *   goes on from the state: its summary extends the state's (C, A, B), its run goes on from the state's p.  Every other piece is
 *   summarised from nothing and run from its S_i.  The carry starts from the state's S (1.0 at e0 == 0) and applies
 *   S_{i+1} = fmin(C_i, A_i*S_i + B_i) for every block that completes inside the range.
 *   Snapshot.  The outgoing state is written by the lanes that own the piece holding e1, as a snapshot WHILE THEY PASS e1:
 *   the piece is never split at e1.  A serial extension cut in two keeps its bits; a block summarised in two halves and composed
 *   does not.  Blocks that complete in the overlap [e1, e1 + L-1) are completed again by the next call, from that state, with the same
 *   bits.
 *   State rules, those of RRX_tracks_true_peak_window_device.  The state is read for a track only when its index e0 > 0.  Every call
 *   with win_frames > 0 and row_frames > 0 writes EVERY entry of d_state_out (when it is not NULL); a track without a processed
 *   frame (not begun, already ended, zero length) gets a copy of its d_state_in entries, or zeros when d_state_in is NULL.
 *   d_state_in NULL is allowed only with win_first == 0.  The two buffers must not overlap over ntracks * 8 doubles (RR_INVPARAM,
 *   equal pointers included).  d_state_out may be NULL.
 *   Order of calls.  Windows that partition [0, row_frames), taken in ascending contiguous order, each given the state of the one
 *   before, leave the bits of ONE RRX_tracks_limit_release_device call, for any cut positions: the samples, d_reduction and
 *   d_limited.  Anything else gives other numbers, never an access outside d_buf, d_dst, d_work or the states.  With
 *   release == 0.0 the call leaves RRX_tracks_limit_window_device's bytes and statistics, whatever the state holds and in any
 *   order (fmin(v, 0*p + v) = v for the finite p a state holds).
 * Everything in front of the release is RRX_tracks_limit_window_device's on the same sub-ranges -- detector, window minimum, the
 * same back / ahead, coverage rule and clamps --, everything behind it the box, fmin, product and statistics with q in place of m.
 *   d_work: at least RRX_tracks_limit_release_window_work_doubles(ntracks, win_frames, taps, lookahead, hold, block) doubles, which
 *   is ntracks * (2 * (win_frames + 2 * lookahead + hold + 2 * taps) + 4 * ((win_frames + lookahead - 1) / block + 2)) -- the window
 *   call's r and m and C, A, B, S of the pieces of a window, a range of E entries meeting at most E / block + 2 blocks -- or 0 for
 *   arguments the call refuses and for a total of 2^60 doubles or more (host only).  Its content after the call is unspecified.
 *   Launches: the window call's detector and window minimum, then summary (one lane per (track, piece)), carry (one wave per
 *   track) and run (the summary's lanes, q over m in place), then the window call's smoothing and product; each split over chunks
 *   of 32768 tracks.  The call only enqueues: no allocation, no host synchronisation.
 * Returns RR_INVPARAM, before any device is touched, for everything RRX_tracks_limit_window_device refuses (its work rule replaced
 * by the function above), a release that is a NaN, below 0 or not below 1, a block outside
 * RRX_LIMIT_RELEASE_MIN_BLOCK..RRX_LIMIT_RELEASE_MAX_BLOCK, and the two state rules; RR_EXTUNINIT before init_ratelib; RR_INTERNAL
 * for a failed launch.  win_frames == 0 or row_frames == 0 is RR_OK and touches nothing, the state included. */
#define RRX_LIMIT_RELEASE_WIN_STATE 8
size_t RRX_tracks_limit_release_window_work_doubles(int ntracks, size_t win_frames, int taps, size_t lookahead, size_t hold,
                                                    size_t block);
int RRX_tracks_limit_release_window_device(int device, void *hip_stream, const RRX_track *d_tracks, int ntracks, int nch,
                                           int src_format, const void *d_buf, size_t buf_stride, size_t buf_first,
                                           size_t buf_frames, size_t row_frames, size_t win_first, size_t win_frames,
                                           int dst_format, void *d_dst, size_t dst_stride, const double *d_gain, double ceiling,
                                           const double *coefs, int phases, int taps, size_t lookahead, size_t hold,
                                           double release, size_t block, const double *d_state_in, double *d_state_out,
                                           double *d_reduction, unsigned long long *d_limited, double *d_work,
                                           size_t work_doubles);
/* Test hook (host only, needs no device), refused with -1 unless RSMP_TEST_HOOKS is set as above: the call above on HOST pointers
 * and a HOST table, as serial loops over the very functions the kernels call for the cut, the pieces and every step.  Same
 * refusals, same results. */
int RRX_debug_tracks_limit_release_window_host(const RRX_track *tracks, int ntracks, int nch, int src_format, const void *buf,
                                               size_t buf_stride, size_t buf_first, size_t buf_frames, size_t row_frames,
                                               size_t win_first, size_t win_frames, int dst_format, void *dst, size_t dst_stride,
                                               const double *gain, double ceiling, const double *coefs, int phases, int taps,
                                               size_t lookahead, size_t hold, double release, size_t block,
                                               const double *state_in, double *state_out, double *reduction,
                                               unsigned long long *limited, double *work, size_t work_doubles);

/* Test hook (host only, needs no device), refused with -1 unless RSMP_TEST_HOOKS is set as above: what the two window calls take
 * from one HOST table entry for the window [win_first, win_first + win_frames) of rows of row_frames frames, computed by the very
 * functions their kernels call.  stage[10]: the window-relative half-open ranges of the backward extension, the copied track, the
 * forward extension and the zeros (two values each; adjacent, covering [0, win_frames)), the frame of the packed source that the
 * first copied frame comes from (no copied frame: the clamped src_first), and how many of the copied frames lie inside the source
 * (the rest read as zeros).  finish[4]: the window-relative range of the processed frames, the track-relative index of the first
 * and its destination frame (all zero when the slice does not meet the window); `write` zero is the d_dst NULL case.
 * RR_INVPARAM for a NULL pointer or a window outside the rows. */
int RRX_debug_tracks_window_cut(const RRX_track *entry, size_t row_frames, size_t src_total, size_t dst_total, int write,
                                size_t win_first, size_t win_frames, unsigned long long *stage, unsigned long long *finish);

/* Introspection: isamp_max of rate_base.h:531, frames currently pullable (fifo_occupancy of the last
 * fifo, rate_base.h:447-448), shape of the handle. */
size_t RRX_isamp_max(const RR_handle *h);
size_t RRX_available(const RR_handle *h);
int RRX_channels(const RR_handle *h);
int RRX_streams(const RR_handle *h);

/* Host-only (no GPU needed): JSON description of the stage chain the planner builds for `config`
 * (what rate_init decides, rate/rate_base.h:247-423).  Returns the length written (without the
 * terminator), or the negated RR_error on failure; the text is truncated to cap-1 bytes. */
int RRX_describe_plan(const RR_config *config, char *buf, size_t cap);

/* The plan cache.  Designing the filters of a config takes under a millisecond at phase 50 and 50 ms to 0.6 s at other phase
 * settings, and the plan is a pure function of the six RR_config fields.  Every call of this library that needs a plan -- the open calls and the
 * host-only calls RRX_describe_plan, RRX_describe_dispatch, RRX_plan_table, RRX_track_geometry, RRX_tracks_plan,
 * RRX_tracks_batches -- takes it from a process-wide cache keyed by those fields (the doubles by bit pattern): at most 16 plans,
 * the least recently used evicted, guarded by a mutex so that threads may open concurrently (chain.h:36).  A cached plan is the
 * same bits as a designed one; configs the planner refuses are not kept.  Only the host-side design is shared: every handle
 * still uploads its own device tables.
 * RRX_plan_cache_clear drops every plan and zeroes the counters.  RRX_plan_cache_stats reports lookups served from the cache,
 * lookups that had to design (refused configs included), and the plans held now; any pointer may be NULL; it returns RR_OK.
 * Both are host-only. */
void RRX_plan_cache_clear(void);
int RRX_plan_cache_stats(unsigned long long *hits, unsigned long long *misses, int *entries);

/* Host-only (no GPU needed): which kernel form the first stage pair of `config` gets on handles of `nchannels` channels per
 * stream, as JSON: {"sub_blocked": false} or {"sub_blocked": true, "two_round": .., "nsub": .., "Vs": .., "V": .., "taps": ..,
 * "N": .., "Pref": .., "sub_blocks": [{"off", "len", "win", "shift"} ...]} -- the geometry of the sub-blocked fused kernels
 * (DESIGN.md 4), decided from the plan alone.  Nothing in the reference corresponds to it (its blocks are one transform
 * each, rate/dft_filter.h:60-190); it exists so that the decision can be tested without a device.  Returns as
 * RRX_describe_plan does. */
int RRX_describe_dispatch(const RR_config *config, int nchannels, char *buf, size_t cap);

/* Host-only: copy a designed table for `config` into out[0..cap): which = 0 / 1 -> taps of the first /
 * second DFT-stage filter (after phase conversion, before the 2L/N scaling of rate_base.h:175),
 * which = 2 -> polyphase table [phase][tap][order+1] (rate/prepare_coefs.h:20-46).  *count receives
 * the full length.  Returns RR_OK or RR_INVPARAM. */
int RRX_plan_table(const RR_config *config, int which, double *out, size_t cap, size_t *count);

/* Channel mixing ("Channel mixing"): a matrix applied per frame -- on load in the stage pass of a ragged batch, so
 * that a 5.1 library is read once, as stored, and only two channels are ever resampled, and on plain rows behind a handle (mono to
 * stereo, mid/side, swap, polarity).
 *
 * The mixing rule is part of this ABI.  `mix` is a HOST pointer to nch_dst * nch_src finite doubles, row-major: mix[o * nch_src + c]
 * is the coefficient of source channel c in output channel o, 1 <= nch_src, nch_dst <= RRX_MIX_MAX_CH.  The calls copy the matrix
 * into their launch arguments (as RRX_true_peak_device copies coefs): it may be freed on return.  For one frame and output channel o
 *   v_c = the source sample of channel c as an exact double: s * 2^-15 (S16), s * 2^-23 (S24_3), s * 2^-31 (S32), (double)x for
 *         float32, x for float64
 *   y_o = sum over c ascending of mix[o][c] * v_c, every product and every sum rounded on its own (fp64, no fused multiply-add),
 *         WHERE TERMS WITH mix[o][c] == 0.0 (either sign) ARE LEFT OUT; the sum starts from its first product, not from 0.0; a row
 *         of zeros gives +0.0
 *   x_o = (float)y_o for float32 rows (one rounding, to nearest even), y_o for float64 rows
 * A zero coefficient means "not connected", not a multiplication by zero: a NaN or an infinity in an unconnected channel (a dropped
 * LFE) does not reach the output; -0.0 passes through an identity or permutation matrix unchanged; and with the identity matrix
 * the integer sources give the bits of RRX_tracks_stage_device_samples's conversion, hence its rows.
 * S32 is exact in the double, so a mixed S32 source is rounded ONCE, from the exact sum.  That is deliberately not the result of
 * converting to float32 first (the un-mixed stage's conversion) and mixing afterwards.
 *
 * RRX_mix_device: source rows [nstreams][src_stride][nch_src] and destination rows [nstreams][dst_stride][nch_dst], both of `fmt`,
 * RRX_FMT_FLOAT or RRX_FMT_DOUBLE; frames [0, frames) of every stream are mixed by the rule above, and nothing outside [0, frames)
 * of a destination row is written.  Strides (in frames, ignored for nstreams == 1), the alignment of one sample, device, hip_stream,
 * stream ordering and "only enqueues" are RRX_finish_device's.  The buffers must not overlap.  Returns RR_INVPARAM, before any
 * device is touched, for mix NULL, a coefficient that is not finite, a channel count outside 1..RRX_MIX_MAX_CH, a format other than
 * those two, a NULL buffer, d_dst == d_src or any other overlap, nstreams < 1, a stride below frames, sizes of 2^60 samples or more,
 * or device < -1; RR_EXTUNINIT, RR_INTERNAL as RRX_finish_device.  frames == 0 is RR_OK and touches nothing. */
#define RRX_MIX_MAX_CH 16
int RRX_mix_device(int device, void *hip_stream, int fmt, const void *d_src, size_t src_stride, int nstreams, size_t frames,
                   int nch_src, void *d_dst, size_t dst_stride, int nch_dst, const double *mix);

/* RRX_tracks_stage_device_samples with the mix on load.  The packed source is [src_total][nch_src] of src_format (RRX_FMT_FLOAT,
 * RRX_FMT_S16, RRX_FMT_S24_3 -- nch_src * 3 bytes a frame, so a track starts at any byte offset -- or RRX_FMT_S32; RRX_FMT_DOUBLE is
 * refused as there), the rows are [ntracks][row_frames][nch] float32, and mix is [nch][nch_src].  The rows equal, bit for bit, those
 * of RRX_tracks_stage_device on the float32 packed buffer [src_total][nch] whose frames are the mixed frames x_o of the source.  So
 * the copied frames are mixed, both LPC extensions run on the mixed base frames (the rule is applied as they are loaded, by the
 * same function), zeros stand behind the extension, and frames that a wrong table puts past the source are +0.0f.  RRX_track is in
 * frames and does not change: a table of RRX_tracks_plan serves any channel pair.
 * The read contract (only aligned dwords that hold a byte of the source are read), the clamps (a wrong table gives wrong samples,
 * never an access outside source or rows), "every frame of every row is written exactly once", device, hip_stream, stream ordering,
 * "only enqueues", refusals and return values are RRX_tracks_stage_device_samples's, word for word, with nch_src in the source
 * sizes and nch in the row sizes; and RR_INVPARAM, before any device is touched, also for mix NULL, a coefficient that is not
 * finite, or nch or nch_src outside 1..RRX_MIX_MAX_CH.
 * RRX_tracks_stage_mix_window_device has the bits of the whole-row call for frames [win_first, win_first + win_frames), as
 * RRX_tracks_stage_window_device has of its whole-row call, with that call's window rules and refusals. */
int RRX_tracks_stage_mix_device(int device, void *hip_stream, size_t in_rate, size_t out_rate, const RRX_track *d_tracks, int ntracks,
                                int src_format, int nch_src, const void *d_packed, size_t src_total, int nch, const double *mix,
                                fb_sample_t *d_rows, size_t row_frames);
int RRX_tracks_stage_mix_window_device(int device, void *hip_stream, size_t in_rate, size_t out_rate, const RRX_track *d_tracks,
                                       int ntracks, int src_format, int nch_src, const void *d_packed, size_t src_total, int nch,
                                       const double *mix, size_t row_frames, size_t win_first, size_t win_frames, fb_sample_t *d_win,
                                       size_t win_stride);
/* Test hooks (host only, need no device), refused with -1 unless RSMP_TEST_HOOKS is set as above: serial loops over the very
 * per-frame function the kernels call.  RRX_debug_mix_host is RRX_mix_device on HOST pointers, with its refusals.
 * RRX_debug_tracks_mix_host writes out[count][nch], the mixed float32 frames [first_frame, first_frame + count) of a HOST source
 * [..][nch_src] of src_format; RR_INVPARAM for an unknown format, a NULL pointer, a channel count outside 1..RRX_MIX_MAX_CH or a
 * coefficient that is not finite. */
int RRX_debug_mix_host(int fmt, const void *src, size_t src_stride, int nstreams, size_t frames, int nch_src, void *dst,
                       size_t dst_stride, int nch_dst, const double *mix);
int RRX_debug_tracks_mix_host(int src_format, const void *src, int nch_src, size_t first_frame, size_t count, int nch,
                              const double *mix, float *out);

#ifdef __cplusplus
}
#endif

#endif
