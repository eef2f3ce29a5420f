/* Gapless albums: ragged track batches (ratelib_amd.h, RRX_track) whose tracks may be cut from ONE master -- live records,
 * classical movements, DJ mixes.  RRX_tracks_plan treats every track as an island: both ends are extended by LPC extrapolation and
 * its output grid starts at its own first frame, which is the plugin's treatment of a track change after a flush.  At a join of a
 * gapless album that invents a context that exists (the 50 ms in front of track k + 1 are the end of track k) and moves the output
 * grid by up to one output sample of time.  The calls below plan and stage such tracks from their neighbours, on the album's grid:
 * a track's row, resampled on a fresh handle and cut by its table entry, gives the samples the album resampled as one stream has
 * there, with exactly its frame counts.  Nothing else changes: RRX_track keeps its fields, and RRX_tracks_finish_device, the
 * meters and the limiter take these tables as they are.
 *
 * The header is an extension of ratelib_amd.h and includes it; the functions live in the same library. */
#ifndef RATELIB_AMD_ALBUM_H
#define RATELIB_AMD_ALBUM_H

#include "ratelib_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per track, what lies beside it in the packed source: `back` = frames of the SAME album directly in front of src_first, `ahead` =
 * frames of it directly behind src_first + frames.  RRX_LINK_NONE: the edge is an album's edge or a single's -- extrapolate. */
#define RRX_LINK_NONE (~0ULL)
typedef struct RRX_track_link {
  unsigned long long back;
  unsigned long long ahead;
} RRX_track_link;

/* Host-only (no GPU needed): RRX_tracks_plan for tracks that lie in the packed source in the order given, with group[t] < 0 for a
 * single and consecutive tracks of one non-negative group[t] forming an album in play order.  A single gets RRX_tracks_plan's
 * entry, field for field, and links of RRX_LINK_NONE; so does every track of an album of at most 64 frames in all.
 * For an album of A frames, with g = gcd(in_rate, out_rate), r1 = in_rate / g, r2 = out_rate / g, n_add and n_drop of
 * RRX_edge_geometry, S_k the first frame of track k counted from the album's first, and ph_k = S_k mod r1:
 *   lead_k       = n_add + ph_k                         row k starts at album frame S_k - lead_k, a multiple of r1
 *   out_first_k  = n_drop + ceil(ph_k * r2 / r1)
 *   out_frames_k = ceil(S_{k+1} * r2 / r1) - ceil(S_k * r2 / r1)                      k not the last
 *   out_frames_k = out_frames of RRX_track_geometry(A) - ceil(S_k * r2 / r1)          k the last (0 if that is negative)
 * so the out_frames of an album add up to the out_frames of the album as one track.  src_first and dst_first run on over all
 * tracks as in RRX_tracks_plan.  links[k] = { S_k, A - S_k - frames_k }, with RRX_LINK_NONE for `back` of the first track and `ahead`
 * of the last.  *row_frames = the largest frames + 2 * lead; the other three outputs as in RRX_tracks_plan.
 * The planner confirms with the handle's counter arithmetic that every album row yields out_first_k + out_frames_k frames and
 * returns RR_INTERNAL if one does not.
 * An entry is self-contained (src_first and dst_first are absolute), so any subset of the entries, in any order, with the same
 * subset of the links, is a valid batch table for the packed source and destination of the whole plan; its row_frames is the
 * subset's largest frames + 2 * lead.
 * Returns RR_INVPARAM for what RRX_tracks_plan refuses, a NULL group or links, and a group id that appears again after another
 * id (albums are consecutive). */
int RRX_tracks_plan_album(const RR_config *config, const size_t *frames, const int *group, int ntracks, RRX_track *table,
                          RRX_track_link *links, size_t *row_frames, size_t *out_row_cap, size_t *src_total, size_t *dst_total);

/* RRX_tracks_stage_device_samples with links.  d_links is DEVICE memory, [ntracks], beside d_tracks.  Per edge of track t, after
 * the clamps of that call (lead, frames and the extension cut to row_frames, src_first to src_total):
 *   link RRX_LINK_NONE   exactly what RRX_tracks_stage_device_samples writes there: the LPC extension (zeros from a track of at
 *                        most 32 frames), bit for bit;
 *   backward link        row frame i < lead is frame src_first - lead + i of the packed source where lead - i <= min(back,
 *                        src_first), and +0.0f in front of that (the album began inside the extension);
 *   forward link         row frame lead + frames + i, i < lead, is frame src_first + frames + i of the source where i < min(ahead,
 *                        src_total - src_first - frames), and +0.0f behind that; a track that the table puts across the end of
 *                        the source has no frames behind it.
 * Copied frames are converted by RRX_tracks_stage_device_samples' rule.  Zeros behind the forward extension, every frame of every
 * row written exactly once, nothing outside the rows written, d_packed only read, the read contract for integer sources (aligned
 * dwords that hold a byte of the source's frames, nothing further out), the unvalidated device table -- a wrong table or link
 * gives wrong samples, never an access outside the source or the track's own row --, device, hip_stream, stream ordering, "only
 * enqueues", every refusal and return value: RRX_tracks_stage_device_samples', word for word.
 * d_links == NULL is RRX_tracks_stage_device_samples itself: the same code path, bit for bit. */
int RRX_tracks_stage_album_device(int device, void *hip_stream, size_t in_rate, size_t out_rate, const RRX_track *d_tracks,
                                  const RRX_track_link *d_links, int ntracks, int nch, int src_format, const void *d_packed,
                                  size_t src_total, fb_sample_t *d_rows, size_t row_frames);

/* RRX_tracks_stage_album_device on a window of the rows, as RRX_tracks_stage_window_device is of RRX_tracks_stage_device_samples:
 * frames [win_first, win_first + win_frames) of every row, bit for bit, into d_win [ntracks][win_stride][nch]; the window
 * arguments, their refusals and the empty window (RR_OK, nothing touched) are that call's.  d_links == NULL is that call. */
int RRX_tracks_stage_album_window_device(int device, void *hip_stream, size_t in_rate, size_t out_rate, const RRX_track *d_tracks,
                                         const RRX_track_link *d_links, int ntracks, int nch, int src_format, const void *d_packed,
                                         size_t src_total, size_t row_frames, size_t win_first, size_t win_frames,
                                         fb_sample_t *d_win, size_t win_stride);

/* Test hook (host only, needs no device), refused with -1 unless RSMP_TEST_HOOKS is set as for the other hooks: the window form
 * above on HOST memory, as serial loops over the interval function the kernels call (whole rows: win_first = 0, win_frames =
 * win_stride = row_frames).  It writes the copied frames and the zeros; the frames of an extrapolated edge (link RRX_LINK_NONE, or
 * links == NULL: every edge) are left as they are.  The refusals are the device call's, without the device. */
int RRX_debug_tracks_stage_album_host(size_t in_rate, size_t out_rate, const RRX_track *tracks, const RRX_track_link *links,
                                      int ntracks, int nch, int src_format, const void *packed, size_t src_total,
                                      size_t row_frames, size_t win_first, size_t win_frames, fb_sample_t *win, size_t win_stride);

#ifdef __cplusplus
}
#endif

#endif
