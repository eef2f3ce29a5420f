// Gapless albums ("Gapless albums"): the stage pass of a ragged batch whose tracks may be cut from one master.  At a
// join the frames in front of track k + 1 exist, as the end of track k, and they lie directly in front of it in the packed source;
// so a linked edge of a row is a copy of the neighbour's frames where tracks.hip extrapolates.  A row with both edges linked is ONE
// contiguous run of the packed source with zeros around it.  Implemented in tracks_album.hip; tracks.hip is not touched.
#pragma once
#include "tracks.hpp"

namespace rsmp {

// RRX_track_link of include/ratelib_amd_album.h, field for field; in frames
struct TrackLink {
  unsigned long long back, ahead;
};
constexpr unsigned long long kLinkNone = ~0ull; // RRX_LINK_NONE: this edge is extrapolated, as tracks.hip does it

// One workgroup of the copy kernel looks at this many samples of a row: 256 lanes x 4 samples x 8 steps (32 KiB written).  The
// tests take their lengths around the seams from this line.
constexpr int kAlbumThreads = 256;
constexpr int kAlbumSteps = 8;
constexpr int kAlbumTileSamples = kAlbumThreads * 4 * kAlbumSteps;

// ------------------------------------------------------------------------------------------------------ interval arithmetic
// The stage pass of one track with its links inside a window (the whole row is the window [0, row_frames)): the regions of the row,
// each cut to the window, as half-open ranges of WINDOW frames.  They are adjacent, in this order, and cover [0, w.frames):
//   zb   zeros in front of a linked backward edge whose album begins inside the extension (empty for an extrapolated edge)
//   bk   the backward LPC extension (empty for a linked edge)
//   cp   the copy: the neighbour's last `back_frames` frames, the track, the neighbour's first `ahead_frames` frames
//   fw   the forward LPC extension (empty for a linked edge)
//   z    zeros: what a linked forward edge lacks of its extension, and the track's drain
// The kernels and RRX_debug_tracks_stage_album_host both call this function, and everything they take from an entry and its link
// goes through it: tracks_entry's clamps first, then the links clamped to the extension and to the source.  So a wrong table or
// link gives wrong samples, never a read outside [0, src_total) or a write outside the track's own row.
struct TracksAlbumCut {
  TracksEntry e;
  unsigned long long back_frames, ahead_frames; // frames of the neighbours that the row holds (0 for an extrapolated edge)
  bool lpc_back, lpc_ahead;                     // the edge is extrapolated
  unsigned long long zb[2], bk[2], cp[2], fw[2], z[2];
  unsigned long long src_frame; // frame of the packed source that window frame cp[0] is a copy of (cp empty: the run's first)
  unsigned long long readable;  // of the frames [cp[0], cp[1]), the first `readable` lie inside the source; the rest read as zeros
};

__host__ __device__ __forceinline__ unsigned long long tracks_album_min(unsigned long long x, unsigned long long y) { return x < y ? x : y; }

__host__ __device__ __forceinline__ TracksAlbumCut tracks_album_cut(const Track &tr, const TrackLink &ln, unsigned long long row_frames,
                                                                    unsigned long long src_total, const TracksWindow &w)
{
  TracksAlbumCut c;
  c.e = tracks_entry(tr, row_frames, src_total);
  c.lpc_back = ln.back == kLinkNone;
  c.lpc_ahead = ln.ahead == kLinkNone;
  // the neighbour's frames in front: no more than the extension, than the album has, than the source has
  c.back_frames = c.lpc_back ? 0 : tracks_album_min(tracks_album_min(c.e.lead, ln.back), c.e.first);
  // and behind: only where the track itself is whole (first + frames <= src_total), so that the run stays contiguous
  const unsigned long long end = c.e.first + c.e.have; // <= src_total
  c.ahead_frames = c.lpc_ahead || c.e.have < c.e.frames ? 0 : tracks_album_min(tracks_album_min(c.e.fwd, ln.ahead), src_total - end);
  const unsigned long long t0 = c.e.lead, t1 = t0 + c.e.frames, x1 = t1 + c.e.fwd; // the track and the end of its extension, <= row_frames
  const unsigned long long c0 = t0 - c.back_frames, c1 = t1 + c.ahead_frames;
  const unsigned long long b0 = c.lpc_back ? 0 : c0;  // [0, b0) zeros, [b0, c0) backward LPC
  const unsigned long long z0 = c.lpc_ahead ? x1 : c1; // [c1, z0) forward LPC, [z0, row_frames) zeros
  tracks_window_range(w, 0, b0, c.zb);
  tracks_window_range(w, b0, c0, c.bk);
  tracks_window_range(w, c0, c1, c.cp);
  tracks_window_range(w, c1, z0, c.fw);
  tracks_window_range(w, z0, row_frames, c.z);
  const unsigned long long n = c.cp[1] - c.cp[0], off = n ? w.first + c.cp[0] - c0 : 0; // frame of the run that comes first
  const unsigned long long run = c.back_frames + c.e.have + c.ahead_frames;             // frames of the run inside the source
  c.src_frame = c.e.first - c.back_frames + off;
  c.readable = run > off ? (run - off < n ? run - off : n) : 0;
  return c;
}

// what RRX_tracks_stage_album_device was given, after validation: the stage arguments, and the links on the device
struct TracksAlbumArgs {
  TracksStageArgs s;
  const TrackLink *links; // [ntracks]
};

// Only enqueues on `stream`: the copy kernel (split past grid.y's 16-bit count) and the LPC kernel, whose workgroups of a linked edge
// return at once.  a.s.rows is the window's buffer [ntracks][w.stride][nch]; the whole rows are the window [0, row_frames) with
// w.stride == row_frames.  w.frames > 0.  Reads of an integer source as in launch_tracks_stage (tracks.hpp): aligned dwords that
// hold a byte of the frames the run may read, and nothing further out.
hipError_t launch_tracks_stage_album(hipStream_t stream, const TracksAlbumArgs &a, const TracksWindow &w);

// the host twin: the copy and the zeros of every row, by the same cut; the frames of an extrapolated edge are left as they are
void tracks_stage_album_host(const TracksAlbumArgs &a, const TracksWindow &w);

} // namespace rsmp
