// Run-time and build-time switches of the library, in ONE place.
//
// Run-time knobs (environment, read ONCE per process by knobs(); nothing on the launch path calls getenv).  Every one of
// them only selects between kernel variants that produce the same samples to the parity bar, or sizes a buffer:
//   RSMP_NO_FUSE / RSMP_NO_MFMA / RSMP_NO_POLYMF / RSMP_NO_FAST / RSMP_NO_SPLIT / RSMP_NO_SPLIT2 / RSMP_NO_DFTX / RSMP_NO_POLYI /
//   RSMP_NO_POLYCOOP /
//   RSMP_SPREAD_VECTOR    keep a chain off the named fast variant (the generic variant of the same stage runs instead)
//   RSMP_NO_SIDE          seam kernels on the main stream instead of the side stream
//   RSMP_SLAB_MB=n        fp64 fifo budget of a time slab (default 1536)
//   RSMP_SEAM_RING_MB=n   budget of a fused chain's seam ring (default 1280): bounds the blocks per launch (tests force many launches per push)
//   RSMP_STAMPS=1         per-phase cycle sums of the fused kernels (s_memtime), printed when the handle closes
//   RSMP_LDS_PAD=n / RSMP_OCC=1   occupancy experiments of fused_kernel (more LDS per workgroup / print blocks per CU)
//   RSMP_TEST_HOOKS       arms the RRX_debug_* entry points (allocation failures, host models of the tile walk and the output stage)
//   RATELIB_AMD_DEVICES=all | i,j,...   RR_open / RRX_open_batch deal new handles round-robin over these devices
//                         (unset: a handle lives on the calling thread's current device)
//
// Build-time switch:
//   -DRSMP_STAMPS_BUILD   (tools/build_variant.sh) compiles the per-phase stamp points into the lean fused kernels
//                         (fused_fast.hip), which RSMP_STAMPS=1 then reads; correct results, how DESIGN.md 5a is re-measured
#pragma once
#include <cstddef>

namespace rsmp {

struct Knobs {
  bool no_fuse = false, no_mfma = false, no_polymf = false, no_fast = false, no_split = false, no_split2 = false, no_dftx = false, no_polyi = false,
       no_polycoop = false, spread_vector = false, no_side = false, stamps = false, occ = false, test_hooks = false;
  double slab_mb = 1536.0, seam_ring_mb = 1280.0;
  size_t lds_pad = 0;
};
// the process's knobs: the environment is read at the first call (thread-safe), never again
const Knobs &knobs();

} // namespace rsmp
