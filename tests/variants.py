"""The table of run-time knob settings (csrc/knobs.hpp) whose fallback kernels the suite holds to the parity bars.

A row: (id, environment of the child process, cases, must launch, must not launch).
  cases        rows in the shape of chain_ld.CASES: (id, in_rate, out_rate, options, frames, channels, streams, call pattern).
               Frame counts as in chain_ld.CASES: three blocks of the chain's longest DFT stage (12 000 for 4096-point blocks,
               24 000 for 8192, 48 000 for 16384).  Rows that chain_ld.CASES already has (same rates, options, frames and
               channels) are repeated as they are, so chain_ld.reference's cache serves both test files.
  must launch  kernel names, written out in full as RRX_profile_report prints them.  A plain string must be among the names of
               at least one case of the row; a (case id, name) pair must be among the names of that case; a (case id, name of
               the float32 handle, name of the float64 handle) triple where the two formats have kernels of their own.
  must not     fragments that no kernel name of any case of the row may contain.
tests/test_variants_table.py checks on the CPU that every case's plan has the property its row relies on and that every
variant-selecting knob has a row; tests/test_gpu_variants.py runs the rows, one child process per row (the knobs are read once
per process, and a variable that is merely set counts as on).

Two scheduling switches (RSMP_NO_SIDE, RSMP_SLAB_MB) move launches, not kernels: SCHEDULING names their environments, the
call patterns are in tests/variant_child.py.

spread_vector: 48k -> 44.1k plans as x2 dft -> 147/320, so its step is 320 like 96k -> 44.1k's, with 2048-point input spectra;
it is the one chain that reaches the padded-window vector instance at P = 2^11.  The step-160 chain is 48k -> 88.2k (x2 dft ->
147/160).
"""
from chain_ld import BW99, NORM

# seconds a child may take.  Measured on an MI355X over three runs: 2.1 .. 3.1 s per child of VARIANTS, 0.5 .. 4.1 s per child of
# SCHEDULING, and 13.0 s once for a child that imported torch behind the library's first handle (variant_child.py now imports it
# first); 10 x that slowest one
CHILD_TIMEOUT = 130

VARIANTS = [
    ("no_fast", {"RSMP_NO_FAST": "1"},
     [("44k1_96k_lean", 44100, 96000, {}, 12000, 2, 1, "flow"),
      ("96k_44k1_4ch", 96000, 44100, {}, 12000, 4, 1, "flow"),
      ("44k1_48k_bw99_flow", 44100, 48000, BW99, 48000, 2, 1, "flow")],
     [("44k1_96k_lean", "rsmp::fused_kernel<12, 11, 2, 7, true>"), ("96k_44k1_4ch", "rsmp::fused_kernel<12, 12, 2, 8, true>"),
      ("44k1_96k_lean", "rsmp::seam_kernel"), ("96k_44k1_4ch", "rsmp::seam_kernel"),
      ("44k1_48k_bw99_flow", "rsmp::dft_kernel<14, 13, 14, false>"), ("44k1_48k_bw99_flow", "rsmp::polymf_kernel<9>")],
     ["fused_fast", "fused_split"]),
    ("no_mfma", {"RSMP_NO_MFMA": "1"},
     [("44k1_96k_lean", 44100, 96000, {}, 12000, 2, 1, "flow"),
      ("96k_44k1_2ch_push", 96000, 44100, {}, 12000, 2, 1, "push"),
      ("44k1_48k_bw99_push", 44100, 48000, BW99, 48000, 2, 1, "push")],
     [("44k1_96k_lean", "rsmp::fused_kernel<12, 11, 2, 25, false>"), ("96k_44k1_2ch_push", "rsmp::fused_kernel<12, 12, 2, 27, false>"),
      ("44k1_48k_bw99_push", "rsmp::poly_kernel<0>"), ("44k1_48k_bw99_push", "rsmp::dft_kernel<14, 13, 14, false>")],
     ["true>", "polymf", "fused_fast", "fused_split"]),
    ("no_fuse", {"RSMP_NO_FUSE": "1"},
     [("44k1_96k_lean", 44100, 96000, {}, 12000, 2, 1, "flow"),
      ("44k1_96k_generic", 44100, 96000, {}, 12000, 3, 1, "push"),
      ("96k_44k1", 96000, 44100, {}, 12000, 3, 1, "flow")],
     [("44k1_96k_lean", "rsmp::dft_kernel<12, 11, 12, false>"), ("44k1_96k_generic", "rsmp::dft_kernel<12, 11, 12, false>"),
      ("96k_44k1", "rsmp::dft_kernel<12, 12, 12, false>"),
      ("44k1_96k_lean", "rsmp::polymf_kernel<7>"), ("44k1_96k_generic", "rsmp::polymf_kernel<7>"), ("96k_44k1", "rsmp::polymf_kernel<8>")],
     ["fused_kernel", "fused_fast", "fused_split"]),  # (fused_prep_kernel is legitimate under polymf_kernel)
    ("no_fuse_no_polymf", {"RSMP_NO_FUSE": "1", "RSMP_NO_POLYMF": "1"},
     [("44k1_96k_generic", 44100, 96000, {}, 12000, 3, 1, "push"),       # L 160, n 24: table 30 720 B, in LDS
      ("8k_11k025", 8000, 11025, {}, 12000, 3, 1, "push"),              # L 441, n 24: table 84 672 B, read from memory
      ("96k_44k1_2ch", 96000, 44100, {}, 12000, 2, 1, "flow")],
     [("44k1_96k_generic", "rsmp::poly_kernel<0>"), ("8k_11k025", "rsmp::poly_kernel<0>"), ("96k_44k1_2ch", "rsmp::poly_kernel<0>"),
      ("44k1_96k_generic", "rsmp::dft_kernel<12, 11, 12, false>"), ("8k_11k025", "rsmp::dft_kernel<12, 11, 12, false>"),
      ("96k_44k1_2ch", "rsmp::dft_kernel<12, 12, 12, false>")],
     ["fused_kernel", "fused_fast", "fused_split", "polymf"]),
    ("no_polyi", {"RSMP_NO_POLYI": "1"},
     [("44k1_48001", 44100, 48001, {}, 12000, 3, 1, "flow"),            # order 3, n 24: eight lanes per output
      ("96k_44101_norm", 96000, 44101, NORM, 12000, 3, 1, "flow"),      # order 2, n 16: eight lanes per output
      ("44k1_11027_norm", 44100, 11027, NORM, 24000, 3, 1, "flow"),     # order 1, n 12: n % 8 != 0, generic
      ("16k_11026", 16000, 11026, {}, 24000, 3, 1, "flow"),             # order 2, n 20: generic
      ("11k025_8007", 11025, 8007, {}, 12000, 3, 1, "flow")],           # order 3, n 20: generic
     [("44k1_48001", "rsmp::poly_coop_kernel<3>"), ("96k_44101_norm", "rsmp::poly_coop_kernel<2>"),
      ("44k1_11027_norm", "rsmp::poly_kernel<1>"), ("16k_11026", "rsmp::poly_kernel<2>"), ("11k025_8007", "rsmp::poly_kernel<3>")],
     ["polyi_kernel"]),
    ("no_polyi_no_polycoop", {"RSMP_NO_POLYI": "1", "RSMP_NO_POLYCOOP": "1"},
     [("44k1_48001", 44100, 48001, {}, 12000, 3, 1, "flow"),
      ("96k_44101_norm", 96000, 44101, NORM, 12000, 3, 1, "flow"),
      ("8k_8001_bw99", 8000, 8001, BW99, 48000, 3, 1, "flow")],         # order 3, n 28, behind 16384-point blocks
     [("44k1_48001", "rsmp::poly_kernel<3>"), ("96k_44101_norm", "rsmp::poly_kernel<2>"), ("8k_8001_bw99", "rsmp::poly_kernel<3>")],
     ["polyi_kernel", "poly_coop"]),
    ("no_dftx", {"RSMP_NO_DFTX": "1"},
     [("48k_192k", 48000, 192000, {}, 24000, 3, 1, "flow"),
      ("44k1_192k_bw99_sub", 44100, 192000, BW99, 48000, 2, 1, "flow")],
     [("48k_192k", "rsmp::dft_kernel<13, 11, 13, false>"), ("44k1_192k_bw99_sub", "rsmp::dft_kernel<13, 11, 13, false>")],
     ["dftx_kernel"]),
    ("spread_vector", {"RSMP_SPREAD_VECTOR": "1"},
     [("96k_44k1_2ch", 96000, 44100, {}, 12000, 2, 1, "flow"),          # step 320, P = 2^12
      ("48k_44k1", 48000, 44100, {}, 12000, 2, 1, "flow"),              # step 320, P = 2^11
      ("48k_88k2", 48000, 88200, {}, 12000, 2, 1, "flow"),              # step 160
      ("44k1_96k_lean", 44100, 96000, {}, 12000, 2, 1, "flow")],        # step 147: stays on the lean kernel
     [("96k_44k1_2ch", "rsmp::fused_kernel<12, 12, 2, 27, false>"), ("48k_44k1", "rsmp::fused_kernel<12, 11, 2, 32, false>"),
      ("48k_88k2", "rsmp::fused_kernel<12, 11, 2, 26, false>"), ("44k1_96k_lean", "rsmp::fused_fast_kernel<11, 7, false>", "rsmp::fused_fast_dio_kernel<11, 7, false>")],
     []),
]
VARIANT_IDS = [v[0] for v in VARIANTS]

# the knobs that move launches: (environment of the run under test, environment of the comparison run)
SCHEDULING = {
    "side_stream": ({"RSMP_SEAM_RING_MB": "0.01"}, {"RSMP_SEAM_RING_MB": "0.01", "RSMP_NO_SIDE": "1"}),
    "slabs": ({"RSMP_SLAB_MB": "0.001"}, {}),
}

# what a knob of knobs.hpp's list needs no row for (tests/test_variants_table.py): instrumentation, the test switch, and the
# two sub-block switches that tests/test_gpu_split.py and the sub-blocked cases above cover
NOT_VARIANTS = ("RSMP_STAMPS", "RSMP_OCC", "RSMP_LDS_PAD", "RSMP_TEST_HOOKS", "RSMP_NO_SPLIT", "RSMP_NO_SPLIT2")


def child_env(environ, extra):
    """The environment of a child: the caller's without any RSMP_* name except RSMP_TEST_HOOKS and without
    RATELIB_AMD_DEVICES, plus the row's variables -- a knob exported around the suite does not change what is tested."""
    env = {k: v for k, v in environ.items() if not (k.startswith("RSMP_") and k != "RSMP_TEST_HOOKS") and k != "RATELIB_AMD_DEVICES"}
    env.update(extra)
    return env
