"""Batch handles against one-stream handles, bit for bit, at the indexing seams of the resampling chain's own kernels (fused*.hip,
kernels.hip, polymf.hip, dftx.hip, dftbig.hip), at batch sizes that are not round:

  A  the workgroups of a frame of 4, 6 or 8 channels, dealt over the XCDs in groups, with more than one stream (item_map /
     item_grid and the stream term of pair_span)
  B  seam_kernel's groups of 64 channels with a partial group behind full ones
  C  polyi_kernel walking several groups of 16 channels in one workgroup
  D  launch_dft_big's rounds over its workspaces, with a round boundary inside a block
  E  launches whose grid.y is the channel or stream count, past 65 535

Inputs, caller and reference are tests/batch_cases.py's: stream s gets base signal s % 7, every stream is compared with the
one-stream handle's output for its signal, signal 0 with the oracle.  Every case asserts from the plan and from profile_report()
that its shape still reaches the seam it is about: a shape that stops reaching it fails."""
import pytest

import foo_dsp_resampler_amd as F
import batch_cases as B

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FLOAT, DOUBLE, S16 = F.RRX_FMT_FLOAT, F.RRX_FMT_DOUBLE, F.RRX_FMT_S16
BW99 = {"bandwidth": 99.0}


def ran(run, prefix, call=None):
    return any(k.startswith(prefix) for k in run.kernels(call))


def batch_against_reference(fi, fo, nch, S, fmt, kw, pushes, path="device"):
    """the batch run, every stream compared; returns the run for the caller's own assertions"""
    ref_bits, ref_counts = B.reference(fi, fo, nch, fmt, B.frozen(kw), tuple(pushes), path)
    base = B.base_signals(sum(pushes), nch, fmt)
    run = (B.run_device if path == "device" else B.run_host)(fi, fo, nch, S, fmt, kw, base, B.dealt(S), list(pushes))
    B.assert_streams_equal_reference(run, B.dealt(S), ref_bits, ref_counts)
    return run


# ------------------------------------------------------------------------------------------------ A: frame groups across streams

# (fi, fo, kw, kernel-name prefixes that must all have run)
CHAINS_A = {
    "up": (44100, 96000, {}, ["rsmp::fused_fast"]),                              # dft x2 + 160/147: the lean fused kernel
    "down": (96000, 44100, {}, ["rsmp::fused_fast"]),                            # dft + 147/320: lean too; generic through the host row
    "dftx": (44100, 176400, {}, ["rsmp::dftx_kernel<"]),                         # x4 as four component transforms
    "three-stage": (44100, 192000, BW99, ["rsmp::fused_split", "rsmp::dftx_kernel<"]),   # sub-blocked 16384-point stage -> x4
}
PUSHES_A = (9000, 14000)
CASES_A = [(c, nch, S, FLOAT, "device") for c in CHAINS_A for nch in (4, 6, 8) for S in (3, 5, 11)]
CASES_A += [(c, 8, S, fmt, "device") for c in CHAINS_A for fmt in (DOUBLE, S16) for S in (3, 5, 11)]   # pair words of 16 and 4 bytes
CASES_A += [("down", 6, 5, FLOAT, "host")]                              # through push / pull_all: the ring side of the views


@pytest.mark.parametrize("chain,nch,S,fmt,path", CASES_A, ids=lambda v: str(v))
def test_frame_groups_across_streams(chain, nch, S, fmt, path):
    """hp = nch / 2 >= 2 pair-workgroups share every frame and are placed together (fifo_device.hpp, item_map): with S > 1 the
    stream term of `pair` and of pair_span's addresses is not zero, and blocks * S is no multiple of 8, so the grid's padding is
    cut too."""
    fi, fo, kw, families = CHAINS_A[chain]
    plan = F.describe_plan(fi, fo, **kw)
    blocks = B.first_stage_blocks(plan, PUSHES_A)
    assert nch % 2 == 0 and nch >= 4 and S > 1
    assert any(nb and (nb * S) % 8 for nb in blocks), (blocks, S)               # some launch's groups do not fill the last 8
    run = batch_against_reference(fi, fo, nch, S, fmt, kw, PUSHES_A, path)
    for fam in (["rsmp::fused_kernel<"] if path == "host" else families):
        assert ran(run, fam), (fam, run.kernels())


# ------------------------------------------------------------------------------------------------------------ B: seam groups

PUSHES_B = (12000, 11000)


@pytest.mark.parametrize("fi,fo", [(44100, 96000), (44100, 48000)])
@pytest.mark.parametrize("S,nch", [(65, 2), (43, 3), (100, 2)])
def test_seam_groups_with_a_partial_last_group(fi, fo, S, nch):
    """seam_kernel takes 64 channels a workgroup: 130 channels are two full groups and one of 2, 129 leave a lone channel in the
    last group, 200 are a library-sized count that is no power of two."""
    C = S * nch
    assert C > 64 and C % 64 != 0
    run = batch_against_reference(fi, fo, nch, S, FLOAT, {}, PUSHES_B)
    for call in range(len(PUSHES_B)):
        assert ran(run, "rsmp::seam_kernel", call) and ran(run, "rsmp::fused", call), run.kernels(call)


# ------------------------------------------------------------------------------------------------------ C: polyi's group walk

@pytest.mark.parametrize("fi,fo,kw", [(44100, 48001, {}), (44100, 48001, {"quality": 1}), (96000, 44101, {})],
                         ids=["44100-48001", "44100-48001-q1", "96000-44101"])
def test_polyi_walks_several_groups_in_a_workgroup(fi, fo, kw):
    """polyi_kernel's grid holds gy = min(groups, ceil(3072 / tiles)) groups of 16 channels side by side and walks the others in
    the kernel (kernels.hip, launch_poly).  39 streams x 5 channels are 13 groups with a partial last one; a first push that
    yields m >= 35 713 frames has 280 tiles or more, so gy <= 11 < 13 and some workgroups take two groups; a second, short
    push has gy == 13."""
    S, nch = 39, 5
    C = S * nch
    ngroups = -(-C // 16)
    pushes = (max(36000, -(-36500 * fi // fo)), -(-9000 * fi // fo))
    plan = F.describe_plan(fi, fo, **kw)
    assert plan["stages"][-1]["kind"] == "poly" and plan["stages"][-1]["interp_order"] >= 1, plan["stages"]
    run = batch_against_reference(fi, fo, nch, S, FLOAT, kw, pushes)
    gys = []
    for call in range(2):
        assert run.launches("rsmp::polyi_kernel<", call) == 1, run.reports[call]   # one launch: its count is the call's frames
        m = run.counts[call]
        gys.append(min(ngroups, -(-3072 // -(-m // 128))))
    print("polyi: groups %d, gy per push %s, frames per push %s" % (ngroups, gys, run.counts[:2]))
    assert gys[0] < ngroups, (gys, ngroups)
    assert gys[1] == ngroups, (gys, ngroups)


# -------------------------------------------------------------------------------------------------------- D: long-block rounds

# (fi, fo, kw, block length, S, nch, blocks in the one push)
CASES_D = {
    "npairs3": (24000, 8000, BW99, 32768, 1, 5, 7),                # 16 items a round: the boundary lies one pair into the sixth block
    "cap": (24000, 8000, BW99, 32768, 130, 2, 5),                  # 512 items a round: 122 pairs into the fourth block
    "npairs3-65536": (16000, 8000, {"bandwidth": 99.7}, 65536, 1, 5, 7),
}


@pytest.mark.parametrize("case", list(CASES_D))
def test_long_block_rounds_with_a_boundary_inside_a_block(case):
    """launch_dft_big takes the (block, pair) items of a launch in rounds of ws_items (dftbig.hip).  One push that spans several
    rounds, with ws_items no multiple of the pairs, so that a round ends inside a block.  The profile has one record per call of
    launch_dft_big, whatever its rounds: the test asserts that the whole push was ONE call and counts the rounds from the plan
    (blocks in the push x pairs against ws_items, as Engine::init_dft_stage sizes it).  One stream is compared with a one-stream
    handle that is pushed the same frames in pieces of at most two blocks, one round each (the header promises push-size
    invariance for these blocks).  A batch has every stream compared with its one-stream handle given the same single push (5
    items: one round); a one-stream case, whose single push is itself the launch of several rounds, is held to the oracle."""
    fi, fo, kw, N, S, nch, nblocks = CASES_D[case]
    plan = F.describe_plan(fi, fo, **kw)
    assert len(plan["stages"]) == 1 and plan["stages"][0]["dft_length"] == N, plan["stages"]
    n = B.frames_for_blocks(plan, nblocks) + 17
    assert B.first_stage_blocks(plan, [n]) == [nblocks] and n <= plan["isamp_max"]
    npairs, ws_items, rounds = B.big_rounds(plan, nch, S, nblocks)
    print("long blocks %s: %d frames, %d blocks x %d pairs, %d items a round, %d rounds" % (case, n, nblocks, npairs, ws_items, rounds))
    assert rounds >= 2 and ws_items % npairs != 0 and ws_items < nblocks * npairs, (npairs, ws_items, rounds)
    streams = B.dealt(S)
    base = B.base_signals(n, nch, FLOAT)
    run = B.run_device(fi, fo, nch, S, FLOAT, kw, base, streams, [n])
    assert run.launches("rsmp::big_cols_fwd_kernel", 0) == 1, run.reports[0]     # the push's blocks went to one launch_dft_big
    # the same frames in pieces: at most two blocks a push, one round each
    piece = 30011
    pieces = [piece] * (n // piece) + ([n % piece] if n % piece else [])
    assert max(B.first_stage_blocks(plan, pieces)) * ((nch + 1) // 2) <= 16
    small = B.run_device(fi, fo, nch, 1, FLOAT, kw, base, [streams[-1]], pieces)
    assert sum(small.counts) == sum(run.counts)
    B.assert_same_bits(run.bits[S - 1], small.bits[0], "stream %d against its frames pushed in pieces of %d" % (S - 1, piece))
    if S > 1:
        ref_bits, ref_counts = B.reference(fi, fo, nch, FLOAT, B.frozen(kw), (n,))
        B.assert_streams_equal_reference(run, streams, ref_bits, ref_counts)
    else:
        B.check_against_oracle(run.numpy()[0].view("float32"), fi, fo, nch, FLOAT, kw, base[0], [n])


# ----------------------------------------------------------------------------------- E: channel and stream counts in grid.y

def test_flow_device_without_stages_writes_the_frames_it_reports():
    """in_rate == out_rate: the handle's input ring is its output fifo and no kernel writes the caller's buffer, so a flow's frames
    must come out of the ring by a copy.  (flow_device used to count them as written in place and leave the buffer as it was:
    found by the sentinel of the 65 537-stream case below.)  Three stereo streams; the output is the input."""
    S, nch, n = 3, 2, 100
    run = batch_against_reference(44100, 44100, nch, S, FLOAT, {}, (n,))
    assert run.counts == [n, 0]
    x = B.base_signals(n, nch, FLOAT)
    for s in range(S):
        B.assert_same_bits(run.bits[s], x[s % B.K].view("int32"), "stream %d against its input" % s)


def test_more_than_65535_streams_in_grid_y():
    """44100 -> 44100 has no stage: a push is copied into the ring and a pull out of it by copy_frames_kernel, whose grid.y is
    the stream count (kernels.hip, copy_range; the copies carry no profile record, so there is no kernel name to assert).  65 537
    mono streams of 64 frames."""
    S, nch, n = 65537, 1, 64
    assert S > 65535 and F.describe_plan(44100, 44100)["stages"] == []
    run = batch_against_reference(44100, 44100, nch, S, FLOAT, {}, (n,))
    print("grid.y = %d streams: handle footprint %.2f GB, %.1f ms from open to close" % (S, run.footprint / 2.0 ** 30, run.seconds * 1e3))
    assert sum(run.counts) == n


def test_more_than_65535_channels_in_grid_y():
    """192000 -> 44100 begins with a half-band stage, whose grid.y is the channel count (kernels.hip, launch_half; so is the
    element-wise copy's that moves an fp64 ring when it grows, but the copies carry no profile record and none is asserted).
    32 769 stereo streams are 65 538 channels; stream 32 767 (channels 65 534 and 65 535) gets base signal 0 and stream 32 768
    base signal 1.  Measured: the handle takes 10.01 GB of device memory, 4.3 GB of it the fused pair's seam ring."""
    S, nch, n = 32769, 2, 2048
    assert S * nch > 65535 and B.dealt(S)[32767] != B.dealt(S)[32768]
    run = batch_against_reference(192000, 44100, nch, S, FLOAT, {}, (n,))
    print("grid.y = %d channels: handle footprint %.2f GB, %.1f ms from open to close" % (S * nch, run.footprint / 2.0 ** 30, run.seconds * 1e3))
    assert ran(run, "rsmp::half_kernel<") and ran(run, "rsmp::fused"), run.kernels()
