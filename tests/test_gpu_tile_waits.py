"""GPU tests of the lean fused kernels' polyphase rounds after their waits were recounted (fused_fast.hip): the window start of a
residue group is arithmetic (multiply-high by a reciprocal of polyL) instead of a value that came with the coefficient tile,
and the tile loop runs pairs of tiles with one exit and an odd last tile behind it.

Device-resident flow calls, 3 streams each, every sample of every stream against the CPU oracle at the project's bar
(tests/parity.py: 1 ulp, 1e-7 relative RMS in float32).  The output buffer is filled with NaN before every call, so an
output that no tile stores fails its sample.  Call patterns per rate pair, in units of the chain-input frames one block of
the fused stage consumes: a call that completes exactly one block; three blocks and an odd remainder; the same input in calls of 1000 frames
(launches of one block, waves with no tile or one, rounds without tiles); and a destination that ends in the middle of a
block, the rest fetched by a second call."""
import functools

import numpy as np
import pytest

import foo_dsp_resampler_amd as F
from oracle_binding import Oracle, lcg_noise
from parity import assert_parity
from test_tile_walk import lean_chains

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

S = 3
# rate pair, channels, plan options, the lean kernel that must run (prefix, substring)
PAIRS = {
    "44k1_96k": (44100, 96000, 2, {}, ("rsmp::fused_fast_kernel<11, 7, false>", "")),           # KS 7, 10 groups
    "44k1_48k": (44100, 48000, 2, {}, ("rsmp::fused_fast_kernel<", ", 8, ")),                   # KS 8
    "96k_44k1": (96000, 44100, 4, {}, ("rsmp::fused_fast_kernel<12, ", "")),                    # x1, polyL 147: partial last group
    "44k1_192k": (44100, 192000, 8, {"bandwidth": 99.0}, ("rsmp::fused_split", "")),            # sub-blocked, fp64-ring output
}
PATTERNS = ("one_block", "three_blocks_odd", "calls_of_1000", "short_destination")


def block_frames(fi, fo, nch, kw):
    """chain-input frames that one block of the lean fused stage consumes"""
    _, chains = lean_chains(fi, fo, nch, **kw)
    assert chains, (fi, fo)
    g, ahead, dft_L = chains[0]
    return int(round(g.V / (ahead * dft_L)))


@functools.lru_cache(maxsize=None)
def noise(nch, n):
    x = np.stack([lcg_noise(n, nch, 71 + s).reshape(n, nch) for s in range(S)])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def oracle_all(name, n):
    """the oracle's output for the first n frames of every stream, pushed at once"""
    fi, fo, nch, kw, _ = PAIRS[name]
    x = noise(nch, n)
    outs = []
    for s in range(S):
        o = Oracle(fi, fo, nch, **kw)
        o.push(x[s])
        outs.append(o.pull_all())
    return outs


def flow(name, n, calls, first_cap=None):
    """calls: input frames per flow_device call; first_cap: capacity of the first call's destination (else ample), whatever it
    leaves behind is fetched by calls without input.  Returns the concatenated outputs [S, m, nch] and the kernels' names."""
    fi, fo, nch, kw, _ = PAIRS[name]
    x = noise(nch, n)
    r = F.Resampler(fi, fo, nch=nch, nstreams=S, **kw)
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    r.profile(True)
    xd = torch.from_numpy(np.array(x)).cuda()
    outs, pos = [], 0
    for i, k in enumerate(calls):
        cap = first_cap if (i == 0 and first_cap) else int(k * fo / fi) + 8192
        while True:
            xin = xd[:, pos:pos + k].contiguous() if k else None
            y = torch.full((S, cap, nch), float("nan"), dtype=torch.float32, device="cuda")
            iu, og = r.flow_device(xin, k, y, cap)
            assert iu <= k and og <= cap
            outs.append(y[:, :og].cpu().numpy())
            pos += iu
            k -= iu
            if k == 0 and og < cap:
                break
            assert iu > 0 or og > 0, (name, i, k)  # (no progress: never loops)
            cap = int(n * fo / fi) + 8192
    assert pos == n
    r.sync()
    names = sorted({k["kernel"] for k in r.profile_report()})
    r.close()
    return np.concatenate(outs, axis=1), names


def run_pattern(name, pattern):
    fi, fo, nch, kw, (prefix, sub) = PAIRS[name]
    blk = block_frames(fi, fo, nch, kw)
    n3 = 3 * blk + 37
    first_cap = None
    if pattern == "one_block":
        # a block spans more input than it consumes, and three blocks + 37 frames complete two of them: one block less of input
        # completes exactly one
        n, calls = 2 * blk + 37, (2 * blk + 37,)
    elif pattern == "three_blocks_odd":
        n, calls = n3, (n3,)
    elif pattern == "calls_of_1000":
        n, calls = n3, tuple([1000] * (n3 // 1000) + ([n3 % 1000] if n3 % 1000 else []))
    else:
        n, calls = n3, (n3,)
        first_cap = int(1.5 * blk * fo / fi) + 3  # ends inside the second block's outputs
    got, names = flow(name, n, calls, first_cap)
    print("%s %s: block %d frames, %d calls, %d outputs, kernels %s" % (name, pattern, blk, len(calls), got.shape[1], names))
    if pattern == "three_blocks_odd":
        assert any(k.startswith(prefix) and sub in k for k in names), names  # the path under test is the one that ran
    assert got.shape[1] > 0, (name, pattern)  # (no case is empty)
    refs = oracle_all(name, n)
    for s in range(S):
        assert got[s].shape == refs[s].shape, (s, got[s].shape, refs[s].shape)
        assert not np.isnan(got[s]).any(), (s, int(np.isnan(got[s]).sum()))
        assert_parity(got[s], refs[s])
    return got


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("name", list(PAIRS))
def test_call_patterns(name, pattern):
    run_pattern(name, pattern)


def test_one_call_and_calls_of_1000_give_the_same_bits():
    one = run_pattern("44k1_96k", "three_blocks_odd")
    cut = run_pattern("44k1_96k", "calls_of_1000")
    assert one.shape == cut.shape, (one.shape, cut.shape)
    assert np.array_equal(one.view(np.uint32), cut.view(np.uint32))
