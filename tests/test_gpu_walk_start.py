"""GPU tests of the lean fused kernels' table-driven polyphase rounds (fused_fast.hip): every round's start state comes from the
WalkStart record that fused_prep_kernel writes beside the block table, and the first coefficient tiles of a round are
requested ahead of the barrier in front of its image.

Device-resident flow calls on small inputs, every sample against the CPU oracle at the project's bar (tests/parity.py: 1 ulp,
1e-7 relative RMS; double and 16-bit PCM handles at the bars of tests/test_gpu_double_io.py and tests/test_gpu_int_io.py).  The
output buffer is filled with NaN (PCM: the most negative value) before every call, so an output that no tile stores fails
its sample."""
import numpy as np
import pytest

import foo_dsp_resampler_amd as F
from oracle_binding import Oracle, lcg_noise
from parity import assert_parity

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CALLS_A = (9000, 5318, 30000)  # 5318 = 3 * 1771 + 5: the second call's head block comes from the ring, K = 1 (mod 4) blocks among them
TORCH_DT = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.int16): torch.int16}


def noise(S, n, nch, seed):
    return np.stack([lcg_noise(n, nch, seed + s).reshape(n, nch) for s in range(S)])


def flow_calls(fi, fo, nch, kw, x, calls, **handle):
    """x: [S, n, nch] host array in the handle's sample type; one flow_device per entry of `calls`.  Returns the outputs of
    every call ([S, m, nch] each) and the names of the kernels that ran."""
    S = x.shape[0]
    r = F.Resampler(fi, fo, nch=nch, nstreams=S, **kw, **handle)
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    r.profile(True)
    tdt = TORCH_DT[x.dtype]
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    outs, pos = [], 0
    for k in calls:
        xin = xd[:, pos:pos + k].contiguous()
        pos += k
        cap = int(k * fo / fi) + 8192
        fill = float("nan") if tdt.is_floating_point else -32768
        y = torch.full((S, cap, nch), fill, dtype=tdt, device="cuda")
        iu, og = r.flow_device(xin, k, y, cap)
        assert iu == k
        outs.append(y[:, :og].cpu().numpy())
    assert pos == x.shape[1]
    r.sync()
    names = sorted({k["kernel"] for k in r.profile_report()})
    r.close()
    return outs, names


def oracle_calls(fi, fo, nch, kw, x1, calls):
    """the same calls on one stream of the oracle: float32 frames out of every call"""
    o = Oracle(fi, fo, nch, **kw)
    outs, pos = [], 0
    for k in calls:
        o.push(x1[pos:pos + k])
        pos += k
        outs.append(o.pull_all())
    return outs


def oracle_fifo64(fi, fo, nch, kw, x1):
    """the oracle's fp64 output fifo after one push of everything (never pulled)"""
    o = Oracle(fi, fo, nch, **kw)
    o.push(x1)
    ns = len(o.plan())
    return np.stack([o.stage_fifo(ch, ns) for ch in range(nch)], axis=1)


def check_float(fi, fo, nch, S, kw, calls, seed, lean):
    x = noise(S, sum(calls), nch, seed)
    outs, names = flow_calls(fi, fo, nch, kw, x, calls)
    assert any(k.startswith(lean) for k in names), names  # the path under test is the one that ran
    for s in range(S):
        refs = oracle_calls(fi, fo, nch, kw, x[s], calls)
        for i, ref in enumerate(refs):
            got = outs[i][s]
            assert got.shape == ref.shape, (s, i, got.shape, ref.shape)
            assert not np.isnan(got).any(), (s, i, int(np.isnan(got).sum()))
            assert_parity(got, ref)
    return outs


@pytest.fixture(scope="module")
def case_a_three_calls():
    """(a) 44.1k -> 96k, 2 streams x 2 channels, float32, three consecutive calls; shared with (f)"""
    return check_float(44100, 96000, 2, 2, {}, CALLS_A, 31, "rsmp::fused_fast_kernel<11, 7, false>")


def test_a_headline_chain_three_calls(case_a_three_calls):
    assert len(case_a_three_calls) == 3 and all(o.shape[1] > 0 for o in case_a_three_calls)  # (the checks are the fixture's)


def test_b_44k1_to_48k_stereo():
    check_float(44100, 48000, 2, 1, {}, (20000,), 32, "rsmp::fused_fast_kernel<")


def test_c_96k_to_44k1_four_channels_uniform_walk():
    check_float(96000, 44100, 4, 1, {}, (20000,), 33, "rsmp::fused_fast_kernel<")


@pytest.mark.parametrize("bw,lean", [(98.0, "rsmp::fused_split2_kernel<"), (99.0, "rsmp::fused_split_kernel<")])
def test_d_sub_blocked_forms(bw, lean):
    check_float(44100, 96000, 2, 1, {"bandwidth": bw}, (40000,), 34, lean)


def test_e_double_handle():
    """case (a) on a float64 handle, at the bar of tests/test_gpu_double_io.py::test_fp64_parity_with_oracle: 1e-13 of the
    oracle's largest sample, against its fp64 output fifo"""
    x = noise(2, sum(CALLS_A), 2, 31)
    outs, names = flow_calls(44100, 96000, 2, {}, x.astype(np.float64), CALLS_A, dtype=np.float64)
    assert any(k.startswith("rsmp::fused_fast_dio_kernel<11, 7, false>") for k in names), names
    got = np.concatenate(outs, axis=1)
    assert not np.isnan(got).any(), int(np.isnan(got).sum())
    for s in range(2):
        ref = oracle_fifo64(44100, 96000, 2, {}, x[s])
        assert ref.shape == got[s].shape, (ref.shape, got[s].shape)
        rel = np.abs(got[s] - ref).max() / np.abs(ref).max()
        print("double handle, stream %d: max |y - o| / max |o| = %.3g" % (s, rel))
        assert rel < 1e-13, rel


def test_e_pcm16_handle():
    """case (a) on a 16-bit PCM handle, at the bar of tests/test_gpu_int_io.py::test_against_oracle: within 1 LSB of the
    quantised fp64 oracle, differing only next to a rounding tie (window 2^15 * 1e-13 * max|o|), at most 0.1 % of the samples"""
    x = noise(2, sum(CALLS_A), 2, 31)
    s16 = np.rint(x.astype(np.float64) * 2.0 ** 15).astype(np.int16)
    outs, names = flow_calls(44100, 96000, 2, {}, s16, CALLS_A, sample_format=F.RRX_FMT_S16)
    assert any(k.startswith("rsmp::fused_fast_s16_kernel<11, 7, false>") for k in names), names
    got = np.concatenate(outs, axis=1)
    for s in range(2):
        xo = s16[s].astype(np.float64) * 2.0 ** -15
        ref64 = oracle_fifo64(44100, 96000, 2, {}, xo.astype(np.float32))
        assert ref64.shape == got[s].shape, (ref64.shape, got[s].shape)
        q = ref64 * 2.0 ** 15
        assert q.max() < 2.0 ** 15 - 1 and q.min() > -2.0 ** 15  # none clip (so the fill value is no valid output either)
        ref = np.clip(np.rint(q), -2.0 ** 15, 2.0 ** 15 - 1).astype(np.int16)
        window = 2.0 ** 15 * 1e-13 * np.abs(ref64).max()
        near_tie = np.abs(np.abs(q - np.floor(q)) - 0.5) <= window
        cap = 1e-3 * ref.size
        d = got[s].astype(np.int64) - ref.astype(np.int64)
        print("pcm16 handle, stream %d: differing %d, in window %d, of %d, max |d| %d" %
              (s, int(np.sum(d != 0)), int(np.sum(near_tie)), ref.size, int(np.abs(d).max())))
        assert np.sum(near_tie) <= cap
        assert np.abs(d).max() <= 1
        assert not np.any((d != 0) & ~near_tie), int(np.sum((d != 0) & ~near_tie))
        assert np.sum(d != 0) <= cap


def test_f_one_call_and_three_calls_give_the_same_bytes(case_a_three_calls):
    x = noise(2, sum(CALLS_A), 2, 31)
    outs, _ = flow_calls(44100, 96000, 2, {}, x, (sum(CALLS_A),))
    one, three = outs[0], np.concatenate(case_a_three_calls, axis=1)
    assert one.shape == three.shape, (one.shape, three.shape)
    assert not np.isnan(one).any()
    assert np.array_equal(one.view(np.uint32), three.view(np.uint32))
