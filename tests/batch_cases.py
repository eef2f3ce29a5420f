"""What the tests of the resampling chain's own seams share (tests/test_gpu_batch_seams.py): the inputs, the caller and the
reference.

ratelib_amd.h promises every stream of a batch handle, bit for bit, the output of a one-stream handle fed the same samples in the
same call sequence.  To hold EVERY stream of a batch to that without one reference run per stream, stream s of a batch gets base
signal s % 7 of K = 7 signals lcg_noise(n, nch, seed + k): 7 is coprime to every width the chain's kernels index by (2 channels
of a pair, 8 XCDs, 16 channels of a polyi group, 64 channels of a seam group, the pairs of a frame, the pairs of a handle, the
items of a workspace round), so an index that is off by one of those widths lands on a stream whose expected output differs.  The
expected outputs are 7 runs of a one-stream handle of the same format, configuration and call sequence; base signal 0 is also
held to the CPU oracle, so that the one-stream handle cannot share a mistake with the batch.

The caller works on torch's current stream through flow_device / pull_device, with output rows farther apart than the capacity it
offers, into a buffer prefilled with a bit pattern no output takes (the references are checked for it): everything outside the
frames a call reported must still hold it."""
import functools
import time

import numpy as np

import foo_dsp_resampler_amd as F
from oracle_binding import Oracle, lcg_noise
from parity import assert_parity

K = 7
SEED = 90210
ROW_TAIL = 5                      # frames between the capacity a call is offered and the next row
FMT_DTYPE = {F.RRX_FMT_FLOAT: np.float32, F.RRX_FMT_DOUBLE: np.float64, F.RRX_FMT_S16: np.int16, F.RRX_FMT_S32: np.int32}
# float formats: a NaN with a payload (finite inputs give finite outputs); integer formats: the most negative value, which an
# output takes only by clipping at -1.0 (the PCM inputs stay within +-0.25, and reference() asserts that no output holds it)
SENTINEL = {F.RRX_FMT_FLOAT: 0x7FA5A5A5, F.RRX_FMT_DOUBLE: 0x7FF5A5A5A5A5A5A5, F.RRX_FMT_S16: -0x8000, F.RRX_FMT_S32: -0x80000000}
BITS_DTYPE = {F.RRX_FMT_FLOAT: np.int32, F.RRX_FMT_DOUBLE: np.int64, F.RRX_FMT_S16: np.int16, F.RRX_FMT_S32: np.int32}


def frozen(kw):
    return tuple(sorted(kw.items()))


@functools.lru_cache(maxsize=None)
def base_signals(n, nch, fmt=F.RRX_FMT_FLOAT, seed=SEED):
    """[7, n, nch] in the format's dtype: noise on +-0.5 with 24 bits; for the PCM formats on +-0.25, scaled by 2^14 (rounded) or
    2^30 (white noise at +-0.5 comes out of the 99 % band chains with peaks of full scale, measured: -32768 in 1 of 801 088
    samples of 44100 -> 192000 on 8 channels; at half the level no output clips, and so none takes the sentinel)"""
    x = np.stack([lcg_noise(n, nch, seed + k) for k in range(K)])
    if fmt == F.RRX_FMT_S16:
        x = np.rint(x.astype(np.float64) * 2.0 ** 14).astype(np.int16)
    elif fmt == F.RRX_FMT_S32:
        x = np.rint(x.astype(np.float64) * 2.0 ** 30).astype(np.int32)
    else:
        x = x.astype(FMT_DTYPE[fmt])
    x.setflags(write=False)
    return x


def as_oracle_input(x, fmt):
    """what the handle makes of its input samples, as the float32 the oracle takes: exact for every format"""
    if fmt == F.RRX_FMT_S16:
        return (x.astype(np.float64) * 2.0 ** -15).astype(np.float32)
    if fmt == F.RRX_FMT_S32:
        return (x.astype(np.float64) * 2.0 ** -31).astype(np.float32)
    return x.astype(np.float32)


def open_handle(fi, fo, nch, S, fmt, kw):
    if fmt == F.RRX_FMT_FLOAT:
        return F.Resampler(fi, fo, nch=nch, nstreams=S, **kw)
    if fmt == F.RRX_FMT_DOUBLE:
        return F.Resampler(fi, fo, nch=nch, nstreams=S, dtype=np.float64, **kw)
    return F.Resampler(fi, fo, nch=nch, nstreams=S, sample_format=fmt, **kw)


class Run:
    """what a call sequence left: `bits` [S, total, nch] (the output's bit patterns; a device tensor after run_device, a numpy
    array after run_host), `counts` (frames per call, the drain's pull last), `reports` (profile_report() after each push and
    after the drain), `footprint` (bytes of device memory the open took) and `seconds` (wall time, open to last sync)"""

    def __init__(self, bits, counts, reports, footprint, seconds):
        self.bits, self.counts, self.reports, self.footprint, self.seconds = bits, counts, reports, footprint, seconds

    def kernels(self, call=None):
        reps = self.reports if call is None else [self.reports[call]]
        return sorted({k["kernel"] for rep in reps for k in rep})

    def launches(self, prefix, call):
        return sum(k["launches"] for k in self.reports[call] if k["kernel"].startswith(prefix))

    def numpy(self):
        return self.bits if isinstance(self.bits, np.ndarray) else self.bits.cpu().numpy()


def out_frames(fi, fo, n):
    return (n * fo + fi - 1) // fi


def run_device(fi, fo, nch, S, fmt, kw, base, streams, pushes):
    """A handle of S streams, stream s fed base[streams[s]], one flow_device per entry of `pushes` (frames), drain, one
    pull_device, all on torch's current stream.  Every output row is ROW_TAIL frames longer than the capacity the calls are
    offered and starts as the sentinel; what lies behind the frames the calls reported must still be the sentinel."""
    import torch
    tdt = getattr(torch, np.dtype(FMT_DTYPE[fmt]).name)
    bdt = getattr(torch, np.dtype(BITS_DTYPE[fmt]).name)
    n = sum(pushes)
    assert base.shape[1] >= n and len(streams) == S
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    t0 = time.perf_counter()
    r = open_handle(fi, fo, nch, S, fmt, kw)
    torch.cuda.synchronize()
    footprint = free0 - torch.cuda.mem_get_info()[0]
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    r.profile(True)
    xb = torch.from_numpy(np.array(base[:, :n])).cuda()                          # (a copy: the cached signals are read-only)
    x = xb[torch.as_tensor(np.asarray(streams, dtype=np.int64)).cuda()]         # [S, n, nch]
    cap = out_frames(fi, fo, n) + 64
    stride = cap + ROW_TAIL
    ybits = torch.full((S, stride, nch), SENTINEL[fmt], dtype=bdt, device="cuda")
    y = ybits.view(tdt)
    counts, reports, got, lo = [], [], 0, 0
    for k in pushes:
        assert k <= r.isamp_max, (k, r.isamp_max)
        seg = x[:, lo:lo + k].contiguous()
        iu, og = r.flow_device(seg, k, y[:, got:], cap - got, out_stride=stride)
        assert iu == k, (iu, k)
        reports.append(r.profile_report())
        counts.append(og)
        got += og
        lo += k
    r.drain()
    og = r.pull_device(y[:, got:], cap - got, stride=stride)
    r.sync()
    reports.append(r.profile_report())
    counts.append(og)
    got += og
    assert r.available == 0 and got < cap, (r.available, got, cap)
    r.profile(False)
    r.close()
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    behind = ybits[:, got:]
    assert bool((behind == SENTINEL[fmt]).all()), "frames behind the %d a stream was given were written" % got
    return Run(ybits[:, :got], counts, reports, footprint, seconds)


def run_host(fi, fo, nch, S, fmt, kw, base, streams, pushes):
    """the same call sequence through push / pull_all on host arrays: the output goes through the handle's ring"""
    r = open_handle(fi, fo, nch, S, fmt, kw)
    r.profile(True)
    x = base[np.asarray(streams)] if S > 1 else base[streams[0]]
    parts, counts, reports, lo = [], [], [], 0
    ax = 0 if S == 1 else 1
    for k in pushes:
        r.push(x[lo:lo + k] if S == 1 else x[:, lo:lo + k])
        p = r.pull_all()
        reports.append(r.profile_report())
        parts.append(p)
        counts.append(p.shape[ax])
        lo += k
    r.drain()
    p = r.pull_all()
    reports.append(r.profile_report())
    parts.append(p)
    counts.append(p.shape[ax])
    r.profile(False)
    r.close()
    y = np.concatenate(parts, axis=ax)
    if S == 1:
        y = y[None]
    return Run(np.ascontiguousarray(y).view(BITS_DTYPE[fmt]), counts, reports, 0, 0.0)


@functools.lru_cache(maxsize=None)
def reference(fi, fo, nch, fmt, kwf, pushes, path="device", seed=SEED):
    """(bits [7, total, nch] as a read-only numpy array, frames per call): a one-stream handle on each base signal, the same calls.
    Signal 0's output is held to the oracle here, once."""
    kw = dict(kwf)
    base = base_signals(sum(pushes), nch, fmt, seed)
    run = run_device if path == "device" else run_host
    runs = [run(fi, fo, nch, 1, fmt, kw, base, [k], pushes) for k in range(K)]
    assert all(r.counts == runs[0].counts for r in runs), [r.counts for r in runs]
    bits = np.concatenate([r.numpy() for r in runs])
    assert not (bits == np.array(SENTINEL[fmt]).astype(BITS_DTYPE[fmt])).any(), "an output of the reference holds the sentinel"
    assert len({bits[k].tobytes() for k in range(K)}) == K, "two base signals gave one output"
    check_against_oracle(bits[0].view(FMT_DTYPE[fmt]), fi, fo, nch, fmt, kw, base[0], pushes)
    bits.setflags(write=False)
    return bits, runs[0].counts


def check_against_oracle(y, fi, fo, nch, fmt, kw, x, pushes):
    """One stream's output against the CPU oracle fed the same pushes.  float32: the parity bar (1 ulp, 1e-7 relative RMS).
    float64: the same after rounding the output to float32 -- the oracle's float32 is its own fp64 sum rounded, the two fp64 sums
    agree to 1e-13 (test_gpu_fp64_parity.py), so the two roundings differ by one ulp at most, and only beside a tie.  16-bit PCM:
    the oracle's float32 carries 2^-24 relative error, far below half an LSB of 16 bits, so the oracle's output rounded to 16
    bits and the handle's differ by at most one LSB, again only beside a tie.  32-bit PCM is compared as float32 at the parity
    bar."""
    o = Oracle(fi, fo, nch, **kw)
    xo = as_oracle_input(x, fmt)
    parts, lo = [], 0
    for k in pushes:
        o.push(xo[lo:lo + k])
        parts.append(o.pull_all())
        lo += k
    o.drain()
    parts.append(o.pull_all())
    ref = np.concatenate(parts)
    assert ref.shape == y.shape, (ref.shape, y.shape)
    if fmt == F.RRX_FMT_S16:
        d = y.astype(np.int64) - np.rint(ref.astype(np.float64) * 2.0 ** 15).astype(np.int64)
        assert np.abs(d).max() <= 1, int(np.abs(d).max())
    elif fmt == F.RRX_FMT_S32:
        assert_parity((y.astype(np.float64) * 2.0 ** -31).astype(np.float32), ref)
    else:
        assert_parity(y.astype(np.float32), ref)


def assert_streams_equal_reference(run, streams, ref_bits, ref_counts):
    """every stream of the run, bit for bit, against the reference of its base signal; names the first (stream, channel, frame)"""
    assert run.counts == ref_counts, (run.counts, ref_counts)
    if isinstance(run.bits, np.ndarray):
        bad = run.bits != ref_bits[np.asarray(streams)]
        if bad.any():
            s, f, c = [int(v) for v in np.argwhere(bad)[0]]
            raise AssertionError("stream %d (base signal %d) channel %d frame %d: %#x, one-stream handle %#x; %d of %d samples differ"
                                 % (s, streams[s], c, f, int(run.bits[s, f, c]), int(ref_bits[streams[s], f, c]), int(bad.sum()), bad.size))
        return
    import torch
    ref = torch.from_numpy(np.array(ref_bits)).cuda()
    idx = torch.as_tensor(np.asarray(streams, dtype=np.int64)).cuda()
    assert tuple(run.bits.shape[1:]) == tuple(ref.shape[1:]), (run.bits.shape, ref.shape)
    nbad, first = 0, None
    for s0 in range(0, len(streams), 4096):                                     # (slices: the gathered reference of 65537 streams stays small)
        bad = run.bits[s0:s0 + 4096] != ref[idx[s0:s0 + 4096]]
        k = int(bad.sum())
        if k and first is None:
            s, f, c = [int(v) for v in torch.nonzero(bad)[0]]
            first = (s0 + s, f, c)
        nbad += k
    if nbad:
        s, f, c = first
        raise AssertionError("stream %d (base signal %d) channel %d frame %d: %#x, one-stream handle %#x; %d of %d samples differ"
                             % (s, streams[s], c, f, int(run.bits[s, f, c]), int(ref_bits[streams[s], f, c]), nbad, run.bits.numel()))


def assert_same_bits(got, want, what):
    """two [frames, nch] outputs of one stream (device tensors or numpy arrays), bit for bit; names the first (channel, frame)"""
    got = got if isinstance(got, np.ndarray) else got.cpu().numpy()
    want = want if isinstance(want, np.ndarray) else want.cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    if bad.any():
        f, c = [int(v) for v in np.argwhere(bad)[0]]
        raise AssertionError("%s: channel %d frame %d: %#x against %#x; %d of %d samples differ"
                             % (what, c, f, int(got[f, c]), int(want[f, c]), int(bad.sum()), bad.size))


def dealt(S):
    """stream s gets base signal s % 7"""
    return [s % K for s in range(S)]


# ------------------------------------------------------------------------------------------------ geometry, from the plan alone

def first_stage_blocks(plan, pushes):
    """blocks the chain's first dft stage takes per push (dft_filter.h:78-84 on the counters, for L = 1 and the power-of-two L
    whose blocks start at slot 0): per push, a list with one count"""
    st = plan["stages"][0]
    assert st["kind"] == "dft" and st["L"] in (1, 2, 4) and st["remL"] == 0, st
    N, L = st["dft_length"], st["L"]
    V = N - (st["num_taps"] - 1)
    take = (V + L - 1) // L
    occ, out = st["preload"], []
    for n in pushes:
        occ += n
        nb = 0
        while L * occ >= N:
            occ -= take
            nb += 1
        out.append(nb)
    return out


def frames_for_blocks(plan, nblocks):
    """the smallest first push after which the first dft stage (L = 1) holds `nblocks` whole blocks"""
    st = plan["stages"][0]
    assert st["kind"] == "dft" and st["L"] == 1, st
    N = st["dft_length"]
    V = N - (st["num_taps"] - 1)
    return N + (nblocks - 1) * V - st["preload"]


def big_rounds(plan, nch, S, nblocks):
    """(pairs, items of a workspace round, rounds) of a long-block stage's launch over `nblocks` blocks (Engine::init_dft_stage,
    launch_dft_big): a round holds at most 256 MiB of workspace and at least 4 blocks' worth of pairs, or 16 items"""
    N = plan["stages"][0]["dft_length"]
    npairs = S * ((nch + 1) // 2)
    ws_items = max(1, min((256 << 20) // (16 * N), max(4 * npairs, 16)))
    return npairs, ws_items, -(-nblocks * npairs // ws_items)
