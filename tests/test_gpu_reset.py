"""RRX_reset on the device (csrc/engine.cpp Engine::reset; DESIGN.md 11, "Libraries"): a handle that was used, reset and used again
against a FRESH handle given the same calls.

The bar throughout is EQUALITY of raw bytes.  What goes through the handle before the reset carries NaN, +-1e30 and full-scale runs
(integer handles: full-scale runs), up to its last frames, so that a ring position, a seam slot or a counter the reset left alone
shows up as a NaN, a huge value or a shifted frame behind it; everything a float handle gives after the reset must also be finite."""
import ctypes as C
import functools

import numpy as np
import pytest

import foo_dsp_resampler_amd as F
from chain_ld import BW99
from devbuf import dev_zeros
from oracle_binding import lcg_noise

pytestmark = pytest.mark.gpu

F32, F64, S16, S32 = F.RRX_FMT_FLOAT, F.RRX_FMT_DOUBLE, F.RRX_FMT_S16, F.RRX_FMT_S32
NP = {F32: np.float32, F64: np.float64, S16: np.int16, S32: np.int32}
# every kernel family: lean fused pairs up and down, the sub-blocked form in a three-stage chain, an interpolated polyphase stage,
# a half-band stage in front, and a filter that is not linear phase
CHAINS = [("44k1_96k", 44100, 96000, {}), ("44k1_48k", 44100, 48000, {}), ("96k_44k1", 96000, 44100, {}),
          ("44k1_192k_bw99", 44100, 192000, BW99), ("44k1_48001", 44100, 48001, {}), ("192k_44k1_half", 192000, 44100, {}),
          ("44k1_48k_phase25", 44100, 48000, {"phase": 25.0})]
CHAIN_IDS = [c[0] for c in CHAINS]
# (format, streams, channels): all four formats, one stream and three, one to three channels; the odd-channel batches matter
SHAPES = [(F32, 3, 3), (F32, 1, 1), (F64, 3, 1), (F64, 1, 2), (S16, 1, 3), (S16, 3, 3), (S32, 3, 2), (S32, 1, 1)]
SHAPE_IDS = ["f32_3x3", "f32_1x1", "f64_3x1", "f64_1x2", "s16_1x3", "s16_3x3", "s32_3x2", "s32_1x1"]
DIRTY_FRAMES = 30011
# after the reset: 1024-frame pushes, a flow straight into the caller's buffer, more pushes, one long odd push; about 50 000 frames,
# three blocks of the longest DFT stage (16384 points) and of the 4096-point stage behind a half-band stage
SCRIPT = [("push", 1024)] * 8 + [("flow", 20000)] + [("push", 1024)] * 4 + [("push", 17001)]


def tdtype(fmt):
    import torch
    return {F32: torch.float32, F64: torch.float64, S16: torch.int16, S32: torch.int32}[fmt]


@functools.lru_cache(maxsize=None)
def clean(fmt, S, nch, frames, seed=11):
    """[S, frames, nch] of the handle's format, read-only: noise at half of full scale (both handles of a comparison get the same
    array, so the generator only has to be quick: a big push is nine million samples)"""
    x = np.random.default_rng(seed).uniform(-0.5, 0.5, (S, frames, nch))
    if fmt in (S16, S32):
        x = np.rint(x * 2.0 ** (15 if fmt == S16 else 31))
    x = np.ascontiguousarray(x.astype(NP[fmt]))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def dirty(fmt, S, nch, frames):
    """what must leave no trace: NaN, +-1e30 and full-scale runs (integer: full-scale runs), in the middle and in the last frames,
    which no stage has consumed when the reset comes"""
    x = clean(fmt, S, nch, frames, seed=29).copy()
    if fmt in (S16, S32):
        lo, hi = np.iinfo(NP[fmt]).min, np.iinfo(NP[fmt]).max
        for at in (100, frames // 2, frames - 700):
            x[:, at:at + 300] = hi
            x[:, at + 300:at + 600] = lo
        x[:, -40:-20] = lo
        x[:, -20:] = hi
    else:
        for at in (100, frames // 2, frames - 700):
            x[:, at] = np.nan
            x[:, at + 50] = 1e30
            x[:, at + 90] = -1e30
            x[:, at + 100:at + 400] = 1.0
            x[:, at + 400:at + 600] = -1.0
        x[:, -9] = 1e30
        x[:, -6] = -1e30
        x[:, -3:] = np.nan
    x.setflags(write=False)
    return x


def to_dev(x):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    torch.cuda.synchronize()
    return t


def shaped(r, t):
    """a one-stream handle takes [frames, nch]"""
    return t[0] if r.nstreams == 1 else t


def pull_all_device(r):
    """everything available, through pull_device, as bytes"""
    out = []
    while r.available:
        n = r.available
        y = dev_zeros((r.nstreams, n, r.nch), tdtype(r.sample_format))
        got = r.pull_device(shaped(r, y), n, stride=n)
        r.sync()
        out.append(y[:, :got].cpu().numpy().tobytes())
    return b"".join(out)


def run_device(r, fmt, script=SCRIPT, seed=11, drain=True):
    """the calls of `script` on device buffers, then a drain: every byte the handle gave.  The input tensors live until the handle
    has been waited for: the calls only enqueue, and torch would hand a freed tensor's memory to the next one."""
    total = sum(n for _, n in script)
    x = clean(fmt, r.nstreams, r.nch, total, seed)
    out, pos, keep = [], 0, []
    for what, n in script:
        t = to_dev(x[:, pos:pos + n])
        keep.append(t)
        pos += n
        if what == "push":
            r.push_device(shaped(r, t), n, stride=n)
            out.append(pull_all_device(r))
        else:
            cap = pos * r.cfg.out_rate // r.cfg.in_rate + 64     # (room for what the pushes before it left in the chain, too)
            y = dev_zeros((r.nstreams, cap, r.nch), tdtype(fmt))
            used, got = r.flow_device(shaped(r, t), n, shaped(r, y), cap, in_stride=n, out_stride=cap)
            r.sync()
            assert used == n
            out.append(y[:, :got].cpu().numpy().tobytes())
            out.append(pull_all_device(r))
    if drain:
        r.drain()
        out.append(pull_all_device(r))
    r.sync()
    return b"".join(out)


def soil(r, fmt, state):
    """bring the handle into one of the three states a reset must undo; returns what the caller keeps alive until the handle has been
    waited for (nothing here synchronises behind the last call: the reset must order itself behind what is queued)"""
    if state == "big_push":
        # ONE push of isamp_max frames: the rings grow, the push is cut into slabs whose seam kernels run on the side stream
        n = r.isamp_max
        x = to_dev(dirty(fmt, r.nstreams, r.nch, n))
        r.push_device(shaped(r, x), n, stride=n)
        assert r.available > 0
        return x
    x = to_dev(dirty(fmt, r.nstreams, r.nch, DIRTY_FRAMES))
    r.push_device(shaped(r, x), DIRTY_FRAMES, stride=DIRTY_FRAMES)
    if state == "drained":                       # after drain and a full pull
        pull_all_device(r)
        r.drain()
        pull_all_device(r)
        assert r.available == 0
    else:                                        # mid-stream: output pending, nothing drained
        assert state == "midstream"
        y = dev_zeros((r.nstreams, 1000, r.nch), tdtype(fmt))
        assert r.pull_device(shaped(r, y), 1000, stride=1000) == 1000
        assert r.available > 0
        return x, y
    return x


def check_finite(raw, fmt):
    if fmt in (F32, F64):
        assert np.isfinite(np.frombuffer(raw, dtype=NP[fmt])).all(), "a NaN or a huge value from before the reset came out"


def open_handle(fs, fo, kw, fmt, S, nch):
    if fmt == F32:
        return F.Resampler(fs, fo, nch=nch, nstreams=S, **kw)
    return F.Resampler(fs, fo, nch=nch, nstreams=S, sample_format=fmt, **kw)


@functools.lru_cache(maxsize=None)
def fresh_device(fs, fo, kw_items, fmt, S, nch):
    """what a FRESH handle gives for SCRIPT: computed once per chain and shape, shared by the states"""
    r = open_handle(fs, fo, dict(kw_items), fmt, S, nch)
    raw = run_device(r, fmt)
    r.close()
    assert len(raw) > 0
    return raw


def reset_against_fresh(fs, fo, kw, fmt, S, nch, state):
    r = open_handle(fs, fo, kw, fmt, S, nch)
    isamp_max = r.isamp_max
    keep = soil(r, fmt, state)
    r.reset()
    assert r.available == 0 and r.isamp_max == isamp_max
    got = run_device(r, fmt)
    r.close()
    del keep
    want = fresh_device(fs, fo, tuple(sorted(kw.items())), fmt, S, nch)
    print(fs, fo, kw, fmt, S, nch, state, len(got), "bytes")
    assert len(got) == len(want)
    assert got == want
    check_finite(got, fmt)


@pytest.mark.parametrize("state", ["drained", "midstream", "big_push"])
@pytest.mark.parametrize("name,fs,fo,kw", CHAINS, ids=CHAIN_IDS)
def test_reset_equals_fresh_in_every_kernel_family(name, fs, fo, kw, state):
    reset_against_fresh(fs, fo, kw, F32, 1, 2, state)


@pytest.mark.parametrize("state", ["drained", "midstream"])
@pytest.mark.parametrize("fmt,S,nch", SHAPES, ids=SHAPE_IDS)
def test_reset_equals_fresh_in_every_format_and_shape(fmt, S, nch, state):
    reset_against_fresh(44100, 96000, {}, fmt, S, nch, state)


@pytest.mark.parametrize("fs,fo", [(44100, 48000), (96000, 44100)])
def test_reset_of_an_odd_channel_batch_after_a_big_push(fs, fo):
    reset_against_fresh(fs, fo, {}, F32, 3, 3, "big_push")


def run_host(r, fmt, chunks, seed, drain=True, pull_last=True):
    """plugin-sized host chunks (RR_push / RRX_push_strided ..., then pull until empty), as bytes"""
    total = sum(chunks)
    x = clean(fmt, r.nstreams, r.nch, total, seed) if seed else dirty(fmt, r.nstreams, r.nch, total)
    out, pos = [], 0
    for k, n in enumerate(chunks):
        r.push(shaped(r, x[:, pos:pos + n]))
        pos += n
        if pull_last or k + 1 < len(chunks):
            out.append(r.pull_all(chunk=8192).tobytes())
    if drain:
        r.drain()
        out.append(r.pull_all(chunk=8192).tobytes())
    return b"".join(out)


@pytest.mark.parametrize("fmt,S,nch", [(F32, 1, 2), (S16, 3, 3), (F64, 1, 3)], ids=["f32_1x2", "s16_3x3", "f64_1x3"])
def test_reset_on_the_host_path_with_frames_in_the_mirror(fmt, S, nch):
    fs, fo = 44100, 96000
    chunks = [4096, 1024, 8192, 4096, 2000, 4096, 4096]
    r = open_handle(fs, fo, {}, fmt, S, nch)
    run_host(r, fmt, [4096] * 5, seed=0, drain=False, pull_last=False)     # the last push's output sits un-pulled in the host mirror
    assert r.available > 0
    r.reset()
    assert r.available == 0
    got = run_host(r, fmt, chunks, seed=5)
    # ... and once more, now from the middle of a stream whose output was pulled
    run_host(r, fmt, [4096] * 3, seed=0, drain=False)
    r.reset()
    again = run_host(r, fmt, chunks, seed=5)
    r.close()
    f = open_handle(fs, fo, {}, fmt, S, nch)
    want = run_host(f, fmt, chunks, seed=5)
    f.close()
    assert len(want) > 0 and got == want and again == want
    check_finite(got, fmt)


def test_reset_of_a_fresh_handle_and_two_in_a_row():
    fs, fo = 44100, 96000
    want = fresh_device(fs, fo, (), F32, 1, 2)
    r = open_handle(fs, fo, {}, F32, 1, 2)
    r.reset()                                    # of a fresh handle
    r.reset()
    assert run_device(r, F32) == want
    r.reset()                                    # after a whole track, twice in a row
    r.reset()
    assert r.available == 0
    assert run_device(r, F32) == want
    keep = soil(r, F32, "midstream")
    r.reset()
    r.reset()
    assert run_device(r, F32) == want
    del keep
    r.close()


def test_without_a_reset_the_bytes_differ():
    """the control of everything above: the same calls on a used handle that was NOT reset give other bytes, and for the states
    that leave NaN in the chain's history, NaN"""
    fs, fo = 44100, 96000
    want = fresh_device(fs, fo, (), F32, 1, 2)
    for state in ("midstream", "big_push"):
        r = open_handle(fs, fo, {}, F32, 1, 2)
        keep = soil(r, F32, state)
        pull_all_device(r)
        got = run_device(r, F32)
        r.close()
        del keep
        assert got != want, state
        assert not np.isfinite(np.frombuffer(got, dtype=np.float32)).all(), state


def test_reset_keeps_the_callers_stream():
    import torch
    fs, fo = 44100, 96000
    want = fresh_device(fs, fo, (), F32, 1, 2)
    side = torch.cuda.Stream()
    r = open_handle(fs, fo, {}, F32, 1, 2)
    r.set_stream(side.cuda_stream)
    keep = soil(r, F32, "midstream")
    r.reset()
    assert r._stream == side.cuda_stream
    # everything below is queued by the handle alone; waiting for the CALLER's stream, and for nothing else, must find it done
    n, cap = 20000, 20000 * fo // fs + 64
    x = to_dev(clean(F32, 1, 2, n, 17))
    y = dev_zeros((cap, 2))
    used, got = r.flow_device(x[0], n, y, cap)
    side.synchronize()
    first = y[:got].cpu().numpy().tobytes()
    r.reset()
    assert run_device(r, F32) == want
    r.use_own_stream()
    r.close()
    f = open_handle(fs, fo, {}, F32, 1, 2)
    y2 = dev_zeros((cap, 2))
    used2, got2 = f.flow_device(x[0], n, y2, cap)
    f.sync()
    assert (used, got) == (used2, got2) and got > 0 and first == y2[:got2].cpu().numpy().tobytes()
    f.close()
    torch.cuda.synchronize()


@pytest.mark.parametrize("fs,fo", [(44100, 48000), (96000, 44100)])
def test_counters_are_fresh_after_a_reset(fs, fo):
    """a second track longer than one second of input AND of output (the whole-second wrap of the counters) drains to the total
    RRX_track_geometry plans for a handle of its own"""
    lead, ext, out_first, out_frames = F.track_geometry(fs, fo, 120000)
    assert ext > fs and out_frames > fo and ext <= 1048576 * min(1.0, fs / fo)
    r = open_handle(fs, fo, {}, F32, 1, 2)
    keep = soil(r, F32, "drained")               # a first track of its own length, drained: the counters have moved and wrapped
    r.reset()
    assert r.available == 0
    raw = run_device(r, F32, script=[("push", ext)], seed=3)
    r.close()
    frames = len(raw) // (2 * 4)
    print(fs, fo, "ext", ext, "frames out", frames, "planned", out_frames + 2 * out_first, "rounded", round(ext * fo / fs))
    assert frames == out_frames + 2 * out_first
    assert frames == int(ext * fo / fs + 0.5)


def test_a_poisoned_handle_stays_poisoned():
    L = F.lib()
    x = lcg_noise(200000, 2, 2)
    r = F.Resampler(44100, 96000, 2)
    r.push(x[:100000])                           # (as tests/test_gpu_round2.py::test_failed_push_poisons_the_handle)
    L.RRX_debug_fail_alloc(1)
    rc = L.RR_push(r.h, x[100000:].ctypes.data, 100000)
    L.RRX_debug_fail_alloc(0)
    assert rc == 1, rc
    assert L.RRX_reset(r.h) == 2                 # RR_INTERNAL, like every data call
    assert L.RR_push(r.h, x.ctypes.data, 100) == 2
    assert L.RRX_reset(r.h) == 2
    assert L.RR_drain(r.h) == 2
    with pytest.raises(F.RRError):
        r.reset()
    r.close()
    assert L.RRX_reset(C.c_void_p()) == 3        # RR_NULLHANDLE
