"""Every device call held to its stream contract under a busy stream (include/ratelib_amd.h: "all work of a call is queued on the
caller's stream" and "the call only enqueues: no allocation, no host synchronisation"; DESIGN.md 12, "Stream order").

The arithmetic of these calls is held to its models elsewhere, always on an idle, synchronised GPU, where a launch on the wrong
stream still finds its inputs ready and a hidden host wait costs nothing.  Here every call runs behind gates (tests/stream_gate.py):
its inputs are produced on the caller's stream behind a kernel that keeps that stream busy, a second gate keeps the null stream
busy, and inputs and outputs are overwritten on the caller's stream right behind the call.  The reference is the same call made the
old way on the same buffers, and the bar is equality of bits.  Nothing here provokes a fault: a violation reads stale, valid inputs.

  1  the apparatus detects: a pending event, a stale read from the null stream, a late write from a gated null stream
  2  one row per handle-free entry point (tests/stream_order_cases.py), through the C ABI and where it takes `stream=` the wrapper
  3  the same rows past the 32768 seam of their launchers' slice loops
  4  handle calls: a script of flows, a push and pull pair, a drain, a reset in mid-pass; and a switch of streams
  5  the side stream of the engine, in a child process (tests/variant_child.py, mode side_stream_gated)
  6  the Python conversions on torch's current stream, with the steps at which their host waits

Every case prints "streamorder {json}" with its measured time and gate lengths; profiles/stream_order.jsonl is one run's lines."""
import sys
import time

import numpy as np
import pytest
import torch

import foo_dsp_resampler_amd as F
import stream_gate as G
import stream_order_cases as SOC
from chain_ld import BW99

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def stream():
    return G.independent_stream()


@pytest.fixture(scope="module", autouse=True)
def module_wall_time():
    """the module's whole wall time, from its first test to its last, printed behind the last"""
    t0 = time.perf_counter()
    yield
    print("streamorder-time module %.1f s" % (time.perf_counter() - t0))


@pytest.fixture(autouse=True)
def no_case_behind_a_gpu_error():
    """a case that left the device in error is the last one: nothing more is started on it"""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:
        pytest.exit("the GPU reported an error, no further case is started: %s" % e, returncode=3)


def driver(stream, seen, recs=None, **kw):
    def run(enqueue, inputs, outputs, entry, scratch=()):
        seen.append(entry)
        rec = G.gated(enqueue, inputs, outputs, stream, scratch=scratch, label=entry, **kw)
        if recs is not None:
            recs.append(rec)
    return run


# ------------------------------------------------------------------------------------------------------------- 1  the apparatus

def test_an_event_behind_a_gate_is_pending(stream):
    e = G.gate(stream, 100.0)
    assert not e.query()
    stream.synchronize()
    assert e.query()
    g = G.gate(G.null_stream(), 100.0)
    done = torch.cuda.Event()
    x = torch.zeros(16, device="cuda")
    with torch.cuda.stream(stream):
        x.add_(1.0)
        done.record(stream)
        stream.synchronize()
    assert done.query() and not g.query(), "the caller's stream does not run beside a gated null stream"
    torch.cuda.synchronize()


def test_a_copy_on_the_null_stream_reads_stale_values(stream):
    """what a launch on the wrong stream does: it runs while the caller's stream sleeps"""
    fresh = torch.arange(1024, dtype=torch.float32, device="cuda") + 1.0
    buf, early = torch.zeros(1024, device="cuda"), torch.full((1024,), 9.0, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        G.gate(stream, 100.0)
        buf.copy_(fresh)
    with torch.cuda.stream(G.null_stream()):
        early.copy_(buf)
    torch.cuda.synchronize()
    assert bool((early == 0.0).all()) and torch.equal(buf, fresh)


def test_an_op_on_a_gated_null_stream_is_overtaken(stream):
    """what a launch on the null stream does under G2: it runs after the consumer has read, so the consumer sees the guard"""
    fresh = torch.arange(1024, dtype=torch.float32, device="cuda") + 1.0
    out, took = torch.full((1024,), G.FLOAT_GUARD, device="cuda"), torch.zeros(1024, device="cuda")
    torch.cuda.synchronize()
    g = G.gate(G.null_stream(), 100.0)
    with torch.cuda.stream(G.null_stream()):
        out.copy_(fresh)
    with torch.cuda.stream(stream):
        took.copy_(out)
        stream.synchronize()
    assert not g.query() and bool((took == G.FLOAT_GUARD).all())
    torch.cuda.synchronize()
    assert torch.equal(out, fresh)


# --------------------------------------------------------------------------------------- 2 and 3  the handle-free entry points

@pytest.mark.parametrize("entry", sorted(SOC.rows()))
def test_entry_point_is_ordered_on_the_callers_stream_and_only_enqueues(entry, stream):
    seen = []
    t0 = time.perf_counter()
    SOC.rows()[entry](driver(stream, seen), False)
    assert seen and set(seen) == {entry}, seen
    print("streamorder-time %s %.2f s" % (entry, time.perf_counter() - t0))


@pytest.mark.parametrize("entry", sorted(set(SOC.rows()) - set(SOC.SEAM_IS_THE_CASE) - set(SOC.SEAMLESS)))
def test_the_second_slice_of_32768_is_ordered_too(entry, stream):
    seen = []
    t0 = time.perf_counter()
    SOC.rows()[entry](driver(stream, seen), True)
    assert seen == [entry], seen
    print("streamorder-time %s past the seam %.2f s" % (entry, time.perf_counter() - t0))


@pytest.mark.parametrize("entry", SOC.WRAPPER_ROWS)
def test_python_wrapper_forwards_its_stream_and_only_enqueues(entry, stream):
    """the thin wrapper of every entry point whose wrapper takes `stream=` (the rows above make the call themselves where the wrapper
    takes every buffer): what it allocates and returns is made on torch's current stream, which is the caller's"""
    seen, recs = [], []
    SOC.wrapper_rows()[entry](driver(stream, seen, recs))
    assert seen == [entry], seen
    # The reference here is the wrapper's own synchronised run, whose work buffer is new on every call.  A pass that never got its
    # input in any run leaves the same zeros in all of them; the models hold the bits elsewhere, this holds that there are some.
    assert recs[0]["returned_all_zero"] == [], (entry, "a tensor the wrapper returned is all zeros in the synchronised run", recs[0])


# ------------------------------------------------------------------------------------------------------------ 4  handle calls

FLOW = 8192
CHAINS = {"44k1_96k_2ch": (44100, 96000, 2, {}),                 # the lean fused kernel
          "44k1_96k_3ch": (44100, 96000, 3, {}),                 # the generic fused kernel and the seam kernel
          "44k1_48k_bw99_2ch": (44100, 48000, 2, BW99),          # sub-blocked
          "96k_44k1_3ch": (96000, 44100, 3, {})}
HANDLES = [("44k1_96k_2ch", "f32"), ("44k1_96k_3ch", "f32"), ("44k1_48k_bw99_2ch", "f32"), ("96k_44k1_3ch", "f32"),
           ("44k1_96k_2ch", "f64"), ("44k1_96k_2ch", "s16")]
FORMATS = {"f32": (dict(dtype=np.float32), torch.float32), "f64": (dict(dtype=np.float64), torch.float64),
           "s16": (dict(sample_format=F.RRX_FMT_S16), torch.int16)}
# a call of the script that legitimately waits on the host would be named here, with the line that explains it: none does
HANDLE_WAITS = {}


def handle_buffers(chain, fmt, nin, nout):
    fi, fo, nch, _ = CHAINS[chain]
    tdt = FORMATS[fmt][1]
    x = np.random.default_rng([7, nch, nin]).uniform(-0.5, 0.5, (nin, 1, FLOW, nch))
    x = np.rint(x * 2.0 ** 15).astype(np.int16) if fmt == "s16" else x.astype(np.float32 if fmt == "f32" else np.float64)
    X = [torch.from_numpy(x[k]).cuda() for k in range(nin)]
    cap = FLOW * fo // fi + 4096
    Y = [torch.zeros((1, cap if k < nout - 2 else 1 << 17, nch), dtype=tdt, device="cuda") for k in range(nout)]
    return X, Y, cap


def script(r, X, Y, cap):
    """at least four flows of 8192 frames, a push and pull pair, a drain and a final pull; then a second pass with RRX_reset in
    its middle.  Returns what the calls returned."""
    ret = []
    r.reset()
    for k in range(4):
        ret.append(r.flow_device(X[k], FLOW, Y[k], cap))
    r.push_device(X[4], FLOW)
    ret.append(r.pull_device(Y[4], cap))
    r.drain()
    ret.append(r.pull_device(Y[8], 1 << 17))
    r.reset()
    ret.append(r.flow_device(X[5], FLOW, Y[5], cap))
    ret.append(r.flow_device(X[6], FLOW, Y[6], cap))
    r.reset()
    ret.append(r.flow_device(X[7], FLOW, Y[7], cap))
    r.drain()
    ret.append(r.pull_device(Y[9], 1 << 17))
    return ret


@pytest.mark.parametrize("chain,fmt", HANDLES, ids=["%s-%s" % h for h in HANDLES])
def test_handle_script_on_the_callers_stream(chain, fmt, stream):
    fi, fo, nch, kw = CHAINS[chain]
    X, Y, cap = handle_buffers(chain, fmt, 8, 10)
    # the reference: a fresh handle, the script synchronised
    ref = F.Resampler(fi, fo, nch=nch, **FORMATS[fmt][0], **kw)
    ref.set_stream(stream.cuda_stream)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        want_ret = script(ref, X, Y, cap)
        stream.synchronize()
    want = [y.clone() for y in Y]
    ref.close()
    # five flows and pushes come out in full in the first pass; of the second pass, what the flow behind the reset gives
    assert sum(v if isinstance(v, int) else v[1] for v in want_ret) > 5 * FLOW * fo // fi, want_ret
    assert all(float(want[k].float().abs().max()) > 0 for k in (8, 9)), "a drained output of the script stayed empty"
    for y in Y:
        y.zero_()
    r = F.Resampler(fi, fo, nch=nch, **FORMATS[fmt][0], **kw)
    r.set_stream(stream.cuda_stream)
    got_ret = []

    def call(s):
        got_ret[:] = script(r, X, Y, cap)
        return got_ret

    # (the driver's two synchronised runs warm the handle with the same script: the rings have their capacity under the gates)
    G.gated(call, X, Y, stream, enqueue_only=(chain, fmt) not in HANDLE_WAITS, label="handle %s %s" % (chain, fmt))
    assert got_ret == want_ret, (got_ret, want_ret)
    for k, (a, b) in enumerate(zip(Y, want)):
        assert G.same_bits(a, b), (chain, fmt, "output %d differs from the fresh handle's" % k)
    r.sync()
    r.close()


def own_stream_runs_beside_the_null_stream(r, x, y, cap, stream):
    """the queue caveat: the handle's own stream holds a hardware queue too, and may share the null stream's.  One flow on the own
    stream, joined to `stream` by the switch, while the null stream is gated: did it finish?"""
    torch.cuda.synchronize()
    g = G.gate(G.null_stream(), 80.0)
    r.use_own_stream()
    r.flow_device(x, FLOW, y, cap)
    r.set_stream(stream.cuda_stream)
    done = torch.cuda.Event()
    done.record(stream)
    t0 = time.perf_counter()
    while not done.query() and time.perf_counter() - t0 < 0.04:
        pass
    ok = bool(done.query() and not g.query())
    torch.cuda.synchronize()
    r.reset()
    return ok


def test_switching_streams_orders_the_work_on_both_sides(stream):
    """set_stream(s), flow, use_own_stream(), flow, set_stream(s), drain, pull.  The first flow sits behind G1 on s, so the flow on
    the handle's own stream must wait for it through the switch (its input is ready: the own stream cannot be gated from outside,
    and for another stream the contract asks for just that); the drain and the pull on s must wait for the own stream."""
    chain, fmt = "44k1_96k_3ch", "f32"
    fi, fo, nch, kw = CHAINS[chain]
    X, Y, cap = handle_buffers(chain, fmt, 2, 3)
    ready = X[1].clone()                             # the second flow's input: never staged, never overwritten
    torch.cuda.synchronize()

    def switch(r):
        ret = []
        r.reset()
        r.set_stream(stream.cuda_stream)
        ret.append(r.flow_device(X[0], FLOW, Y[0], cap))
        r.use_own_stream()
        ret.append(r.flow_device(ready, FLOW, Y[1], cap))
        r.set_stream(stream.cuda_stream)
        r.drain()
        ret.append(r.pull_device(Y[2], 1 << 17))
        return ret

    ref = F.Resampler(fi, fo, nch=nch, **kw)
    with torch.cuda.stream(stream):
        want_ret = switch(ref)
        stream.synchronize()
    want = [y.clone() for y in Y]
    ref.close()
    r = F.Resampler(fi, fo, nch=nch, **kw)
    r.set_stream(stream.cuda_stream)
    g2 = own_stream_runs_beside_the_null_stream(r, ready, Y[1], cap, stream)
    G.log({"what": "own stream beside the null stream", "independent": g2})
    for y in Y:
        y.zero_()
    got_ret = []

    def call(s):
        got_ret[:] = switch(r)
        return got_ret

    G.gated(call, [X[0]], Y, stream, label="handle switch %s" % chain, g2=g2)
    assert got_ret == want_ret
    for k, (a, b) in enumerate(zip(Y, want)):
        assert G.same_bits(a, b), ("switch", "output %d differs from the fresh handle's" % k)
    r.sync()
    r.close()


# ------------------------------------------------------------------------------------------------------------ 5  the side stream

def test_side_stream_seams_behind_a_gate(tmp_path):
    """tests/variant_child.py, mode side_stream_gated: the run of test_side_stream_seams_change_no_sample (seam ring of 0.01 MB, so
    that a push is several launches with a seam kernel on the side stream behind each), and the same run with the second push on
    a caller's stream behind G1, its input overwritten right behind the call.  One child; its exit status is handled as there."""
    from test_gpu_variants import run_child
    from variants import SCHEDULING
    got = run_child("side_stream_gated", {"mode": "side_stream_gated"}, SCHEDULING["side_stream"][0], tmp_path)
    for tag in ("32", "64"):
        G.log({"what": "side stream f" + tag, "t_ms": round(float(got["t_ms" + tag]), 3), "g1_ms": float(got["g1_ms" + tag]),
               "g2_ms": float(got["g2_ms" + tag]), "g1_pending_after_call": bool(got["pending" + tag]),
               "g2_used": bool(got["g2_used" + tag]), "g2_pending_at_end": bool(got["g2_pending" + tag]), "lean": int(got["lean" + tag])})
        assert int(got["lean" + tag]) >= 3
        assert np.array_equal(got["cuts" + tag], got["gcuts" + tag])
        assert got["f" + tag].shape == got["g" + tag].shape and got["f" + tag].tobytes() == got["g" + tag].tobytes()
        assert bool(got["pending" + tag]), "the push returned only when its stream's gate was over"
        assert bool(got["g2_pending" + tag]) or not bool(got["g2_used" + tag])


# --------------------------------------------------------------------------------------------------- 6  the Python conversions

TRACKS = (40, 65, 1500, 7000)
MAX_WAITS = 6


class HostWaits:
    """Which steps of a conversion make the host wait.  While the conversion runs, every Python call and return and every call of a
    builtin looks at the event behind the gate of the caller's stream: pending before a step and over behind it means the host
    waited in that step (a gate outlasts the host's own work twenty times).  A new gate of the same length is queued at once, up
    to MAX_WAITS times, so that the next wait shows too; a conversion that waits more often fails.  A step is (the function of
    ratelib.py it happened in, the builtin that waited or "-")."""

    def __init__(self, stream):
        self.stream, self.event, self.ms, self.steps = stream, None, 0.0, []

    def arm(self, event, ms):
        self.event, self.ms = event, ms
        sys.setprofile(self.look)

    def stop(self):
        sys.setprofile(None)
        self.event = None

    def look(self, frame, event, arg):
        if self.event is None or not self.event.query():
            return
        f = frame
        while f is not None and not f.f_code.co_filename.endswith("ratelib.py"):
            f = f.f_back
        who = f.f_code.co_name if f is not None else "?"
        what = getattr(arg, "__name__", "?") if event == "c_return" else "-"
        self.steps.append((who, what))
        self.event = G.gate(self.stream, self.ms) if len(self.steps) <= MAX_WAITS else None


def conversion_tracks(nch=2, fmt=torch.float32):
    rng = np.random.default_rng(66)
    return [torch.from_numpy((rng.standard_normal((n, nch)) * 0.3).astype(np.float32)).cuda() for n in TRACKS]


KW = dict(dither=True, seed=0x1234567887654321)
CONVERSIONS = {
    "convert_track_device": lambda r, tr: r.convert_track_device(tr[3][None].expand(r.nstreams, -1, -1).contiguous()),
    "convert_tracks_device": lambda r, tr: r.convert_tracks_device(tr),
    "convert_tracks_device mix": lambda r, tr: r.convert_tracks_device(tr, mix="swap"),
    "convert_tracks_to_pcm_device": lambda r, tr: r.convert_tracks_to_pcm_device(tr, F.RRX_FMT_S16, **KW),
    "convert_tracks_to_pcm_device shaped": lambda r, tr: r.convert_tracks_to_pcm_device(tr, F.RRX_FMT_S16, shaping="wannamaker9", segment=1024, **KW),
    "convert_tracks_to_pcm_loudness_limited": lambda r, tr: r.convert_tracks_to_pcm_loudness_limited(tr, F.RRX_FMT_S16, release_ms=50.0),
    "convert_tracks_to_pcm_loudness_normalized": lambda r, tr: r.convert_tracks_to_pcm_loudness_normalized(tr, F.RRX_FMT_S16),
    "convert_tracks_to_pcm_streamed": lambda r, tr: r.convert_tracks_to_pcm_streamed(tr, F.RRX_FMT_S16, window=1000, **KW),
    "convert_tracks_to_pcm_streamed_shaped": lambda r, tr: r.convert_tracks_to_pcm_streamed_shaped(tr, F.RRX_FMT_S16, "wannamaker9", segment=1024,
                                                                                                   window=1000, seed=KW["seed"]),
    "convert_library_to_pcm": lambda r, tr: r.convert_library_to_pcm(tr, F.RRX_FMT_S16, window=None, **KW),
    "convert_library_to_pcm window": lambda r, tr: r.convert_library_to_pcm(tr, F.RRX_FMT_S16, window=1000, **KW),
}
# The steps at which each conversion makes the host wait, in order (DESIGN.md 12 has the table).  Both are uploads from pageable
# host memory, which the host sees through: the plan's table (TracksPlan.to_device: torch's .to of a host tensor) once a batch, and
# in the library forms the batch's track indices in front of it (torch.tensor(idx, device=) in _convert_library; two batches here).
# convert_track_device has no table and never waits; no conversion reads a measured value back, the loudness forms included.
UPLOAD, INDEX = ("to_device", "to"), ("_convert_library", "tensor")
HOST_WAITS = {name: [UPLOAD] for name in CONVERSIONS}
HOST_WAITS["convert_track_device"] = []
HOST_WAITS["convert_library_to_pcm"] = HOST_WAITS["convert_library_to_pcm window"] = [INDEX, UPLOAD, INDEX, UPLOAD]


def own_stream_switches_beside_the_null_stream(r, stream):
    """the queue caveat for a conversion: it takes a handle from its own stream to torch's current one and back, and the switch
    records an event on the stream it leaves, for the stream it enters to wait on.  Where the own stream shares the null
    stream's hardware queue, that event lies behind the null stream's gate, and the caller's stream with it.  One switch beside a
    gated null stream: did the caller's stream get on?"""
    torch.cuda.synchronize()
    g = G.gate(G.null_stream(), 80.0)
    r.set_stream(stream.cuda_stream)
    done = torch.cuda.Event()
    done.record(stream)
    t0 = time.perf_counter()
    while not done.query() and time.perf_counter() - t0 < 0.04:
        pass
    ok = bool(done.query() and not g.query())
    torch.cuda.synchronize()
    r.use_own_stream()
    torch.cuda.synchronize()
    return ok


@pytest.mark.parametrize("own", [False, True], ids=["handle on s", "handle on its own stream"])
@pytest.mark.parametrize("name", list(CONVERSIONS))
def test_conversion_runs_on_torchs_current_stream(name, own, stream):
    """Both gates, and the table of host waits, with the handle already on s: the conversion then touches no stream but s, and G2
    holds whatever hardware queue the handle's own stream has.  Then the way a caller who never called set_stream has it, the
    handle on its own stream and switched to s and back by the conversion: under G2 where the switch gets on beside a gated null
    stream (asked of the handle first, and printed), under G1 and the overwrite alone where it does not.  In both forms the
    caller's stream is gated again behind every host wait, so that what follows an upload does not run on an idle stream."""
    library = name.startswith("convert_library")
    r = F.Resampler(44100, 48000, nch=2, nstreams=2 if library else len(TRACKS))
    tracks = conversion_tracks()
    watch = HostWaits(stream)
    if own:
        g2 = own_stream_switches_beside_the_null_stream(r, stream)
        G.log({"what": "own stream switch beside the null stream", "label": name, "independent": g2})
    else:
        r.set_stream(stream.cuda_stream)
        torch.cuda.synchronize()
        g2 = True

    def call(s):
        assert torch.cuda.current_stream() == s
        r.reset()
        try:
            return CONVERSIONS[name](r, tracks)
        finally:
            watch.stop()

    try:
        G.gated(call, tracks, [], stream, enqueue_only=False, label=name + (", own stream" if own else ""), g2=g2, watch=watch.arm,
                rearms=MAX_WAITS)
    finally:
        watch.stop()
        print("streamorder-waits %s %r" % (name, watch.steps))
    assert len(watch.steps) <= MAX_WAITS, (name, "more host waits than the gates were made for", watch.steps)
    if own:
        assert r._stream is None, "the handle was not given its own stream back"
    else:
        assert r._stream == stream.cuda_stream, "the handle was not left on the caller's stream"
    assert watch.steps == HOST_WAITS[name], (name, "the host waited at other steps than the table names", watch.steps)
    r.sync()
    r.close()


