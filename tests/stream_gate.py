"""Gates: what the stream-order tests share (tests/test_gpu_stream_order.py; DESIGN.md 12, "Stream order").  Needs a GPU.

Every *_device call of include/ratelib_amd.h promises that all of its work is queued on the caller's stream and that the call
only enqueues.  On an idle, synchronised GPU neither promise can fail: a launch sent to another stream still finds its inputs
ready, and a host wait inside the call is over at once.  A gate removes the idle GPU.  It is a kernel that keeps ONE stream busy
for a chosen time (torch.cuda._sleep, calibrated once per process); the tests are deterministic and catch no race.

  G1, in front of the inputs, on the caller's stream s:  gate, copy every buffer of the call from staging tensors (until this
      copy runs they hold stale values), the call, an event query, clones of the outputs, stale values over the inputs and a guard
      over the outputs, synchronise s, compare the clones.  A launch on any other stream runs while s sleeps and reads stale
      inputs; work left on an unjoined internal stream is overtaken by the overwrite; a host wait inside the call outlasts G1.
  G2, on the null stream, queued first, waited on by nothing:  correct code never touches the null stream and finishes on s while
      it sleeps; a launch sent there runs after the clones were taken.  G2 must still be pending when s has finished, which
      shows that the case kept its power and that the call never synchronised the device.

Stale values are valid inputs, zeros throughout: samples of +0.0, gains of 0.0, states of zeros, tables of zero-length tracks.  A
violation shows as wrong bits, never as an access out of range.  The reference of a gated run is the same call made the old way,
synchronised, on the same buffers; the bar is equality of bits.

Gate lengths are apparatus, not a tolerance.  With t the host time of the synchronised run (call plus synchronise), G1 lasts
max(100 ms, 20 t) and G2 outlasts it by the same amount, capped at 3 s; the assertions are the two pending events.  Every case
prints a line "streamorder {json}" with t and both lengths.

Hardware queues.  A process opens a few hardware queues and its streams share them; work on a stream that shares the null
stream's queue lies behind G2, an event record included.  independent_stream() finds a caller's stream that does not.  A handle's
own stream and side stream hold queues too, so a case that lets a handle touch them asks first whether they get on beside a gated
null stream and counts G2 only then (which queue a handle's streams get depends on how many streams the process made before)."""
import gc
import json
import os
import time

import torch

G1_MIN_MS = 100.0
G2_CAP_MS = 3000.0
FLOAT_GUARD = 777.25
INT_GUARD = 0x5A

_cycles_per_ms = None
_independent = None
records = []                      # one dict per gated case and per calibration, in the order they ran


def log(rec):
    """print the record; with STREAM_ORDER_JSONL in the environment, append it to that file too (how profiles/stream_order.jsonl
    is written)"""
    records.append(rec)
    print("streamorder " + json.dumps(rec))
    path = os.environ.get("STREAM_ORDER_JSONL")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")


def null_stream():
    s = torch.cuda.default_stream()
    assert s.cuda_stream == 0, "torch's default stream is not the null stream here"
    return s


def calibrate():
    """cycles of torch.cuda._sleep per millisecond, measured once per process behind a warm-up call: _sleep(10^7) between two
    timing events.  The rate of the device is not assumed."""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            torch.cuda._sleep(10 ** 6)
            s.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            torch.cuda._sleep(10 ** 7)
            e1.record(s)
            s.synchronize()
        ms = e0.elapsed_time(e1)
        assert ms > 0.05, "torch.cuda._sleep(10^7) took %.4f ms: it is no gate on this device" % ms
        _cycles_per_ms = 10 ** 7 / ms
        log({"what": "calibration", "sleep_cycles": 10 ** 7, "ms": round(ms, 4), "cycles_per_ms": round(_cycles_per_ms, 1)})
    return _cycles_per_ms


def gate(stream, ms):
    """keep `stream` busy for `ms` milliseconds from where its queue stands; returns an event recorded behind the gate"""
    cycles = int(calibrate() * ms)
    e = torch.cuda.Event()
    with torch.cuda.stream(stream):
        while cycles > 0:                            # (one launch takes a 32-bit signed count on some builds)
            torch.cuda._sleep(min(cycles, 2 ** 31 - 1))
            cycles -= 2 ** 31 - 1
        e.record(stream)
    return e


def independent_stream():
    """a fresh torch stream (non-blocking) that runs while the null stream is gated.  Streams beyond the hardware queues of the
    process share one, and a stream that shares the null stream's would make G2 fail falsely; up to eight are tried, and it is a
    failure, not a skip, when none runs."""
    global _independent
    if _independent is None:
        x = torch.zeros(16, device="cuda")
        torch.cuda.synchronize()
        tried = []
        for _ in range(8):
            c = torch.cuda.Stream()
            g = gate(null_stream(), 60.0)
            done = torch.cuda.Event()
            with torch.cuda.stream(c):
                x.add_(1.0)
                done.record(c)
            t0 = time.perf_counter()
            while not done.query() and time.perf_counter() - t0 < 0.03:
                pass
            ok = done.query() and not g.query()
            tried.append(bool(ok))
            torch.cuda.synchronize()
            if ok:
                _independent = c
                break
        log({"what": "independent_stream", "tried": tried})
        assert _independent is not None, "none of eight fresh streams ran while the null stream was gated: %r" % (tried,)
    return _independent


def stale_(t):
    """the stale value of an input: zeros, which every input of the library takes (module docstring)"""
    t.zero_()


def guard_(t):
    """the guard over an output, behind its clone"""
    t.fill_(FLOAT_GUARD if t.dtype.is_floating_point else INT_GUARD)


def stale_cache(stream):
    """zeros over every block that torch's allocator holds free for `stream`.  A call that makes its temporaries with torch.empty
    gets, in the gated run, the very blocks its synchronised run gave back, still holding that run's content -- right values
    that would hide a launch that came too late to write them."""
    with torch.cuda.stream(stream):
        held = []
        for seg in torch.cuda.memory_snapshot():
            if seg.get("stream", stream.cuda_stream) != stream.cuda_stream:
                continue
            for b in seg["blocks"]:
                if b["state"] == "inactive" and b["size"] > 0:
                    held.append(torch.empty((b["size"],), dtype=torch.uint8, device="cuda"))
        for t in held:
            t.zero_()
        del held


def same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _tensors(ret):
    """(the tensors in what a call returned, everything else) -- lists and tuples are walked"""
    ts, rest = [], []

    def walk(v):
        if isinstance(v, torch.Tensor):
            ts.append(v)
            rest.append(("tensor", tuple(v.shape), str(v.dtype)))
        elif isinstance(v, (list, tuple)):
            rest.append(len(v))
            for w in v:
                walk(w)
        else:
            rest.append(v)

    walk(ret)
    return ts, rest


def gated(call, inputs, outputs, stream, enqueue_only=True, scratch=(), label="", g2=True, watch=None, rearms=0):
    """The sequence of the module docstring around call(stream), which enqueues on `stream` and may return tensors it made (they
    count as outputs) and plain values (which must be the synchronised run's).

    `inputs`: device tensors the call reads only, holding their values now.  `outputs`: device tensors it writes or accumulates
    into, holding now what they start from (guards and non-trivial statistics: they are staged behind G1 like the inputs).
    `scratch`: work buffers, whose content after a call is unspecified: they are not compared.  The passes of a call hand their
    intermediates on through them, and the synchronised runs leave the right ones behind, which a pass that came too late
    would find; so they are zeroed before the gated run like the inputs, and again with the overwrite behind the call.
    `enqueue_only`: the call must return with G1 pending.  False where a host wait is legitimate, and then named by the caller.
    `g2`: gate the null stream and require it pending at the end.
    `watch(event, ms)`: called with the G1 event and its length before the call, by a caller who watches the event for host waits
    and queues up to `rearms` further gates of that length on `stream` while the call runs; G2 then outlasts those too.

    Asserts: enqueue only; outputs, returned tensors and returned values equal the synchronised run's, bit for bit; inputs unchanged
    before the overwrite; G2 pending.  Leaves inputs and outputs as the gated call left them, and returns the record it printed."""
    null = null_stream()
    # A handle or tensor that an earlier test left to the garbage collector must not be freed under the gates: RR_close and
    # hipFree wait for the whole device, the null stream's gate included, and the case would fail for it.
    gc.collect()
    everything = list(inputs) + list(outputs)
    staging = [t.clone() for t in everything]
    took = [torch.empty_like(t) for t in everything]

    def sync_run():
        with torch.cuda.stream(stream):
            for t, s in zip(everything, staging):
                t.copy_(s)
            stream.synchronize()
            t0 = time.perf_counter()
            ret = call(stream)
            stream.synchronize()
            dt = time.perf_counter() - t0
            ts, rest = _tensors(ret)
            return dt, [t.clone() for t in everything], [t.clone() for t in ts], rest

    torch.cuda.synchronize()
    _, first, first_ret, first_rest = sync_run()     # warm: code objects, allocator, rings
    t, ref, ref_ret, ref_rest = sync_run()
    repeatable = first_rest == ref_rest and all(same_bits(a, b) for a, b in zip(first + first_ret, ref + ref_ret))
    del first, first_ret
    for k in range(len(inputs)):
        assert same_bits(ref[k], staging[k]), (label, "input %d was written by the synchronised run" % k)
    t_ms = t * 1e3
    g1_ms = max(G1_MIN_MS, 20.0 * t_ms)
    g2_ms = min(G2_CAP_MS, (2.0 + rearms) * g1_ms)
    assert (1.0 + rearms) * g1_ms + 5.0 * t_ms < g2_ms or not g2, (label, "the case is too slow for a null-stream gate of 3 s", t_ms)

    stale_cache(stream)
    with torch.cuda.stream(stream):
        for t_ in list(inputs) + list(scratch):
            stale_(t_)
        for t_ in outputs:
            guard_(t_)
    torch.cuda.synchronize()
    collecting = gc.isenabled()
    gc.disable()
    try:
        e2 = gate(null, g2_ms) if g2 else None
        with torch.cuda.stream(stream):
            e1 = gate(stream, g1_ms)
            for t_, s in zip(everything, staging):
                t_.copy_(s)
            if watch is not None:
                watch(e1, g1_ms)
            ret = call(stream)
            pending = not e1.query()
            ts, rest = _tensors(ret)
            for t_, c in zip(everything, took):
                c.copy_(t_)
            got_ret = [t_.clone() for t_ in ts]
            for t_ in list(inputs) + list(scratch):
                stale_(t_)
            for t_ in outputs:
                guard_(t_)
            for t_ in ts:
                guard_(t_)
            stream.synchronize()
        g2_pending = (not e2.query()) if g2 else None
    finally:
        if collecting:
            gc.enable()
    rec = {"what": "case", "label": label, "t_ms": round(t_ms, 3), "g1_ms": round(g1_ms, 1), "g2_ms": round(g2_ms, 1) if g2 else None,
           "g1_pending_after_call": pending, "g2_pending_at_end": g2_pending, "enqueue_only": bool(enqueue_only)}
    log(rec)
    with torch.cuda.stream(stream):
        for t_, c in zip(everything, took):
            t_.copy_(c)
        stream.synchronize()
    torch.cuda.synchronize()                         # G2 runs out here: the next case starts on an idle device
    if enqueue_only:
        assert pending, (label, "the call returned only when its stream's gate was over: it waited on the host", rec)
    assert rest == ref_rest, (label, "returned values", rest, ref_rest)
    for k, (c, r) in enumerate(zip(took, ref)):
        kind = "input" if k < len(inputs) else "output"
        assert same_bits(c, r), (label, "%s %d differs from the synchronised run" % (kind, k - (0 if k < len(inputs) else len(inputs))), rec)
    assert len(got_ret) == len(ref_ret) and all(same_bits(a, b) for a, b in zip(got_ret, ref_ret)), (label, "returned tensors differ", rec)
    if g2:
        assert g2_pending, (label, "the null stream's gate was over when the caller's stream had finished", rec)
    # (asked last: what the gates see is the better account of a call whose synchronised runs already differ)
    assert repeatable, (label, "two synchronised runs differ: the reference is not deterministic")
    rec["returned_all_zero"] = [k for k, t_ in enumerate(ref_ret) if t_.dtype.is_floating_point and t_.numel() and not bool(t_.any())]
    return rec
