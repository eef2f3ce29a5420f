"""The device LPC edge extrapolator (RRX_lpc_extrapolate_device) against what a caller with device-resident tracks had to do
without it: copy every stream's base frames to the host, run the serial per-channel host extrapolator there (the test
harness's orc_lpc_extrapolate, the restatement of lpc/lpc.cpp), copy the extrapolated frames back.

Shapes: 256 and 1024 streams x 2 channels, data_len = 2205, 2205 frames extrapolated both ways (44100 -> 48000: edge_geometry).
One JSON line per shape, appended to --out (default profiles/lpc_device_perf.jsonl) and printed:

  {"streams", "nch", "data_len", "extra", "order", "device_ms": median, "device_ms_min", "device_ms_max", "device_reps",
   "host_roundtrip_ms": median, "host_ms_min", "host_ms_max", "host_reps", "host_parts_ms": {"d2h", "lpc", "h2d"},
   "speedup": host / device, "bit_equal": the two results agree bit for bit}

device_ms: HIP events on the stream around ONE call (all streams), after --warmup calls.  host_roundtrip_ms: host clock from the
start of the device-to-host copy to the completion of the host-to-device copy (both synchronous), one thread.  Nothing is
asserted about the times.

  python tools/perf_lpc.py [--streams 256,1024] [--reps 50] [--warmup 5] [--host-reps 3] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import foo_dsp_resampler_amd as F  # noqa: E402
from oracle_binding import lib as oracle_lib  # noqa: E402
from test_plugin_layer import music_like  # noqa: E402

NCH, N, EXTRA, ORDER = 2, 2205, 2205, 32


def one_shape(S, reps, warmup, host_reps):
    fn = oracle_lib().orc_lpc_extrapolate
    fn.argtypes, fn.restype = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_size_t, C.c_size_t], None
    frames = EXTRA + N + EXTRA
    base = np.stack([music_like(N, NCH, 44100, 1000 + s) for s in range(min(S, 16))])
    base = np.ascontiguousarray(np.tile(base, ((S + 15) // 16, 1, 1))[:S] * np.linspace(0.5, 1.0, S, dtype=np.float32)[:, None, None])
    buf = np.zeros((S, frames, NCH), np.float32)
    buf[:, EXTRA:EXTRA + N] = base
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t = torch.from_numpy(buf).cuda()
        for _ in range(warmup):
            F.lpc_extrapolate_device(t, EXTRA, N, EXTRA, EXTRA, order=ORDER, stream=stream)
        dev = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            F.lpc_extrapolate_device(t, EXTRA, N, EXTRA, EXTRA, order=ORDER, stream=stream)
            e1.record(stream)
            e1.synchronize()
            dev.append(e0.elapsed_time(e1))
        got = t.cpu().numpy()

        # the host round trip, on a second device buffer holding the same base frames
        u = torch.from_numpy(buf).cuda()
        stream.synchronize()
        host, parts = [], []
        for _ in range(host_reps):
            t0 = time.perf_counter()
            h = np.zeros((S, frames, NCH), np.float32)
            h[:, EXTRA:EXTRA + N] = u[:, EXTRA:EXTRA + N].cpu().numpy()          # D2H of the base frames
            t1 = time.perf_counter()
            for s in range(S):
                fn(h[s].ctypes.data + EXTRA * NCH * 4, N, NCH, ORDER, EXTRA, EXTRA)
            t2 = time.perf_counter()
            u[:, :EXTRA] = torch.from_numpy(h[:, :EXTRA]).cuda()                   # H2D of the two extrapolated edges
            u[:, EXTRA + N:] = torch.from_numpy(h[:, EXTRA + N:]).cuda()
            stream.synchronize()
            t3 = time.perf_counter()
            host.append((t3 - t0) * 1e3)
            parts.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
        want = u.cpu().numpy()
    k = host.index(statistics.median_low(host))
    return {"streams": S, "nch": NCH, "data_len": N, "extra": EXTRA, "order": ORDER,
            "device_ms": round(statistics.median(dev), 4), "device_ms_min": round(min(dev), 4), "device_ms_max": round(max(dev), 4),
            "device_reps": reps, "host_roundtrip_ms": round(host[k], 2), "host_ms_min": round(min(host), 2),
            "host_ms_max": round(max(host), 2), "host_reps": host_reps,
            "host_parts_ms": dict(zip(("d2h", "lpc", "h2d"), [round(v, 2) for v in parts[k]])),
            "speedup": round(host[k] / statistics.median(dev), 1),
            "bit_equal": bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="256,1024")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpc_device_perf.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_lpc.py needs a GPU: there is nothing to time without one")
    for S in [int(v) for v in a.streams.split(",")]:
        line = json.dumps(one_shape(S, a.reps, a.warmup, a.host_reps))
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
