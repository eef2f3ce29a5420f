"""The device output stage (RRX_finish_device: gain, TPDF dither, PCM quantisation, peak, clip count in ONE pass) against what a
caller with float32 frames in HBM writes in torch today for the dither-off case:

    q = (x.double() * g * 2**bits).round().clamp(lo, hi).to(dtype);  peak = x.abs().amax(1)

Input: the output tensor of one bench.py step (RRX_flow_device of isamp_max frames, LCG noise) of BASELINE configs 1 (256 streams
x 2 channels, 44.1k -> 96k) and 3 (16 streams x 32 channels, 96k -> 44.1k), float32, with a per-stream gain.  Four variants of
the call per shape -- S16 without and with dither, packed S24 without, measure only -- and the torch sequence for S16, for 24
bits (into int32: torch has no packed form, so this yardstick writes a byte a sample more and packs nothing) and for the peak
alone.  Everything runs on the same tensor in the same process, `--rounds` rounds (default 3) interleaved: in every round each
candidate is warmed up `--warmup` times and then timed over `--steps` calls between two HIP events on the stream.  The same
session times the bench step itself (flow_device, as bench.py does), so a line can say what the pass adds to a step.
The timed calls all accumulate into the same peak / clipped arrays: from the second call on no peak rises, so the kernel skips its
peak atomics (it issues one only when a workgroup beats the stored value).  The times are those of the later chunks of a track; a
first call into zeroed arrays adds up to one atomic maximum per (workgroup, channel), about 33 000 on config 1.

One JSON line per (shape, variant), appended to --out (default profiles/finish_perf.jsonl) and printed:

  {"config", "streams", "nch", "frames", "variant", "ms": median of the rounds, "ms_rounds", "bytes": read + written by the
   algorithm (4 B a sample in, 2 / 3 / 0 out), "gbs", "hbm_share": gbs / 8000 (the HBM peak bench.py uses), "torch_ms",
   "torch_ms_rounds", "speedup_vs_torch": torch_ms / ms, "dither_on_over_off" (S16 with dither only), "bench_step_ms",
   "share_of_bench_step": ms / bench_step_ms, "steps", "warmup"}

Exit status 1 if a dither-off variant is not faster than its torch sequence.

  python tools/perf_finish.py [--configs 1,3] [--steps 20] [--warmup 3] [--rounds 3] [--out FILE]

--shaped times the noise-shaped call instead (RRX_finish_shaped_device; DESIGN.md 10, "Noise-shaped dither") on the same two
tensors: S16, dither on, the wannamaker9 filter, segments 4096 / 16384 / 65536 / 0, interleaved in every round with the unshaped
dithered RRX_finish_device and with the copy of the float32 tensor into pinned host memory -- what any host-side shaper would have
to begin with.  One JSON line per (shape, segment), appended to --out (default profiles/finish_shaped_perf.jsonl):

  {"config", "streams", "nch", "frames", "variant": "shaped_s16_dither", "filter", "segment", "lanes": (stream, segment, channel)
   chains, "ms", "ms_rounds", "ns_per_frame_of_a_chain": ms / the frames of the longest chain, "unshaped_ms", "unshaped_ms_rounds",
   "ratio_to_unshaped", "to_pinned_host_ms", "to_pinned_host_ms_rounds", "faster_than_the_copy", "steps", "warmup"}

Exit status 1 if, at the default segment (65536), the shaped call is not faster than the copy.  --shaped-once CONFIG runs nothing
but `--steps` shaped calls at the default segment on that config's tensor: the process to collect hardware counters from.

  python tools/perf_finish.py --shaped [--configs 1,3] [--steps 20] [--warmup 3] [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
import foo_dsp_resampler_amd as F  # noqa: E402

HBM_PEAK_GBS = bench.HBM_PEAK_GBS


def timed(stream, fn, steps, warmup):
    """ms per call: `steps` calls between two events on `stream`, after `warmup` calls"""
    with torch.cuda.stream(stream):
        for _ in range(warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(steps):
            fn()
        e1.record(stream)
        e1.synchronize()
    return e0.elapsed_time(e1) / steps


def torch_quantise(x, g, bits, dtype):
    q = (x.double() * g * 2.0 ** bits).round().clamp(-2.0 ** bits, 2.0 ** bits - 1).to(dtype)
    return q, x.abs().amax(1)


def one_config(k, steps, warmup, rounds):
    cfg = bench.CONFIGS[k]
    fi, fo, nch, S = cfg["fi"], cfg["fo"], cfg["nch"], cfg["streams"]
    stream = torch.cuda.Stream()
    r = F.Resampler(fi, fo, nch=nch, nstreams=S, **cfg["kw"])
    P = r.isamp_max
    xin = bench.lcg_noise_device(torch, S, P, nch, 12345, "cuda")
    cap = int(P * fo / fi) + 65536
    y = torch.empty((S, cap, nch), device="cuda", dtype=torch.float32)
    torch.cuda.synchronize()
    r.set_stream(stream.cuda_stream)
    og = [0]

    def bench_step():
        og[0] = r.flow_device(xin, P, y, cap)[1]

    step_ms = [timed(stream, bench_step, steps, warmup)]
    with torch.cuda.stream(stream):
        x = y[:, :og[0]].contiguous()        # the frames of the last step: what a caller would hand to the output stage
        g = torch.linspace(0.5, 1.0, S, dtype=torch.float64, device="cuda")
        g3 = g[:, None, None]
        out16 = torch.empty(x.shape, dtype=torch.int16, device="cuda")
        out24 = torch.empty(x.shape[:2] + (nch * 3,), dtype=torch.uint8, device="cuda")
        peak = torch.zeros((S, nch), dtype=torch.float64, device="cuda")
        clipped = torch.zeros((S, nch), dtype=torch.int64, device="cuda")
    stream.synchronize()
    frames = x.shape[1]

    def call(fmt, out, dither):
        return lambda: F.finish_device(x, fmt, gain=g, dither=dither, seed=1, out=out, peak=peak, clipped=clipped, stream=stream)

    cand = {
        "s16": (call(F.RRX_FMT_S16, out16, False), 2, lambda: torch_quantise(x, g3, 15, torch.int16)),
        "s16_dither": (call(F.RRX_FMT_S16, out16, True), 2, None),
        "s24_3": (call(F.RRX_FMT_S24_3, out24, False), 3, lambda: torch_quantise(x, g3, 23, torch.int32)),
        "measure_only": (call(None, None, False), 0, lambda: x.abs().amax(1)),
    }
    ms = {v: [] for v in cand}
    tms = {v: [] for v in cand}
    for _ in range(rounds):
        for v, (fn, _, ref) in cand.items():
            ms[v].append(timed(stream, fn, steps, warmup))
            if ref is not None:
                tms[v].append(timed(stream, ref, steps, warmup))
        step_ms.append(timed(stream, bench_step, steps, warmup))
    # the results agree where they can be compared: the S16 bits, and the peak of |x * g| against g * the peak of |x|
    with torch.cuda.stream(stream):
        peak.zero_()
        cand["s16"][0]()
        q, pk = cand["s16"][2]()
        agree = bool(torch.equal(q, out16)) and bool(torch.allclose(peak, pk.double() * g[:, None], rtol=1e-15, atol=0))
    stream.synchronize()
    bench_ms = statistics.median(step_ms)
    lines = []
    for v, (_, nb, ref) in cand.items():
        m = statistics.median(ms[v])
        nbytes = S * frames * nch * (4 + nb)
        line = {"config": k, "streams": S, "nch": nch, "frames": frames, "variant": v, "ms": round(m, 4),
                "ms_rounds": [round(t, 4) for t in ms[v]], "bytes": nbytes, "gbs": round(nbytes / m / 1e6, 1),
                "hbm_share": round(nbytes / m / 1e6 / HBM_PEAK_GBS, 4)}
        if ref is not None:
            t = statistics.median(tms[v])
            line.update({"torch_ms": round(t, 4), "torch_ms_rounds": [round(u, 4) for u in tms[v]], "speedup_vs_torch": round(t / m, 2)})
        if v == "s16_dither":
            line["dither_on_over_off"] = round(m / statistics.median(ms["s16"]), 3)
        if v == "s16":
            line["bits_equal_torch"] = agree
        line.update({"bench_step_ms": round(bench_ms, 4), "share_of_bench_step": round(m / bench_ms, 4), "steps": steps, "warmup": warmup})
        lines.append(line)
    r.use_own_stream()
    return lines


SHAPED_SEGMENTS = (4096, 16384, 65536, 0)
SHAPED_DEFAULT = 65536


def step_tensor(k, stream):
    """the frames of one bench.py step of config k, as one_config makes them, and the per-stream gain"""
    cfg = bench.CONFIGS[k]
    fi, fo, nch, S = cfg["fi"], cfg["fo"], cfg["nch"], cfg["streams"]
    r = F.Resampler(fi, fo, nch=nch, nstreams=S, **cfg["kw"])
    P = r.isamp_max
    xin = bench.lcg_noise_device(torch, S, P, nch, 12345, "cuda")
    cap = int(P * fo / fi) + 65536
    y = torch.empty((S, cap, nch), device="cuda", dtype=torch.float32)
    torch.cuda.synchronize()
    r.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        got = r.flow_device(xin, P, y, cap)[1]
        x = y[:, :got].contiguous()
        g = torch.linspace(0.5, 1.0, S, dtype=torch.float64, device="cuda")
    stream.synchronize()
    r.use_own_stream()
    return x, g


def shaped_config(k, steps, warmup, rounds, segments=SHAPED_SEGMENTS, only=False):
    stream = torch.cuda.Stream()
    x, g = step_tensor(k, stream)
    S, frames, nch = x.shape
    with torch.cuda.stream(stream):
        out16 = torch.empty(x.shape, dtype=torch.int16, device="cuda")
        peak = torch.zeros((S, nch), dtype=torch.float64, device="cuda")
        clipped = torch.zeros((S, nch), dtype=torch.int64, device="cuda")
    stream.synchronize()

    def shaped(segment):
        return lambda: F.finish_shaped_device(x, F.RRX_FMT_S16, "wannamaker9", segment, gain=g, dither=True, seed=1, out=out16, peak=peak,
                                              clipped=clipped, stream=stream)

    if only:
        timed(stream, shaped(SHAPED_DEFAULT), steps, warmup)
        return []
    host = torch.empty(x.shape, dtype=torch.float32, pin_memory=True)
    unshaped = lambda: F.finish_device(x, F.RRX_FMT_S16, gain=g, dither=True, seed=1, out=out16, peak=peak, clipped=clipped, stream=stream)  # noqa: E731
    copy = lambda: host.copy_(x, non_blocking=True)  # noqa: E731
    ms = {seg: [] for seg in segments}
    ums, cms = [], []
    for _ in range(rounds):
        for seg in segments:
            ms[seg].append(timed(stream, shaped(seg), steps, warmup))
            ums.append(timed(stream, unshaped, steps, warmup))
        cms.append(timed(stream, copy, steps, warmup))
    u, c = statistics.median(ums), statistics.median(cms)
    lines = []
    for seg in segments:
        m = statistics.median(ms[seg])
        nseg = -(-frames // seg) if seg else 1
        lines.append({"config": k, "streams": S, "nch": nch, "frames": frames, "variant": "shaped_s16_dither", "filter": "wannamaker9",
                      "segment": seg, "lanes": S * nseg * nch, "ms": round(m, 4), "ms_rounds": [round(t, 4) for t in ms[seg]],
                      "ns_per_frame_of_a_chain": round(m * 1e6 / (seg if seg and seg < frames else frames), 2),
                      "unshaped_ms": round(u, 4), "unshaped_ms_rounds": [round(t, 4) for t in ums], "ratio_to_unshaped": round(m / u, 2),
                      "to_pinned_host_ms": round(c, 4), "to_pinned_host_ms_rounds": [round(t, 4) for t in cms],
                      "faster_than_the_copy": bool(m < c), "steps": steps, "warmup": warmup})
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shaped", action="store_true")
    ap.add_argument("--shaped-once", type=int, default=None, metavar="CONFIG")
    ap.add_argument("--configs", default="1,3")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "finish_shaped_perf.jsonl" if a.shaped else "finish_perf.jsonl")
    if not torch.cuda.is_available():
        raise SystemExit("perf_finish.py needs a GPU: there is nothing to time without one")
    if a.shaped_once is not None:
        shaped_config(a.shaped_once, a.steps, a.warmup, 1, only=True)
        return
    if a.shaped:
        late = []
        for k in [int(v) for v in a.configs.split(",")]:
            for line in shaped_config(k, a.steps, a.warmup, a.rounds):
                text = json.dumps(line)
                print(text, flush=True)
                with open(a.out, "a") as f:
                    f.write(text + "\n")
                if line["segment"] == SHAPED_DEFAULT and not line["faster_than_the_copy"]:
                    late.append((k, line["ms"], line["to_pinned_host_ms"]))
        if late:
            raise SystemExit("at the default segment not faster than the copy to pinned host memory: %r" % (late,))
        return
    slower = []
    for k in [int(v) for v in a.configs.split(",")]:
        for line in one_config(k, a.steps, a.warmup, a.rounds):
            text = json.dumps(line)
            print(text, flush=True)
            with open(a.out, "a") as f:
                f.write(text + "\n")
            if line["variant"] in ("s16", "s24_3") and not line["ms"] < line["torch_ms"]:
                slower.append((k, line["variant"]))
    if slower:
        raise SystemExit("slower than the torch sequence: %r" % (slower,))


if __name__ == "__main__":
    main()
