"""The true-peak pass (RRX_true_peak_device: gain, 4x oversampling by the BS.1770 filter, true peak and sample peak in ONE pass)
against the measure-only output stage on the same bytes and against what a caller with float32 frames in HBM writes in torch today:

    w = coefs.view(4, 1, 12).flip(2)                                      # conv1d correlates: flip the taps
    y = conv1d(pad(x.double().permute(0, 2, 1).reshape(S * nch, 1, frames), (11, 11)), w)
    true_peak = y.abs().amax((1, 2)).view(S, nch)

Input: the output tensor of one bench.py step (RRX_flow_device of isamp_max frames, LCG noise) of BASELINE configs 1 (256 streams
x 2 channels, 44.1k -> 96k) and 3 (16 streams x 32 channels, 96k -> 44.1k), float32, as tools/perf_finish.py makes it.  Everything
runs on the same tensor in the same process, `--rounds` rounds (default 3) interleaved: in every round each candidate is warmed
up `--warmup` times and then timed over `--steps` calls between two HIP events on the stream.  The timed calls accumulate into
the same result arrays: from the second call on no peak rises, so the kernels skip their global atomics, as in perf_finish.py.
The torch sequence fuses its multiply-adds and sums in another order, so its number agrees with the call's to rounding, not to
the bit; the line records the largest relative difference.

One JSON line per shape, appended to --out (default profiles/true_peak_perf.jsonl) and printed:

  {"config", "streams", "nch", "frames", "ms": median of the rounds, "ms_rounds", "gsamples_per_s", "measure_only_ms",
   "measure_only_ms_rounds", "ratio_to_measure_only": ms / measure_only_ms, "torch_ms", "torch_ms_rounds", "speedup_vs_torch":
   torch_ms / ms, "max_rel_diff_vs_torch", "steps", "warmup"}

Exit status 1 if the call is not faster than the torch sequence on a shape.

  python tools/perf_true_peak.py [--configs 1,3] [--steps 20] [--warmup 3] [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import foo_dsp_resampler_amd as F  # noqa: E402
from perf_finish import step_tensor, timed  # noqa: E402


def one_config(k, steps, warmup, rounds):
    stream = torch.cuda.Stream()
    x, _ = step_tensor(k, stream)
    S, frames, nch = x.shape
    phases, taps, coefs = F.TRUE_PEAK_FILTERS["bs1770"]
    with torch.cuda.stream(stream):
        tp = torch.zeros((S, nch), dtype=torch.float64, device="cuda")
        pk = torch.zeros((S, nch), dtype=torch.float64, device="cuda")
        pk2 = torch.zeros((S, nch), dtype=torch.float64, device="cuda")
        cl = torch.zeros((S, nch), dtype=torch.int64, device="cuda")
        w = torch.tensor(coefs, dtype=torch.float64, device="cuda").view(phases, 1, taps).flip(2).contiguous()
    stream.synchronize()

    def call():
        return F.true_peak_device(x, true_peak=tp, peak=pk, stream=stream)

    def measure_only():
        return F.finish_device(x, None, peak=pk2, clipped=cl, stream=stream)

    def torch_sequence():
        xs = torch.nn.functional.pad(x.double().permute(0, 2, 1).reshape(S * nch, 1, frames), (taps - 1, taps - 1))
        return torch.nn.functional.conv1d(xs, w).abs().amax((1, 2)).view(S, nch)

    ms, mms, tms = [], [], []
    for _ in range(rounds):
        ms.append(timed(stream, call, steps, warmup))
        mms.append(timed(stream, measure_only, steps, warmup))
        tms.append(timed(stream, torch_sequence, steps, warmup))
    with torch.cuda.stream(stream):
        ref = torch_sequence()
        rel = float(((tp - ref).abs() / ref).max())
    stream.synchronize()
    m, mo, t = statistics.median(ms), statistics.median(mms), statistics.median(tms)
    return {"config": k, "streams": S, "nch": nch, "frames": frames, "ms": round(m, 4), "ms_rounds": [round(v, 4) for v in ms],
            "gsamples_per_s": round(S * frames * nch / m / 1e6, 2), "measure_only_ms": round(mo, 4),
            "measure_only_ms_rounds": [round(v, 4) for v in mms], "ratio_to_measure_only": round(m / mo, 2), "torch_ms": round(t, 4),
            "torch_ms_rounds": [round(v, 4) for v in tms], "speedup_vs_torch": round(t / m, 2), "max_rel_diff_vs_torch": rel,
            "steps": steps, "warmup": warmup}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="1,3")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "true_peak_perf.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_true_peak.py needs a GPU: there is nothing to time without one")
    slower = []
    for k in [int(v) for v in a.configs.split(",")]:
        line = one_config(k, a.steps, a.warmup, a.rounds)
        text = json.dumps(line)
        print(text, flush=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")
        if not line["ms"] < line["torch_ms"]:
            slower.append(k)
    if slower:
        raise SystemExit("not faster than the torch sequence on configs %r" % (slower,))


if __name__ == "__main__":
    main()
