"""The loudness pass (RRX_loudness_device: K-weighted hop energies by block decomposition, three launches) against two yardsticks
that exist without it, on the same bytes in the same process: the measure-only output stage, finish_device(x, None) -- one read of
the tensor, the HBM floor -- and true_peak_device(x).

Input: the output tensor of one bench.py step of BASELINE configs 1 (256 streams x 2 channels, 44.1k -> 96k) and 3 (16 streams x
32 channels, 96k -> 44.1k), float32, as tools/perf_finish.py makes it; the hop is a tenth of a second of the output rate.
`--rounds` rounds (default 3) interleaved: in every round each candidate is warmed up `--warmup` times and then timed over
`--steps` calls between two HIP events on the stream.  The energy, work and result buffers are allocated once.  The gate
(RRX_loudness_gate_device) is timed beside it; it reads the energies only.

The condition the line reports as `held`: the three launches together take no longer than twice true_peak_device.  The carry
launch alone is serial in the hops and cannot be timed between events from outside the call; its time comes from a kernel trace
of this tool (rocprofv3 --kernel-trace --stats -- python tools/perf_loudness.py --rounds 1), loudness_carry_kernel's row.

One JSON line per shape, appended to --out (default profiles/loudness_perf.jsonl) and printed:

  {"config", "streams", "nch", "frames", "hop", "hops", "ms": median of the rounds, "ms_rounds", "gsamples_per_s",
   "measure_only_ms", "measure_only_ms_rounds", "ratio_to_measure_only", "true_peak_ms", "true_peak_ms_rounds",
   "ratio_to_true_peak": ms / true_peak_ms, "held": ms <= 2 * true_peak_ms, "gate_ms", "lufs_first_stream", "steps", "warmup"}

  python tools/perf_loudness.py [--configs 1,3] [--steps 20] [--warmup 3] [--rounds 3] [--out FILE]
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

import bench  # noqa: E402
import foo_dsp_resampler_amd as F  # noqa: E402
from perf_finish import step_tensor, timed  # noqa: E402


def one_config(k, steps, warmup, rounds):
    stream = torch.cuda.Stream()
    x, _ = step_tensor(k, stream)
    S, frames, nch = x.shape
    rate = bench.CONFIGS[k]["fo"]
    hop = rate // 10
    n = frames // hop
    with torch.cuda.stream(stream):
        energy = torch.zeros((S, nch, n), dtype=torch.float64, device="cuda")
        work = torch.empty((F.lib().RRX_loudness_work_doubles(S, nch, frames, hop),), dtype=torch.float64, device="cuda")
        tp = torch.zeros((S, nch), dtype=torch.float64, device="cuda")
        pk = torch.zeros((S, nch), dtype=torch.float64, device="cuda")
        pk2 = torch.zeros((S, nch), dtype=torch.float64, device="cuda")
        cl = torch.zeros((S, nch), dtype=torch.int64, device="cuda")
    stream.synchronize()

    def call():
        return F.loudness_device(x, rate, energy=energy, work=work, stream=stream)

    def gate():
        return F.loudness_gate_device(energy, hop, stream=stream)

    def measure_only():
        return F.finish_device(x, None, peak=pk2, clipped=cl, stream=stream)

    def true_peak():
        return F.true_peak_device(x, true_peak=tp, peak=pk, stream=stream)

    ms, mms, tms, gms = [], [], [], []
    for _ in range(rounds):
        ms.append(timed(stream, call, steps, warmup))
        mms.append(timed(stream, measure_only, steps, warmup))
        tms.append(timed(stream, true_peak, steps, warmup))
        gms.append(timed(stream, gate, steps, warmup))
    with torch.cuda.stream(stream):
        lufs = float(F.integrated_lufs(gate())[0])
    stream.synchronize()
    m, mo, t = statistics.median(ms), statistics.median(mms), statistics.median(tms)
    return {"config": k, "streams": S, "nch": nch, "frames": frames, "hop": hop, "hops": n, "ms": round(m, 4), "ms_rounds": [round(v, 4) for v in ms],
            "gsamples_per_s": round(S * frames * nch / m / 1e6, 2), "measure_only_ms": round(mo, 4),
            "measure_only_ms_rounds": [round(v, 4) for v in mms], "ratio_to_measure_only": round(m / mo, 2), "true_peak_ms": round(t, 4),
            "true_peak_ms_rounds": [round(v, 4) for v in tms], "ratio_to_true_peak": round(m / t, 3), "held": bool(m <= 2 * t),
            "gate_ms": round(statistics.median(gms), 4), "lufs_first_stream": round(lufs, 3), "steps": steps, "warmup": warmup}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="1,3")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loudness_perf.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_loudness.py needs a GPU: there is nothing to time without one")
    for k in [int(v) for v in a.configs.split(",")]:
        line = one_config(k, a.steps, a.warmup, a.rounds)
        text = json.dumps(line)
        print(text, flush=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
