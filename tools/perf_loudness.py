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

--meter times the loudness meter on top of the energies instead (meter_rows below): one JSON line per input and grouping, appended
to profiles/loudness_stats_perf.jsonl.

  python tools/perf_loudness.py --meter [--steps 20] [--warmup 3] [--rounds 3] [--out FILE]
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


def meter_rows(steps, warmup, rounds):
    """--meter: the five calls of the loudness meter (RRX_loudness_blocks_device three times: (4, 1) with every output, (30, 1) for
    the maximum alone, (30, 10) with blocks and counts; RRX_loudness_gate_groups_device on the (4, 1) blocks;
    RRX_loudness_range_groups_device on the (30, 10) blocks) through the C ABI on buffers allocated once, on two inputs: "a", the
    energies of config 1's bench tensor, and "b", synthetic energies of 256 x 2 x 3000 hops (five-minute tracks); each with every
    stream as its own group and with all streams in one.  On "a" RRX_loudness_device's three launches are timed in the same
    rounds, and `held` says that the five calls together take no longer.  `gate_no_blocks_ms` / `range_no_blocks_ms` are the same
    calls with every block count zero -- the launches and the walks over the streams, without the walks over the blocks -- so
    `gate_block_walk_share` is the share of the per-stream serial sums in the gate, and `range_block_walk_share` that of the
    selection passes (and the one serial stage in front of them) in the range call."""
    import ctypes as C
    stream = torch.cuda.Stream()
    x, _ = step_tensor(1, stream)
    S, frames, nch = x.shape
    rate = bench.CONFIGS[1]["fo"]
    hop = rate // 10
    with torch.cuda.stream(stream):
        energy_a = torch.zeros((S, nch, frames // hop), dtype=torch.float64, device="cuda")
        work_a = torch.empty((F.lib().RRX_loudness_work_doubles(S, nch, frames, hop),), dtype=torch.float64, device="cuda")
        F.loudness_device(x, rate, energy=energy_a, work=work_a, stream=stream)
        gen = torch.Generator(device="cuda").manual_seed(1770)
        energy_b = torch.rand((S, nch, 3000), generator=gen, dtype=torch.float64, device="cuda") * hop * 0.02  # about -20 LUFS, 10 dB of spread
        energy_b *= 10.0 ** (-torch.rand((S, 1, 3000), generator=gen, dtype=torch.float64, device="cuda"))
    stream.synchronize()
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    L, sp = F.lib(), C.c_void_p(stream.cuda_stream)
    rows = []
    for name, energy in (("a", energy_a), ("b", energy_b)):
        nh = energy.shape[2]
        with torch.cuda.stream(stream):
            b4 = torch.zeros((S, nh - 3), dtype=torch.float64, device="cuda")
            b30 = torch.zeros((S, (nh - 30) // 10 + 1), dtype=torch.float64, device="cuda")
            n4, n30, none = (torch.zeros((S,), dtype=torch.int64, device="cuda") for _ in range(3))
            m4, m30 = (torch.zeros((S,), dtype=torch.float64, device="cuda") for _ in range(2))
            res = torch.zeros((S, 4), dtype=torch.float64, device="cuda")
            gwork = torch.empty((L.RRX_loudness_groups_work_doubles(S, S),), dtype=torch.float64, device="cuda")
            grouping = {"own": (torch.arange(S, dtype=torch.int32, device="cuda"), S), "one": (torch.zeros((S,), dtype=torch.int32, device="cuda"), 1)}
        stream.synchronize()
        a_thr, a_rel = F.loudness_gate(-70.0, -10.0)
        r_thr, r_rel = F.loudness_gate(-70.0, -20.0)

        def blocks(Lh, P, b, n, m):
            rc = L.RRX_loudness_blocks_device(-1, sp, vp(energy), nh, S, nch, nh, None, None, hop, Lh, P, vp(b) if b is not None else None,
                                              b.shape[1] if b is not None else 0, vp(n) if n is not None else None, vp(m) if m is not None else None)
            assert rc == 0

        def gate(group, ngroups, counts):
            assert L.RRX_loudness_gate_groups_device(-1, sp, vp(b4), b4.shape[1], S, vp(counts), vp(group), ngroups, a_thr, a_rel, vp(res), vp(gwork),
                                                     gwork.numel()) == 0

        def rng(group, ngroups, counts):
            assert L.RRX_loudness_range_groups_device(-1, sp, vp(b30), b30.shape[1], S, vp(counts), vp(group), ngroups, r_thr, r_rel, 10, 95, vp(res),
                                                      vp(gwork), gwork.numel()) == 0

        def loudness():
            return F.loudness_device(x, rate, energy=energy_a, work=work_a, stream=stream)

        for which, (group, ngroups) in grouping.items():
            calls = {"blocks_4_1_ms": lambda: blocks(4, 1, b4, n4, m4), "blocks_30_1_ms": lambda: blocks(30, 1, None, None, m30),
                     "blocks_30_10_ms": lambda: blocks(30, 10, b30, n30, None), "gate_ms": lambda: gate(group, ngroups, n4),
                     "range_ms": lambda: rng(group, ngroups, n30), "gate_no_blocks_ms": lambda: gate(group, ngroups, none),
                     "range_no_blocks_ms": lambda: rng(group, ngroups, none)}
            if name == "a":
                calls["loudness_ms"] = loudness
            ms = {k: [] for k in calls}
            for _ in range(rounds):
                for k, fn in calls.items():
                    ms[k].append(timed(stream, fn, steps, warmup))
            med = {k: statistics.median(v) for k, v in ms.items()}
            total = sum(med[k] for k in ("blocks_4_1_ms", "blocks_30_1_ms", "blocks_30_10_ms", "gate_ms", "range_ms"))
            with torch.cuda.stream(stream):
                gate(group, ngroups, n4)
                lufs = float(F.integrated_lufs(res[:ngroups])[0])
                rng(group, ngroups, n30)
                lra = float(F.loudness_range_lu(res[:ngroups])[0])
            stream.synchronize()
            row = {"meter": name, "streams": S, "nch": nch, "hops": nh, "groups": which}
            row.update({k: round(v, 4) for k, v in med.items()})
            row.update({"meter_ms": round(total, 4), "meter_ms_rounds": [round(sum(ms[k][i] for k in ("blocks_4_1_ms", "blocks_30_1_ms", "blocks_30_10_ms",
                                                                                                      "gate_ms", "range_ms")), 4) for i in range(rounds)],
                        "gate_block_walk_share": round(1.0 - med["gate_no_blocks_ms"] / med["gate_ms"], 3),
                        "range_block_walk_share": round(1.0 - med["range_no_blocks_ms"] / med["range_ms"], 3),
                        "lufs_first_group": round(lufs, 3), "lra_first_group": round(lra, 3), "steps": steps, "warmup": warmup})
            if name == "a":
                row["held"] = bool(total <= med["loudness_ms"])
            rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meter", action="store_true", help="time the loudness meter's calls instead (profiles/loudness_stats_perf.jsonl)")
    ap.add_argument("--configs", default="1,3")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "loudness_stats_perf.jsonl" if a.meter else "loudness_perf.jsonl")
    if not torch.cuda.is_available():
        raise SystemExit("perf_loudness.py needs a GPU: there is nothing to time without one")
    for line in meter_rows(a.steps, a.warmup, a.rounds) if a.meter else (one_config(k, a.steps, a.warmup, a.rounds) for k in [int(v) for v in a.configs.split(",")]):
        text = json.dumps(line)
        print(text, flush=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
