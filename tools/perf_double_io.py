"""Float32 against float64 frames on each BASELINE config's bench shape (bench.py: streams, frames per push, flow_device
into a preallocated buffer on a stream of ours), both formats in the same process.  One JSON line per config:

  {"config": K, "float": {"msamples_s", "kernel_ms", "hot_kernel_ms", "bytes_per_unit"}, "double": {...}, "ratio": double/float}

Msamples/s counts input channel-samples per second of wall time over the timed steps (bench.py's "value"); kernel_ms is the
summed stage-kernel time of one profiled pass of the same steps (RRX_profile_read), per step; bytes_per_unit is the
algorithmic traffic per input channel-sample: 4 (1 + out/in) for float frames, 8 (1 + out/in) for double frames.

  python tools/perf_double_io.py [--configs 0,1,2,3,4] [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import foo_dsp_resampler_amd as F  # noqa: E402


def measure(cfg, dtype, steps, warmup):
    fi, fo, nch, kw = cfg["fi"], cfg["fo"], cfg["nch"], cfg["kw"]
    S = cfg["streams"]
    r = F.Resampler(fi, fo, nch=nch, nstreams=S, dtype=dtype, **kw)
    P = min(cfg.get("frames") or r.isamp_max, r.isamp_max)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    x = bench.lcg_noise_device(torch, S, P, nch, 12345, "cuda").to(tdt)
    cap = int(P * fo / fi) + 65536
    y = torch.empty((S, cap, nch), device="cuda", dtype=tdt)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    r.set_stream(stream.cuda_stream)

    def step():
        iu, og = r.flow_device(x, P, y, cap)
        assert iu == P
        return og

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    r.sync()
    elapsed = time.perf_counter() - t0
    r.profile(True)
    for _ in range(steps):
        step()
    prof = r.profile_read()
    r.profile(False)
    r.close()
    esz = 8 if dtype == np.float64 else 4
    return {"msamples_s": round(S * P * nch * steps / elapsed / 1e6, 1),
            "kernel_ms": round((prof["hot_ms"] + prof["other_ms"]) / steps, 4), "hot_kernel_ms": round(prof["hot_ms"] / steps, 4),
            "bytes_per_unit": round(esz * (1.0 + fo / fi), 4), "streams": S, "frames": P}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="0,1,2,3,4")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    for k in [int(c) for c in a.configs.split(",")]:
        cfg = bench.CONFIGS[k]
        f = measure(cfg, np.float32, a.steps, a.warmup)
        d = measure(cfg, np.float64, a.steps, a.warmup)
        print(json.dumps({"config": k, "float": f, "double": d, "ratio": round(d["msamples_s"] / f["msamples_s"], 3)}), flush=True)


if __name__ == "__main__":
    main()
