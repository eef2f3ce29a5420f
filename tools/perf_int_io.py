"""Float32 against 16- and 32-bit integer PCM frames on each BASELINE config's bench shape (bench.py: streams, frames per push,
flow_device into a preallocated buffer on a stream of ours), all three formats in the same process.  One JSON line per config:

  {"config": K, "float": {"msamples_s", "kernel_ms", "hot_kernel_ms", "bytes_per_unit", "kernels"}, "s16": {...}, "s32": {...},
   "ratio_s16": s16/float, "ratio_s32": s32/float}

Msamples/s counts input channel-samples per second of wall time over the timed steps (bench.py's "value"), best of --rounds
rounds interleaved over the formats; kernel_ms is the summed stage-kernel time of one profiled pass of the same steps, per step,
"kernels" the same per kernel instance (RRX_profile_report); bytes_per_unit is the algorithmic traffic per input
channel-sample: esz (1 + out/in) with esz = 4 / 2 / 4 bytes.

  python tools/perf_int_io.py [--configs 0,1,2,3,4] [--steps 20] [--warmup 5] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import bench  # noqa: E402
import foo_dsp_resampler_amd as F  # noqa: E402

FORMATS = {"float": (F.RRX_FMT_FLOAT, torch.float32, 4), "s16": (F.RRX_FMT_S16, torch.int16, 2), "s32": (F.RRX_FMT_S32, torch.int32, 4)}


class Run:
    def __init__(self, cfg, name):
        fmt, self.tdt, self.esz = FORMATS[name]
        self.cfg, self.S = cfg, cfg["streams"]
        fi, fo, nch = cfg["fi"], cfg["fo"], cfg["nch"]
        self.r = F.Resampler(fi, fo, nch=nch, nstreams=self.S, sample_format=fmt, **cfg["kw"])
        self.P = P = min(cfg.get("frames") or self.r.isamp_max, self.r.isamp_max)
        x = bench.lcg_noise_device(torch, self.S, P, nch, 12345, "cuda")  # float32 in [-0.5, 0.5)
        if name == "s16":
            x = torch.round(x.double() * 32768.0).to(torch.int16)
        elif name == "s32":
            x = torch.round(x.double() * 2147483648.0).to(torch.int32)
        self.x = x.contiguous()
        self.cap = int(P * fo / fi) + 65536
        self.y = torch.empty((self.S, self.cap, nch), device="cuda", dtype=self.tdt)
        torch.cuda.synchronize()
        self.stream = torch.cuda.Stream()
        self.r.set_stream(self.stream.cuda_stream)
        self.best = 0.0

    def step(self):
        iu, og = self.r.flow_device(self.x, self.P, self.y, self.cap)
        assert iu == self.P
        return og

    def timed(self, steps, warmup):
        for _ in range(warmup):
            self.step()
        self.r.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step()
        self.r.sync()
        elapsed = time.perf_counter() - t0
        self.best = max(self.best, self.S * self.P * self.cfg["nch"] * steps / elapsed / 1e6)

    def finish(self, steps):
        self.r.profile(True)
        for _ in range(steps):
            self.step()
        rep = self.r.profile_report()
        self.r.profile(False)
        self.r.close()
        fi, fo = self.cfg["fi"], self.cfg["fo"]
        return {"msamples_s": round(self.best, 1), "kernel_ms": round(sum(k["ms"] for k in rep) / steps, 4),
                "hot_kernel_ms": round(sum(k["ms"] for k in rep if k["hot"]) / steps, 4),
                "kernels": {k["kernel"].replace("rsmp::", ""): round(k["ms"] / steps, 4) for k in rep},
                "bytes_per_unit": round(self.esz * (1.0 + fo / fi), 4), "streams": self.S, "frames": self.P}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="0,1,2,3,4")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    for k in [int(c) for c in a.configs.split(",")]:
        runs = {name: Run(bench.CONFIGS[k], name) for name in FORMATS}
        for _ in range(a.rounds):  # interleaved: float, s16, s32, float, ...
            for name in FORMATS:
                runs[name].timed(a.steps, a.warmup)
        out = {name: runs[name].finish(a.steps) for name in FORMATS}
        line = {"config": k}
        line.update(out)
        line["ratio_s16"] = round(out["s16"]["msamples_s"] / out["float"]["msamples_s"], 3)
        line["ratio_s32"] = round(out["s32"]["msamples_s"] / out["float"]["msamples_s"], 3)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
