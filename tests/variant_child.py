"""Child program of tests/test_gpu_variants.py: python variant_child.py JOB.json OUT.npz (not a test; needs a GPU).

The library reads its knobs once per process (csrc/knobs.hpp), so every knob setting runs in a process of its own.  This
program sets no environment: the parent starts it with the row's variables (tests/variants.py, child_env).

JOB.json: {"mode": "cases", "cases": [rows in the shape of chain_ld.CASES]} | {"mode": "side_stream"} | {"mode": "slabs"}.
  cases        every case on lcg_noise(frames, nch * S, 4242) -- the input of chain_ld.reference -- through a float32 and a
               float64 handle, both profiled, with the call patterns of tests/callpatterns.py (16384-frame device flows or
               4096-frame host pushes, drain, pull: the generic kernels see blocks that straddle ring and caller buffer).
               OUT.npz: "<case>/f32", "<case>/f64" [S, m, nch], "<case>/names32", "<case>/names64", "<case>/seconds".
  side_stream  44.1k -> 96k, 2 streams x 2 channels, two flow_device pushes of SIDE_FRAMES frames (the first one profiled,
               which keeps its seam kernels on the main stream; the second one not), drain, pull.
               OUT.npz: "f32", "f64" [S, m, nch] (both pushes and the drain), "cuts32", "cuts64" (frames out per call),
               "lean32", "lean64" (launches of the lean fused kernel in the profiled push).
  side_stream_gated  side_stream, and the same run with its second push on a caller's stream behind a gate and its input
               overwritten behind the call (tests/test_gpu_stream_order.py).  OUT.npz: side_stream's, and "g32", "g64", "gcuts32",
               "gcuts64" of the gated run with "t_ms*", "g1_ms*", "g2_ms*", "pending*", "g2_used*", "g2_pending*".
  slabs        192k -> 44.1k 2 ch, one host push of SLAB_FRAMES frames then a drain, and 44.1k -> 192k at a 99 % passband
               3 ch, one push of 48 000 frames then a drain.  OUT.npz: "a/f32", "a/f64", "b/f32", "b/f64" [m, nch],
               "a/half32", "a/half64" (launches of half_kernel in the push).
"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

SEED = 4242
SIDE = (44100, 96000, 2, 2)  # in_rate, out_rate, channels, streams
SIDE_FRAMES = 330000
SLAB_A = (192000, 44100, {}, 100000, 2)  # in_rate, out_rate, options, frames, channels
SLAB_B = (44100, 192000, {"bandwidth": 99.0}, 48000, 3)


def case_input(frames, nch, S):
    """(x float32 [frames, nch * S] as chain_ld.reference has it, the same as [S, frames, nch])."""
    from oracle_binding import lcg_noise
    x = lcg_noise(frames, nch * S, SEED).reshape(frames, nch * S)
    return x, np.ascontiguousarray(x.reshape(frames, S, nch).transpose(1, 0, 2))


def side_input():
    from oracle_binding import lcg_noise
    _, _, nch, S = SIDE
    return np.stack([lcg_noise(2 * SIDE_FRAMES, nch, SEED + s).reshape(-1, nch) for s in range(S)])


def slab_input(frames, nch):
    from oracle_binding import lcg_noise
    return lcg_noise(frames, nch, SEED).reshape(frames, nch)


def run_cases(cases):
    if any(c[7] == "flow" for c in cases):
        import torch  # noqa: F401  (before the library opens its first handle: imported behind one, torch took 10 s to start)
    from callpatterns import run_flow, run_push
    out = {}
    for cid, fi, fo, kw, frames, nch, S, api in cases:
        _, xs = case_input(frames, nch, S)
        t0 = time.time()
        for tag, dt in (("32", np.float32), ("64", np.float64)):
            if api == "flow":
                y, names = run_flow(fi, fo, nch, S, kw, xs.astype(dt), dtype=dt)
            else:
                assert S == 1
                y, names = run_push(fi, fo, nch, kw, xs[0].astype(dt), dtype=dt)
                y = y[None]
            assert y.dtype == dt
            out["%s/f%s" % (cid, tag)] = y
            out["%s/names%s" % (cid, tag)] = np.array(sorted(names))
        out[cid + "/seconds"] = np.array(time.time() - t0)
    return out


def run_side_stream():
    import torch
    import foo_dsp_resampler_amd as F
    fi, fo, nch, S = SIDE
    n = SIDE_FRAMES
    x = side_input()
    out = {}
    for tag, dt, tdt in (("32", np.float32, torch.float32), ("64", np.float64, torch.float64)):
        r = F.Resampler(fi, fo, nch=nch, nstreams=S, dtype=dt)
        r.set_stream(torch.cuda.current_stream().cuda_stream)
        xd = torch.from_numpy(x.astype(dt)).cuda()
        cap = int(n * fo / fi) + 65536
        parts, cuts = [], []
        for k in range(2):
            r.profile(k == 0)
            y = torch.zeros((S, cap, nch), dtype=tdt, device="cuda")
            xin = xd[:, k * n:(k + 1) * n].contiguous()
            torch.cuda.synchronize()
            iu, og = r.flow_device(xin, n, y, cap)
            assert iu == n
            if k == 0:
                out["lean" + tag] = np.array(max([rec["launches"] for rec in r.profile_report() if "fused_fast" in rec["kernel"]] or [0]))
            parts.append(y[:, :og])
            cuts.append(og)
        r.drain()
        tail = torch.zeros((S, 65536, nch), dtype=tdt, device="cuda")
        torch.cuda.synchronize()
        og = r.pull_device(tail, 65536)
        r.sync()
        assert r.available == 0
        parts.append(tail[:, :og])
        cuts.append(og)
        out["f" + tag] = torch.cat(parts, dim=1).cpu().numpy()
        out["cuts" + tag] = np.array(cuts)
        r.close()
    return out


def run_side_stream_gated():
    """run_side_stream, and the same calls with the second push made on a caller's stream behind a gate (tests/stream_gate.py):
    the input of that push is copied into its buffer behind the gate, and the buffer is overwritten with stale values right
    behind the call, so that a seam kernel of the side stream that is not ordered against the caller's stream reads stale input
    or is overtaken.  A second gate keeps the null stream busy; it counts where the handle's side stream runs beside it.  What run_side_stream
    gives, and "g32", "g64", "gcuts32", "gcuts64" of the gated run with its times, gate lengths and pending events."""
    import torch
    import foo_dsp_resampler_amd as F
    import stream_gate as G
    out = run_side_stream()
    fi, fo, nch, S = SIDE
    n = SIDE_FRAMES
    x = side_input()
    s = G.independent_stream()
    for tag, dt, tdt in (("32", np.float32, torch.float32), ("64", np.float64, torch.float64)):
        r = F.Resampler(fi, fo, nch=nch, nstreams=S, dtype=dt)
        r.set_stream(s.cuda_stream)
        xd = torch.from_numpy(x.astype(dt)).cuda()
        cap = int(n * fo / fi) + 65536
        ys = [torch.zeros((S, cap, nch), dtype=tdt, device="cuda") for _ in range(2)]
        tail = torch.zeros((S, 65536, nch), dtype=tdt, device="cuda")
        first, staged = xd[:, :n].contiguous(), xd[:, n:].contiguous()
        xin = torch.zeros_like(staged)
        torch.cuda.synchronize()
        r.profile(True)
        t0 = time.perf_counter()
        iu, og0 = r.flow_device(first, n, ys[0], cap)
        s.synchronize()
        t_ms = (time.perf_counter() - t0) * 1e3
        assert iu == n
        r.profile_report()
        r.profile(False)
        g1_ms = max(G.G1_MIN_MS, 20.0 * t_ms)
        g2_ms = min(G.G2_CAP_MS, 2.0 * g1_ms)
        e2 = G.gate(G.null_stream(), g2_ms)
        with torch.cuda.stream(s):
            e1 = G.gate(s, g1_ms)
            xin.copy_(staged)
            iu, og1 = r.flow_device(xin, n, ys[1], cap)
            pending = not e1.query()
            second = ys[1][:, :og1].clone()          # the consumer reads right behind the call, and the producer overwrites
            xin.zero_()
            ys[1].fill_(G.FLOAT_GUARD)
            r.drain()
            og2 = r.pull_device(tail, 65536)
            parts = [ys[0][:, :og0].clone(), second, tail[:, :og2].clone()]
            tail.fill_(G.FLOAT_GUARD)
            s.synchronize()
        g2_pending = not e2.query()
        torch.cuda.synchronize()
        assert iu == n and r.available == 0
        # Could the null stream's gate be asked for?  The side stream holds a hardware queue too, which it may share with the null
        # stream, and then its seam kernels wait for that gate.  Asked of this very handle, behind everything that is compared:
        # the same two pushes on the reset handle, the second one beside a gated null stream.
        r.reset()
        r.flow_device(first, n, ys[0], cap)
        s.synchronize()
        g = G.gate(G.null_stream(), g1_ms)
        r.flow_device(staged, n, ys[1], cap)
        s.synchronize()
        g2_used = not g.query()
        torch.cuda.synchronize()
        out["g" + tag] = torch.cat(parts, dim=1).cpu().numpy()
        out["gcuts" + tag] = np.array([og0, og1, og2])
        for k, v in (("t_ms", t_ms), ("g1_ms", g1_ms), ("g2_ms", g2_ms), ("pending", pending), ("g2_used", g2_used), ("g2_pending", g2_pending)):
            out[k + tag] = np.array(v)
        r.close()
    return out


def run_slabs():
    import foo_dsp_resampler_amd as F
    out = {}
    for key, (fi, fo, kw, frames, nch) in (("a", SLAB_A), ("b", SLAB_B)):
        x = slab_input(frames, nch)
        for tag, dt in (("32", np.float32), ("64", np.float64)):
            r = F.Resampler(fi, fo, nch=nch, dtype=dt, **kw)
            r.profile(True)
            r.push(x.astype(dt))
            first = r.pull_all()
            out["%s/half%s" % (key, tag)] = np.array(max([rec["launches"] for rec in r.profile_report() if "half_kernel" in rec["kernel"]] or [0]))
            r.drain()
            out["%s/f%s" % (key, tag)] = np.concatenate([first, r.pull_all()])
            r.close()
    return out


def main(argv):
    with open(argv[1]) as f:
        job = json.load(f)
    out = {"cases": lambda: run_cases(job["cases"]), "side_stream": run_side_stream, "side_stream_gated": run_side_stream_gated,
           "slabs": run_slabs}[job["mode"]]()
    np.savez(argv[2], **out)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
