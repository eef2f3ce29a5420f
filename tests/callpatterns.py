"""The two call patterns the fp64 parity tests drive a handle with (tests/test_gpu_fp64_parity.py in its own process,
tests/variant_child.py in a child per knob setting): device flow in chunks on torch's stream, and host push / pull_all.
Both profile every call and return the kernel names next to the output.  GPU only."""
import numpy as np

import foo_dsp_resampler_amd as F

_FMT = {np.dtype(np.float32): F.RRX_FMT_FLOAT, np.dtype(np.float64): F.RRX_FMT_DOUBLE}


def run_flow(fi, fo, nch, S, kw, x, dtype=np.float64):
    """x: [S, n, nch] of `dtype`.  Device flow on torch's stream, drain, pull: (y [S, m, nch] of `dtype`, kernel names)."""
    import torch
    dtype = np.dtype(dtype)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    n = x.shape[1]
    chunk = 16384 if n <= 48000 else 1 << 17
    r = F.Resampler(fi, fo, nch=nch, nstreams=S, dtype=dtype, **kw)
    assert r.format == _FMT[dtype]
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    r.profile(True)
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()
    cap = int(chunk * fo / fi) + 8192
    parts, names = [], set()
    for s0 in range(0, n, chunk):
        k = min(chunk, n - s0)
        xin = xd[:, s0:s0 + k].contiguous()
        y = torch.zeros((S, cap, nch), dtype=tdt, device="cuda")
        iu, og = r.flow_device(xin, k, y, cap)
        assert iu == k
        parts.append(y[:, :og].cpu().numpy())
        names |= {k_["kernel"] for k_ in r.profile_report()}
    r.drain()
    tcap = int(n * fo / fi) + 16
    tail = torch.zeros((S, tcap, nch), dtype=tdt, device="cuda")
    og = r.pull_device(tail, tcap)
    parts.append(tail[:, :og].cpu().numpy())
    r.sync()
    names |= {k_["kernel"] for k_ in r.profile_report()}
    assert r.available == 0
    r.close()
    return np.concatenate(parts, axis=1), names


def run_push(fi, fo, nch, kw, x, chunk=4096, dtype=np.float64):
    """x: [n, nch] of `dtype`.  Host push / pull_all, drain: (y [m, nch] of `dtype`, kernel names)."""
    dtype = np.dtype(dtype)
    r = F.Resampler(fi, fo, nch=nch, dtype=dtype, **kw)
    assert r.format == _FMT[dtype]
    r.profile(True)
    parts, names = [], set()
    for s0 in range(0, x.shape[0], chunk):
        r.push(x[s0:s0 + chunk])
        parts.append(r.pull_all())
        names |= {k_["kernel"] for k_ in r.profile_report()}
    r.drain()
    parts.append(r.pull_all())
    names |= {k_["kernel"] for k_ in r.profile_report()}
    r.close()
    return np.concatenate(parts), names
