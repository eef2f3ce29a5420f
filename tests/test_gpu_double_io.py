"""Float64 sample buffers (RRX_FMT_DOUBLE handles, RRX_*_double calls) on the GPU.

A double handle runs the float handle's chain -- same stage kernels, same geometry, same fp64 arithmetic -- with float64
frames at both ends.  So its output rounded to float32 must equal the float handle's output bit for bit, its fp64 output
must match the oracle's fp64 output fifo far below one float32 ulp, and input detail below float32 resolution must reach
the output."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import foo_dsp_resampler_amd as F
from oracle_binding import Oracle, lcg_noise

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RR_INVPARAM = 6
BW99 = {"bandwidth": 99.0}

# the lean kernels' float64-frame instances carry their own names; every other kernel is the same instance for both formats
DIO_NAMES = {"rsmp::fused_fast_kernel<": "rsmp::fused_fast_dio_kernel<", "rsmp::fused_split_kernel<": "rsmp::fused_split_dio_kernel<",
             "rsmp::fused_split2_kernel<": "rsmp::fused_split2_dio_kernel<"}


def dio_name(k):
    for a, b in DIO_NAMES.items():
        if k.startswith(a):
            return b + k[len(a):]
    return k


def noise(S, n, nch, seed):
    return np.stack([lcg_noise(n, nch, seed + s).reshape(n, nch) for s in range(S)])


def run_device(fi, fo, nch, S, kw, x, dtype, api="flow", chunk=16384):
    """x: [S, n, nch] host array.  Device path on torch's stream; returns (y [S, m, nch] in dtype, kernel names)."""
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    r = F.Resampler(fi, fo, nch=nch, nstreams=S, dtype=dtype, **kw)
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    r.profile(True)
    n = x.shape[1]
    xd = torch.from_numpy(np.ascontiguousarray(x.astype(dtype))).cuda()
    parts = []
    cap = int(chunk * fo / fi) + 8192
    for s0 in range(0, n, chunk):
        k = min(chunk, n - s0)
        xin = xd[:, s0:s0 + k].contiguous()
        y = torch.zeros((S, cap, nch), dtype=tdt, device="cuda")
        if api == "flow":
            iu, og = r.flow_device(xin, k, y, cap)
            assert iu == k
        else:
            r.push_device(xin, k)
            og = r.pull_device(y, cap)
        parts.append(y[:, :og].cpu().numpy())
    r.drain()
    tail = torch.zeros((S, 1 << 17, nch), dtype=tdt, device="cuda")
    og = r.pull_device(tail, 1 << 17)
    parts.append(tail[:, :og].cpu().numpy())
    r.sync()
    names = sorted({k["kernel"] for k in r.profile_report()})
    r.close()
    return np.concatenate(parts, axis=1), names


CASES = [  # (fi, fo, nch, streams, kw, api)
    (44100, 48000, 2, 1, {}, "flow"),                  # BASELINE configs 0 / 4
    (44100, 96000, 2, 1, {}, "flow"),                  # configs 1 (lean kernel)
    (44100, 192000, 8, 1, BW99, "flow"),               # configs 2: fused_split_kernel<9, 1> + dftx_kernel<4>
    (96000, 44100, 32, 1, {}, "flow"),                 # configs 3
    (44100, 48000, 2, 1, BW99, "flow"),                # sub-blocked kernel, OMODE 0 (outputs into the caller's buffer)
    (44100, 48000, 2, 1, BW99, "pushpull"),            # ... OMODE 2 (outputs through the fifo)
    (96000, 44100, 2, 1, BW99, "flow"),                # dft_kernel<13, 13, 13> + polymf
    (44100, 48000, 2, 1, {"bandwidth": 99.7}, "flow"),  # 65536-point blocks: dftbig
    (44100, 48001, 2, 1, {}, "flow"),                  # polyi
    (44100, 11025, 2, 1, {}, "flow"),                  # power-of-two ratio: half-band stages
    (44100, 48000, 2, 1, {"quality": F.RR_NORM}, "flow"),
    (44100, 96000, 2, 1, {"phase": 0.0}, "flow"),
    (44100, 48000, 2, 1, {"phase": 100.0}, "pushpull"),
    (44100, 96000, 1, 1, {}, "flow"),
    (44100, 48000, 3, 1, {}, "flow"),
    (44100, 96000, 5, 1, {}, "pushpull"),
    (44100, 96000, 2, 3, {}, "flow"),
    (44100, 48000, 3, 2, {}, "flow"),
]


@pytest.mark.parametrize("fi,fo,nch,S,kw,api", CASES)
def test_same_arithmetic_wider_ends(fi, fo, nch, S, kw, api):
    x = noise(S, 60000, nch, 17 + nch)
    yf, kf = run_device(fi, fo, nch, S, kw, x, np.float32, api)
    yd, kd = run_device(fi, fo, nch, S, kw, x, np.float64, api)
    assert yd.dtype == np.float64 and yd.shape == yf.shape
    assert np.array_equal(yd.astype(np.float32).view(np.uint32), yf.view(np.uint32))
    assert kd == sorted({dio_name(k) for k in kf}), (kf, kd)


def test_lean_kernels_have_double_counterparts():
    """The headline chain's lean kernel runs as its float64-frame instance on a double handle."""
    x = noise(1, 60000, 2, 5)
    _, kf = run_device(44100, 96000, 2, 1, {}, x, np.float32)
    _, kd = run_device(44100, 96000, 2, 1, {}, x, np.float64)
    assert any(k.startswith("rsmp::fused_fast_kernel<") for k in kf), kf
    assert any(k.startswith("rsmp::fused_fast_dio_kernel<") for k in kd), kd
    _, kd2 = run_device(44100, 192000, 8, 1, BW99, noise(1, 60000, 8, 6), np.float64)
    assert "rsmp::fused_split_dio_kernel<9, 1>" in kd2 and "rsmp::dftx_kernel<4>" in kd2, kd2


def host_double(fi, fo, nch, kw, x, chunk=4096):
    r = F.Resampler(fi, fo, nch=nch, dtype=np.float64, **kw)
    y = r.process(x.astype(np.float64), chunk=chunk)
    r.close()
    return y


@pytest.mark.parametrize("fi,fo,kw", [(44100, 96000, {}), (44100, 48000, BW99)])
def test_fp64_parity_with_oracle(fi, fo, kw):
    """The oracle's fp64 output fifo (pushed whole, never pulled, drained) against the double handle's output.
    Measured max|y - o| / max|o| on an MI355X (50 000 stereo frames): 44.1k->96k 1.13e-15, 44.1k->48k bw 99 1.06e-15 -- the
    engine's fp64 summation order differs from the oracle's, nothing more.  The bound, 1e-13, is ~100x that and ~6e5x under
    one float32 ulp (~6e-8), so any float-rounded sample fails it."""
    x = lcg_noise(50000, 2, 4242).reshape(-1, 2)
    y = host_double(fi, fo, 2, kw, x)
    o = Oracle(fi, fo, 2, **kw)
    o.push(x)
    o.drain()
    ns = len(o.plan())
    ref = np.stack([o.stage_fifo(ch, ns) for ch in range(2)], axis=1)
    assert ref.shape == y.shape, (ref.shape, y.shape)
    rel = np.abs(y - ref).max() / np.abs(ref).max()
    assert rel < 1e-13, rel


def test_sub_float_input_reaches_output():
    a = lcg_noise(40000, 2, 99).reshape(-1, 2).astype(np.float64)
    rng = np.random.default_rng(3)
    d = rng.standard_normal(a.shape) * np.abs(a) * 2.0 ** -30
    x = a + d
    assert np.mean(x.astype(np.float32).astype(np.float64) != x) > 0.9  # d is below float32 resolution next to a
    ya = host_double(44100, 96000, 2, {}, a)
    yx = host_double(44100, 96000, 2, {}, x)
    yd = host_double(44100, 96000, 2, {}, d * 2.0 ** 30) * 2.0 ** -30
    diff = yx - ya
    rel = np.sqrt(np.mean((diff - yd) ** 2) / np.mean(yd ** 2))
    assert rel <= 1e-5, rel


def test_call_pattern_invariance():
    fi, fo, nch, n = 44100, 48000, 2, 30000
    x = lcg_noise(n, nch, 7).reshape(n, nch).astype(np.float64)
    ref = host_double(fi, fo, nch, {}, x, chunk=n)  # one push (below isamp_max)
    assert ref.shape[0] == round(n * fo / fi)
    r = F.Resampler(fi, fo, nch=nch, dtype=np.float64)
    parts, pos, sizes, i = [], 0, [1, 977, 4096], 0
    while pos < n:
        k = min(sizes[i % 3], n - pos)
        r.push(x[pos:pos + k])
        parts.append(r.pull_all())
        pos, i = pos + k, i + 1
    r.drain()
    parts.append(r.pull_all())
    assert np.array_equal(np.concatenate(parts).view(np.uint64), ref.view(np.uint64))
    r2 = F.Resampler(fi, fo, nch=nch, dtype=np.float64)
    parts = []
    for s0 in range(0, n, 5000):
        iu, y = r2.flow(x[s0:s0 + 5000], 8000)
        assert iu == min(5000, n - s0)
        parts.append(y)
    r2.drain()
    parts.append(r2.pull_all())
    assert np.array_equal(np.concatenate(parts).view(np.uint64), ref.view(np.uint64))
    r3 = F.Resampler(fi, fo, nch=nch, dtype=np.float64)
    big = np.tile(x, (int(r3.isamp_max // n) + 2, 1))
    r3.push(big)  # clamped to isamp_max, like RR_push
    got = r3.pull_all()
    r3.drain()
    got = np.concatenate([got, r3.pull_all()])
    assert got.shape[0] == round(r3.isamp_max * fo / fi)


def test_device_forms_strided_offset_odd_channels():
    """torch.float64 buffers with a stream stride, based one double past an allocation (8- but not 16-byte aligned), odd
    channel count, consumed in place by RRX_flow_device_double on torch's stream (tests/devbuf.py's ordering rule: the
    handle works on the stream that filled the buffers)."""
    fi, fo, nch, S, n = 44100, 96000, 3, 2, 40000
    x = noise(S, n, nch, 31).astype(np.float64)
    ref = np.stack([host_double(fi, fo, nch, {}, x[s], chunk=n) for s in range(S)])
    r = F.Resampler(fi, fo, nch=nch, nstreams=S, dtype=np.float64)
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    istride, ostride = n + 5, int(n * fo / fi) + 9000
    ib = torch.zeros(1 + S * istride * nch, dtype=torch.float64, device="cuda")
    ob = torch.zeros(1 + S * ostride * nch, dtype=torch.float64, device="cuda")
    iv, ov = ib[1:].view(S, istride, nch), ob[1:].view(S, ostride, nch)
    assert iv.data_ptr() % 16 == 8
    iv[:, :n] = torch.from_numpy(x).cuda()
    iu, og = r.flow_device(iv, n, ov, ostride, in_stride=istride, out_stride=ostride)
    assert iu == n
    r.drain()
    tail = torch.zeros((S, 65536, nch), dtype=torch.float64, device="cuda")
    og2 = r.pull_device(tail, 65536)
    r.sync()
    y = np.concatenate([ov[:, :og].cpu().numpy(), tail[:, :og2].cpu().numpy()], axis=1)
    assert np.array_equal(y.view(np.uint64), ref.view(np.uint64))
    assert ib[0].item() == 0.0 and ob[0].item() == 0.0  # nothing in front of the caller's buffers was touched


MANY = (
    "import sys, json; sys.path[:0] = [%r, %r]\n"
    "import numpy as np, torch, foo_dsp_resampler_amd as F\n"
    "from oracle_binding import lcg_noise\n"
    "S, n, nch, fi, fo = 64, 300000, 2, 44100, %d\n"
    "x = torch.from_numpy(np.stack([lcg_noise(n, nch, 500 + s).reshape(n, nch) for s in range(S)]).astype(np.float64)).cuda()\n"
    "r = F.Resampler(fi, fo, nch=nch, nstreams=S, dtype=np.float64)\n"
    "r.set_stream(torch.cuda.current_stream().cuda_stream)\n"
    "r.profile(True)\n"
    "cap = int(n * fo / fi) + 65536\n"
    "y = torch.zeros((S, cap, nch), dtype=torch.float64, device='cuda'); iu, og = r.flow_device(x, n, y, cap)\n"
    "rep = r.profile_report(); r.sync()\n"
    "launches = max([k['launches'] for k in rep if 'fused' in k['kernel'] and 'prep' not in k['kernel']] or [0])\n"
    "np.save(%r, y[[0, S // 2, S - 1], :og].cpu().numpy())\n"
    "print(json.dumps({'launches': launches, 'og': og}))\n"
)


@pytest.mark.parametrize("fo", [96000, 48000])
def test_many_launches_per_push_double(fo, tmp_path):
    """RSMP_SEAM_RING_MB=4 (read once per process: own process) cuts one push of 64 stereo streams x 300 000 frames into
    several launches with seam kernels beside them; the double seam path must give the bits of one launch."""
    outs = {}
    for tag, env_mb in (("many", "4"), ("one", None)):
        f = str(tmp_path / ("%s.npy" % tag))
        env = dict(os.environ)
        env.pop("RSMP_SEAM_RING_MB", None)
        if env_mb:
            env["RSMP_SEAM_RING_MB"] = env_mb
        p = subprocess.run([sys.executable, "-c", MANY % (ROOT, os.path.join(ROOT, "tests"), fo, f)], env=env, capture_output=True,
                           text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        outs[tag] = (json.loads(p.stdout.strip().splitlines()[-1]), np.load(f))
    assert outs["many"][0]["launches"] > outs["one"][0]["launches"], outs
    assert outs["many"][0]["og"] == outs["one"][0]["og"]
    assert np.array_equal(outs["many"][1].view(np.uint64), outs["one"][1].view(np.uint64))


def test_mismatched_call_leaves_handle_untouched():
    fi, fo, nch = 44100, 96000, 2
    x = lcg_noise(20000, nch, 8).reshape(-1, nch).astype(np.float64)
    ref = host_double(fi, fo, nch, {}, x, chunk=4096)
    r = F.Resampler(fi, fo, nch=nch, dtype=np.float64)
    assert r.format == F.RRX_FMT_DOUBLE
    L = F.lib()
    f32 = np.zeros((4096, nch), np.float32)
    n = C.c_size_t(0)
    assert L.RR_push(r.h, f32.ctypes.data, 4096) == RR_INVPARAM
    assert L.RR_pull(r.h, f32.ctypes.data, 4096, C.byref(n)) == RR_INVPARAM
    assert L.RRX_push_strided(r.h, f32.ctypes.data, 4096, 4096) == RR_INVPARAM
    assert r.available == 0
    y = r.process(x, chunk=4096)
    assert np.array_equal(y.view(np.uint64), ref.view(np.uint64))
    rf = F.Resampler(fi, fo, nch=nch)
    assert rf.format == F.RRX_FMT_FLOAT
    assert L.RRX_push_double(rf.h, x.ctypes.data, 4096, 4096) == RR_INVPARAM
    assert rf.available == 0
