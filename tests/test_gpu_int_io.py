"""Integer PCM sample buffers (RRX_FMT_S16 / RRX_FMT_S32 handles, RRX_*_samples calls) on the GPU.

An integer handle runs the float handle's chain -- same stage kernels, same geometry, same fp64 arithmetic -- with loads that
scale by 2^-bits and stores that round to even, saturate and narrow.  The defining property: its output equals, bit for bit,
the output of a double handle fed s * 2^-bits, quantised by that rule.  The double handle is pinned on the CPU oracle by
tests/test_gpu_double_io.py; three chains are also checked against the oracle directly here."""
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
FMTS = [F.RRX_FMT_S16, F.RRX_FMT_S32]
BITS = {F.RRX_FMT_S16: 15, F.RRX_FMT_S32: 31}
NPDT = {F.RRX_FMT_FLOAT: np.float32, F.RRX_FMT_DOUBLE: np.float64, F.RRX_FMT_S16: np.int16, F.RRX_FMT_S32: np.int32}
TAG = {F.RRX_FMT_S16: "s16", F.RRX_FMT_S32: "s32"}


def int_name(k, fmt):
    """the lean kernels' integer-frame instances carry their own names; every other kernel is the same instance for all formats"""
    for fam in ("fused_fast", "fused_split2", "fused_split"):
        a = "rsmp::%s_kernel<" % fam
        if k.startswith(a):
            return "rsmp::%s_%s_kernel<" % (fam, TAG[fmt]) + k[len(a):]
    return k


def noise(S, n, nch, seed):
    return np.stack([lcg_noise(n, nch, seed + s).reshape(n, nch) for s in range(S)])


def to_pcm(x, fmt, amp=1.0, seed=0):
    """float noise (24-bit resolution) -> the format's integers; S32 gets its low 8 bits from a second noise, so all 32 bits carry data"""
    bits = BITS[fmt]
    q = np.rint(np.asarray(x, np.float64) * amp * 2.0 ** bits)
    if fmt == F.RRX_FMT_S32:
        low = lcg_noise(x.size, 1, 9001 + seed).reshape(x.shape).view(np.uint32) & 0xFF
        q = q + low.astype(np.float64) - 128.0
    return np.clip(q, -2.0 ** bits, 2.0 ** bits - 1).astype(NPDT[fmt])


def quantise(y, fmt):
    """the output rule of ratelib_amd.h in numpy: round half to even, saturate in fp64, narrow"""
    bits = BITS[fmt]
    return np.clip(np.rint(y * 2.0 ** bits), -2.0 ** bits, 2.0 ** bits - 1).astype(NPDT[fmt])


def as_double(s, fmt):
    return s.astype(np.float64) * 2.0 ** -BITS[fmt]


def run_device(fi, fo, nch, S, kw, x, fmt, api="flow", chunk=16384):
    """x: [S, n, nch] host array of the format's dtype.  Device path on torch's stream; returns (y [S, m, nch], frames per
    call, kernel names)."""
    dt = NPDT[fmt]
    assert x.dtype == dt
    tdt = getattr(torch, np.dtype(dt).name)
    r = F.Resampler(fi, fo, nch=nch, nstreams=S, sample_format=fmt, **kw)
    assert r.format == fmt
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    r.profile(True)
    n = x.shape[1]
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    parts, counts = [], []
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
        counts.append(og)
        parts.append(y[:, :og].cpu().numpy())
    r.drain()
    tail = torch.zeros((S, 1 << 17, nch), dtype=tdt, device="cuda")
    og = r.pull_device(tail, 1 << 17)
    counts.append(og)
    parts.append(tail[:, :og].cpu().numpy())
    r.sync()
    names = sorted({k["kernel"] for k in r.profile_report()})
    r.close()
    return np.concatenate(parts, axis=1), counts, names


CASES = [  # (fi, fo, nch, streams, kw, api): the list of tests/test_gpu_double_io.py
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


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("fi,fo,nch,S,kw,api", CASES)
def test_defining_property_and_dispatch(fi, fo, nch, S, kw, api, fmt):
    """integer handle == quantise(double handle fed s * 2^-bits), bit for bit, frame counts equal after every call; and the
    kernels are the float run's with the lean ones replaced by their integer instances"""
    s = to_pcm(noise(S, 60000, nch, 17 + nch), fmt, seed=nch)
    if fmt == F.RRX_FMT_S32:
        assert np.mean((s & 0xFF) != 0) > 0.9  # all 32 bits in use
    yi, ci, ki = run_device(fi, fo, nch, S, kw, s, fmt, api)
    yd, cd, _ = run_device(fi, fo, nch, S, kw, as_double(s, fmt), F.RRX_FMT_DOUBLE, api)
    _, _, kf = run_device(fi, fo, nch, S, kw, as_double(s, fmt).astype(np.float32), F.RRX_FMT_FLOAT, api)
    assert ci == cd, (ci, cd)
    assert yi.dtype == NPDT[fmt] and yi.shape == yd.shape
    ref = quantise(yd, fmt)
    assert np.array_equal(yi, ref), (int(np.sum(yi != ref)), yi.size)
    assert ki == sorted({int_name(k, fmt) for k in kf}), (kf, ki)


def test_lean_kernels_have_integer_counterparts():
    s = to_pcm(noise(1, 60000, 2, 5), F.RRX_FMT_S16)
    _, _, k16 = run_device(44100, 96000, 2, 1, {}, s, F.RRX_FMT_S16)
    assert any(k.startswith("rsmp::fused_fast_s16_kernel<") for k in k16), k16
    for fmt in FMTS:
        s = to_pcm(noise(1, 60000, 8, 6), fmt)
        _, _, k2 = run_device(44100, 192000, 8, 1, BW99, s, fmt)
        assert "rsmp::fused_split_%s_kernel<9, 1>" % TAG[fmt] in k2 and "rsmp::dftx_kernel<4>" in k2, k2


def host_run(fi, fo, nch, kw, x, fmt, chunk=4096):
    r = F.Resampler(fi, fo, nch=nch, sample_format=fmt, **kw)
    y = r.process(x, chunk=chunk)
    r.close()
    return y


def tie_rule_reference(ref64, fmt):
    """The oracle's fp64 output as the integer handle must give it: (the quantised samples, the mask of samples whose scaled
    value lies within 2^bits * 1e-13 * max|o| of a rounding tie).  None may clip."""
    bits = BITS[fmt]
    q = ref64 * 2.0 ** bits
    assert q.max() < 2.0 ** bits - 1 and q.min() > -2.0 ** bits  # none clip
    window = 2.0 ** bits * 1e-13 * np.abs(ref64).max()
    return quantise(ref64, fmt), np.abs(np.abs(q - np.floor(q)) - 0.5) <= window


def assert_tie_rule(size, in_window, max_abs_d, differing, unexcused):
    """The tie-window rule on the counts of a comparison of `size` samples: d = handle - quantised oracle, `in_window` samples
    in the tie window, `differing` with d != 0, `unexcused` of those outside the window."""
    cap = 1e-3 * size
    assert in_window <= cap, (in_window, cap)
    assert max_abs_d <= 1, max_abs_d
    assert unexcused == 0, unexcused
    assert differing <= cap, (differing, cap)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("fi,fo,kw", [(44100, 96000, {}), (44100, 48000, BW99), (96000, 44100, {})])
def test_against_oracle(fi, fo, kw, fmt):
    """The oracle's fp64 output fifo (pushed whole, drained), quantised in numpy, against the integer handle.  Every sample
    within 1 LSB; a sample may differ only where the oracle's scaled value lies within 2^bits * 1e-13 * max|o| of a rounding
    tie (1e-13: the fp64 parity bound of test_fp64_parity_with_oracle); at most 0.1 % of the samples may, and the oracle's own
    count of in-window samples must be below that cap too (so the test cannot pass by excusing everything).  (The rule itself:
    tie_rule_reference and assert_tie_rule above, shared with tests/test_gpu_far_positions.py.)"""
    x = lcg_noise(50000, 2, 4242).reshape(-1, 2)
    if fmt == F.RRX_FMT_S16:
        s = np.rint(x.astype(np.float64) * 2.0 ** 15).astype(np.int16)
    else:
        s = (np.rint(x.astype(np.float64) * 2.0 ** 23).astype(np.int64) << 8).astype(np.int32)  # 24-bit audio, left-justified
    xo = as_double(s, fmt)
    assert np.array_equal(xo.astype(np.float32).astype(np.float64), xo)  # exact in the oracle's float32 input
    y = host_run(fi, fo, 2, kw, s, fmt)
    o = Oracle(fi, fo, 2, **kw)
    o.push(xo.astype(np.float32))
    o.drain()
    ns = len(o.plan())
    ref64 = np.stack([o.stage_fifo(ch, ns) for ch in range(2)], axis=1)
    assert ref64.shape == y.shape, (ref64.shape, y.shape)
    ref, near_tie = tie_rule_reference(ref64, fmt)
    d = y.astype(np.int64) - ref.astype(np.int64)
    print("against oracle: fmt %d %d->%d differing %d, in window %d, of %d, max |d| %d" %
          (fmt, fi, fo, int(np.sum(d != 0)), int(np.sum(near_tie)), y.size, int(np.abs(d).max())))
    assert_tie_rule(y.size, int(np.sum(near_tie)), int(np.abs(d).max()), int(np.sum(d != 0)), int(np.sum((d != 0) & ~near_tie)))


@pytest.mark.parametrize("fmt", FMTS)
def test_saturation(fmt):
    """full-scale noise: the chain's peaks pass 1.0, so both rails are hit; saturated, never wrapped"""
    bits = BITS[fmt]
    s = to_pcm(noise(1, 60000, 2, 4242), fmt, amp=2.0)
    yd, _, _ = run_device(44100, 96000, 2, 1, {}, as_double(s, fmt), F.RRX_FMT_DOUBLE)
    assert yd.max() > 1.0 and yd.min() < -1.0
    ref = quantise(yd, fmt)
    hi, lo = int(2 ** bits - 1), int(-2 ** bits)
    assert np.sum(ref == hi) > 0 and np.sum(ref == lo) > 0  # not vacuous
    yi, _, _ = run_device(44100, 96000, 2, 1, {}, s, fmt)
    assert np.array_equal(yi, ref)
    over = yd * 2.0 ** bits
    assert np.all(yi[over >= hi] == hi) and np.all(yi[over <= lo] == lo)


@pytest.mark.parametrize("fmt", FMTS)
def test_call_pattern_invariance(fmt):
    fi, fo, nch, n = 44100, 48000, 2, 30000
    x = to_pcm(lcg_noise(n, nch, 7).reshape(n, nch), fmt)
    ref = host_run(fi, fo, nch, {}, x, fmt, chunk=n)  # one push (below isamp_max)
    assert ref.shape[0] == round(n * fo / fi) and ref.dtype == NPDT[fmt]
    r = F.Resampler(fi, fo, nch=nch, sample_format=fmt)
    parts, pos, sizes, i = [], 0, [1, 977, 4096], 0  # plugin-sized pushes: the page-locked slot and mirror path; 1-frame pushes
    while pos < n:
        k = min(sizes[i % 3], n - pos)
        r.push(x[pos:pos + k])
        parts.append(r.pull_all())
        pos, i = pos + k, i + 1
    r.drain()
    parts.append(r.pull_all())
    assert np.array_equal(np.concatenate(parts), ref)
    r.drain()  # re-drain: nothing more
    assert r.pull_all().shape[0] == 0
    r2 = F.Resampler(fi, fo, nch=nch, sample_format=fmt)
    parts = []
    for s0 in range(0, n, 5000):
        iu, y = r2.flow(x[s0:s0 + 5000], 8000)
        assert iu == min(5000, n - s0)
        parts.append(y)
    r2.drain()
    parts.append(r2.pull_all())
    assert np.array_equal(np.concatenate(parts), ref)
    r3 = F.Resampler(fi, fo, nch=nch, sample_format=fmt)
    big = np.tile(x, (int(r3.isamp_max // n) + 2, 1))
    r3.push(big)  # clamped to isamp_max, like RR_push
    got = r3.pull_all()
    r3.drain()
    got = np.concatenate([got, r3.pull_all()])
    assert got.shape[0] == round(r3.isamp_max * fo / fi)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("nch", [1, 3, 5])
def test_odd_channels_odd_pushes_host(nch, fmt):
    """odd channel counts with an odd number of frames per push: S16 frames are then not a multiple of 4 bytes anywhere (slot,
    mirror, ring carry, copy out)"""
    fi, fo, n = 44100, 96000, 20001
    x = to_pcm(lcg_noise(n, nch, 70 + nch).reshape(n, nch), fmt)
    ref = host_run(fi, fo, nch, {}, x, fmt, chunk=n)
    r = F.Resampler(fi, fo, nch=nch, sample_format=fmt)
    parts, pos = [], 0
    for k in [333, 1, 4097, 7, 2501] * 100:
        if pos >= n:
            break
        k = min(k, n - pos)
        r.push(x[pos:pos + k])
        if (pos // 3) % 2:  # leave some pushes unpulled: ring carry and mirror spill
            parts.append(r.pull(1501))
        pos += k
    r.drain()
    parts.append(r.pull_all())
    assert np.array_equal(np.concatenate(parts), ref)
    # device push / pull gives the same bits as device flow and as the host path
    xs = x[None]
    y1, _, _ = run_device(fi, fo, nch, 1, {}, xs, fmt, "flow", chunk=4999)
    y2, _, _ = run_device(fi, fo, nch, 1, {}, xs, fmt, "pushpull", chunk=4999)
    assert np.array_equal(y1[0], ref) and np.array_equal(y2[0], ref)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("fi,fo,nch,kw", [(44100, 96000, 3, {}), (44100, 96000, 2, {}), (44100, 48000, 2, BW99), (44100, 192000, 2, BW99)])
def test_device_forms_strided_offset(fi, fo, nch, kw, fmt):
    """batch buffers with a stream stride, based one sample past an allocation (S16 pairs only 2-byte aligned, S32 pairs only
    4-byte aligned), consumed in place by RRX_flow_device_samples on torch's stream"""
    S, n = 2, 40000
    dt = NPDT[fmt]
    tdt = getattr(torch, np.dtype(dt).name)
    x = to_pcm(noise(S, n, nch, 31), fmt)
    ref = np.stack([host_run(fi, fo, nch, kw, x[s], fmt, chunk=n) for s in range(S)])
    r = F.Resampler(fi, fo, nch=nch, nstreams=S, sample_format=fmt, **kw)
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    istride, ostride = n + 5, int(n * fo / fi) + 9000
    ib = torch.zeros(1 + S * istride * nch, dtype=tdt, device="cuda")
    ob = torch.zeros(1 + S * ostride * nch, dtype=tdt, device="cuda")
    iv, ov = ib[1:].view(S, istride, nch), ob[1:].view(S, ostride, nch)
    esz = np.dtype(dt).itemsize
    assert iv.data_ptr() % (2 * esz) == esz
    iv[:, :n] = torch.from_numpy(x).cuda()
    iu, og = r.flow_device(iv, n, ov, ostride, in_stride=istride, out_stride=ostride)
    assert iu == n
    r.drain()
    tail = torch.zeros((S, 1 << 17, nch), dtype=tdt, device="cuda")
    og2 = r.pull_device(tail, 1 << 17)
    r.sync()
    y = np.concatenate([ov[:, :og].cpu().numpy(), tail[:, :og2].cpu().numpy()], axis=1)
    assert np.array_equal(y, ref)
    assert ib[0].item() == 0 and ob[0].item() == 0  # nothing in front of the caller's buffers was touched
    r.close()


MANY = (
    "import sys, json; sys.path[:0] = [%r, %r]\n"
    "import numpy as np, torch, foo_dsp_resampler_amd as F\n"
    "from oracle_binding import lcg_noise\n"
    "S, n, nch, fi, fo, fmt = 64, 300000, 2, 44100, %d, %d\n"
    "bits = 15 if fmt == 16 else 31\n"
    "x = np.stack([lcg_noise(n, nch, 500 + s).reshape(n, nch) for s in range(S)]).astype(np.float64)\n"
    "x = torch.from_numpy(np.rint(x * 2.0 ** bits).astype(np.int16 if fmt == 16 else np.int32)).cuda()\n"
    "r = F.Resampler(fi, fo, nch=nch, nstreams=S, sample_format=fmt)\n"
    "r.set_stream(torch.cuda.current_stream().cuda_stream)\n"
    "r.profile(True)\n"
    "cap = int(n * fo / fi) + 65536\n"
    "y = torch.zeros((S, cap, nch), dtype=x.dtype, device='cuda'); iu, og = r.flow_device(x, n, y, cap)\n"
    "rep = r.profile_report(); r.sync()\n"
    "launches = max([k['launches'] for k in rep if 'fused' in k['kernel'] and 'prep' not in k['kernel']] or [0])\n"
    "np.save(%r, y[[0, S // 2, S - 1], :og].cpu().numpy())\n"
    "print(json.dumps({'launches': launches, 'og': og}))\n"
)


@pytest.mark.parametrize("fo,fmt", [(96000, F.RRX_FMT_S16), (48000, F.RRX_FMT_S32)])
def test_many_launches_per_push(fo, fmt, tmp_path):
    """RSMP_SEAM_RING_MB=4 (read once per process: own process) cuts one push of 64 stereo streams x 300 000 frames into
    several launches with seam kernels beside them; the integer seam path must give the bits of one launch."""
    outs = {}
    for tag, env_mb in (("many", "4"), ("one", None)):
        f = str(tmp_path / ("%s.npy" % tag))
        env = dict(os.environ)
        env.pop("RSMP_SEAM_RING_MB", None)
        if env_mb:
            env["RSMP_SEAM_RING_MB"] = env_mb
        p = subprocess.run([sys.executable, "-c", MANY % (ROOT, os.path.join(ROOT, "tests"), fo, fmt, f)], env=env, capture_output=True,
                           text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        outs[tag] = (json.loads(p.stdout.strip().splitlines()[-1]), np.load(f))
    assert outs["many"][0]["launches"] > outs["one"][0]["launches"], outs
    assert outs["many"][0]["og"] == outs["one"][0]["og"]
    assert np.array_equal(outs["many"][1], outs["one"][1])


@pytest.mark.parametrize("fmt", FMTS)
def test_mismatched_calls_leave_handle_untouched(fmt):
    fi, fo, nch = 44100, 96000, 2
    dt = NPDT[fmt]
    x = to_pcm(lcg_noise(20000, nch, 8).reshape(-1, nch), fmt)
    ref = host_run(fi, fo, nch, {}, x, fmt, chunk=4096)
    r = F.Resampler(fi, fo, nch=nch, sample_format=fmt)
    assert r.format == fmt
    L = F.lib()
    r.push(x[:4096])  # something in the fifo, so "untouched" is visible in RRX_available
    avail = r.available
    assert avail > 0
    hb = np.zeros((4096, nch), np.float64)  # large enough for any format
    db = torch.zeros((4096, nch), dtype=torch.float64, device="cuda")
    hp, dp = hb.ctypes.data, C.c_void_p(db.data_ptr())
    n, m = C.c_size_t(0), C.c_size_t(0)
    # every typed data call
    assert L.RR_push(r.h, hp, 4096) == RR_INVPARAM
    assert L.RR_pull(r.h, hp, 4096, C.byref(n)) == RR_INVPARAM
    assert L.RR_flow(r.h, hp, hp, 2048, 2048, C.byref(n), C.byref(m)) == RR_INVPARAM
    assert L.RRX_push_strided(r.h, hp, 4096, 4096) == RR_INVPARAM
    assert L.RRX_pull_strided(r.h, hp, 4096, 4096, C.byref(n)) == RR_INVPARAM
    assert L.RRX_push_device(r.h, dp, 4096, 4096) == RR_INVPARAM
    assert L.RRX_pull_device(r.h, dp, 4096, 4096, C.byref(n)) == RR_INVPARAM
    assert L.RRX_flow_device(r.h, dp, 2048, dp, 2048, 2048, 2048, C.byref(n), C.byref(m)) == RR_INVPARAM
    assert L.RRX_push_double(r.h, hp, 4096, 4096) == RR_INVPARAM
    assert L.RRX_pull_double(r.h, hp, 4096, 4096, C.byref(n)) == RR_INVPARAM
    assert L.RRX_flow_double(r.h, hp, 2048, hp, 2048, 2048, 2048, C.byref(n), C.byref(m)) == RR_INVPARAM
    assert L.RRX_push_device_double(r.h, dp, 4096, 4096) == RR_INVPARAM
    assert L.RRX_pull_device_double(r.h, dp, 4096, 4096, C.byref(n)) == RR_INVPARAM
    assert L.RRX_flow_device_double(r.h, dp, 2048, dp, 2048, 2048, 2048, C.byref(n), C.byref(m)) == RR_INVPARAM
    # every format-tagged call with another format's tag
    for other in (F.RRX_FMT_FLOAT, F.RRX_FMT_DOUBLE, F.RRX_FMT_S16, F.RRX_FMT_S32, 24):
        if other == fmt:
            continue
        assert L.RRX_push_samples(r.h, other, hp, 4096, 4096) == RR_INVPARAM
        assert L.RRX_pull_samples(r.h, other, hp, 4096, 4096, C.byref(n)) == RR_INVPARAM
        assert L.RRX_flow_samples(r.h, other, hp, 2048, hp, 2048, 2048, 2048, C.byref(n), C.byref(m)) == RR_INVPARAM
        assert L.RRX_push_device_samples(r.h, other, dp, 4096, 4096) == RR_INVPARAM
        assert L.RRX_pull_device_samples(r.h, other, dp, 4096, 4096, C.byref(n)) == RR_INVPARAM
        assert L.RRX_flow_device_samples(r.h, other, dp, 2048, dp, 2048, 2048, 2048, C.byref(n), C.byref(m)) == RR_INVPARAM
    assert r.available == avail
    parts = [r.pull_all()]
    for s0 in range(4096, x.shape[0], 4096):
        r.push(x[s0:s0 + 4096])
        parts.append(r.pull_all())
    r.drain()
    parts.append(r.pull_all())
    assert np.array_equal(np.concatenate(parts), ref)
    r.close()


@pytest.mark.parametrize("fmt", [F.RRX_FMT_FLOAT, F.RRX_FMT_DOUBLE])
def test_samples_calls_on_float_and_double_handles(fmt):
    """the format-tagged calls with the matching tag give the typed calls' bits; an integer tag is refused"""
    fi, fo, nch, n = 44100, 96000, 2, 20000
    dt = NPDT[fmt]
    x = lcg_noise(n, nch, 8).reshape(-1, nch).astype(dt)
    r0 = F.Resampler(fi, fo, nch=nch, dtype=dt)
    ref = r0.process(x, chunk=4096)
    r0.close()
    L = F.lib()
    r = F.Resampler(fi, fo, nch=nch, dtype=dt)
    g = C.c_size_t(0)
    assert L.RRX_push_samples(r.h, F.RRX_FMT_S16, x.ctypes.data, 4096, 4096) == RR_INVPARAM
    assert L.RRX_push_samples(r.h, F.RRX_FMT_S32, x.ctypes.data, 4096, 4096) == RR_INVPARAM
    assert r.available == 0
    parts = []

    def pull_all():
        while True:
            out = np.empty((8192, nch), dt)
            assert L.RRX_pull_samples(r.h, fmt, out.ctypes.data, 8192, 8192, C.byref(g)) == 0
            if not g.value:
                return
            parts.append(out[:g.value].copy())

    for s0 in range(0, n, 4096):
        xs = np.ascontiguousarray(x[s0:s0 + 4096])
        assert L.RRX_push_samples(r.h, fmt, xs.ctypes.data, xs.shape[0], xs.shape[0]) == 0
        pull_all()
    r.drain()
    pull_all()
    y = np.concatenate(parts)
    assert y.shape == ref.shape and np.array_equal(y.view(np.uint8), ref.view(np.uint8))
    # device forms against the typed device forms
    tdt = getattr(torch, np.dtype(dt).name)
    xd = torch.from_numpy(x).cuda()
    outs = []
    for tagged in (False, True):
        rr = F.Resampler(fi, fo, nch=nch, dtype=dt)
        rr.set_stream(torch.cuda.current_stream().cuda_stream)
        cap = int(n * fo / fi) + 8192
        yd = torch.zeros((cap, nch), dtype=tdt, device="cuda")
        iu, og = C.c_size_t(0), C.c_size_t(0)
        if tagged:
            rc = L.RRX_flow_device_samples(rr.h, fmt, C.c_void_p(xd.data_ptr()), n, C.c_void_p(yd.data_ptr()), cap, n, cap, C.byref(iu), C.byref(og))
            assert rc == 0 and iu.value == n
            got = og.value
        else:
            _, got = rr.flow_device(xd, n, yd, cap)
        rr.sync()
        outs.append(yd[:got].cpu().numpy())
        rr.close()
    assert outs[0].shape == outs[1].shape and np.array_equal(outs[0].view(np.uint8), outs[1].view(np.uint8))
