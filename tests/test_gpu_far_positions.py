"""One stream taken past 2^31 and 2^32 frames of absolute position on the GPU, held to the oracle all the way.

Every case of tests/far_cases.py pushes ONE device-resident buffer n_far times -- until the input count, the output count and
every stage fifo's count have passed 2^32 -- and compares every call's output on the device with the oracle's window R by
running output position (the premise: tests/test_far_cases_api.py).  Nothing synchronises per push: each call's result is
folded into a few device scalars and a per-call vector, read once at the end.  A narrowing of an absolute position to 32 bits
anywhere in a kernel or its launcher shows as an error that begins at one call; the failure message names that call's position.

Measured on an MI355X (wall time of the whole test, max error, relative RMS, bit-equal fraction): RESULTS below.
"""
import time

import numpy as np
import pytest

import foo_dsp_resampler_amd as F
import far_cases as FC
from parity import ULP_FLOOR, assert_parity

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_int_io import assert_tie_rule, tie_rule_reference  # noqa: E402  (the integer rule, reused and not restated)

RESULTS = """
case    n_far  seconds  max error              rel_rms    bit_equal_frac   (every call, positions Wo .. n_far Wo)
up       8920   2.3     0 ulp                  0          1.0
down     8921   1.6     0.25 ulp               1.6e-15    0.99999923
x4      17839   3.9     0.0078 ulp             7.0e-18    0.99999998
half    17842   3.0     1.0 ulp                1.1e-14    0.99999996
odd      4460   1.8     1.0 ulp                6.4e-15    0.999999993
f64      4460   1.3     1.19e-15 full scale    1.8e-16    0.073
s16      8920   2.0     0 LSB, none differ     -          1.0
long    12292   3.0     1.0 ulp                1.3e-15    0.99999909
interp   4460   1.6     residual 4.06e-08 (rms 1.015e-08) on the GPU over 259 calls; r_o 3.75e-08 (rms 1.014e-08) on the oracle
host     8921   1.0     0 ulp over 192 host pushes around the four crossings
(seconds: the whole test with its reference, one process per test.  An error below one ulp is a sample under 2^-17, where the ulp
is taken at 2^-17; 1.0 ulp is one float32 rounding flip against R, which is the oracle at ANOTHER period of the same phase: its
own periods differ by up to 0.25 ulp, tests/test_far_cases_api.py.  No case needed cutting to 2^31.)
"""

OPEN = {"f32": {}, "f64": {"dtype": np.float64}, "s16": {"sample_format": F.RRX_FMT_S16}}
TDT = {"f32": torch.float32, "f64": torch.float64, "s16": torch.int16}


class Fold:
    """Comparison of a handle's output with reference rows, folded on the device: fold(i, got, o) holds the frames `got` of call
    i against rows [o, o + len(got)) of `ref64` and only enqueues; report() synchronises, once.  Per format the bar of the
    project: f32 -- tests/parity.py (<= 1 ulp at max(|ref|, 2^-17), relative RMS <= 1e-7, formed from the sums); f64 -- 1e-13 of
    full scale (tests/test_gpu_fp64_parity.py); s16 -- the tie-window rule of tests/test_gpu_int_io.py::test_against_oracle."""

    def __init__(self, fmt, ref64, ncalls, scale=None):
        self.fmt, self.n, self.host_sum, self.starts = fmt, 0, 0.0, {}
        self.percall = torch.zeros(max(ncalls, 1), dtype=torch.float64, device="cuda")
        self.sq = torch.zeros((), dtype=torch.float64, device="cuda")
        self.ne = torch.zeros((), dtype=torch.int64, device="cuda")
        self.unexcused = torch.zeros((), dtype=torch.int64, device="cuda")
        if fmt == "f32":
            r32 = ref64.astype(np.float32)
            self.ref = torch.from_numpy(r32).cuda()
            self.ulp = torch.from_numpy(np.spacing(np.maximum(np.abs(r32), np.float32(ULP_FLOOR)).astype(np.float32))).cuda()
            host = (r32.astype(np.float64) ** 2).sum(axis=1)  # sum of ref^2 per row: rel_rms's denominator, by prefix sums
        elif fmt == "f64":
            self.ref = torch.from_numpy(np.array(ref64)).cuda()  # (a copy: the shared reference is read-only)
            self.scale = float(np.abs(ref64).max()) if scale is None else scale
            host = np.zeros(ref64.shape[0])
        else:
            q, tie = tie_rule_reference(ref64, F.RRX_FMT_S16)
            self.ref, self.tie = torch.from_numpy(q).cuda(), torch.from_numpy(tie).cuda()
            host = tie.sum(axis=1).astype(np.float64)  # samples in the tie window per row
        self.cs = np.concatenate([[0.0], np.cumsum(host)])

    def fold(self, i, got, o, pos=None):
        m = got.shape[0]
        if not m:
            return
        ref = self.ref[o:o + m]
        assert ref.shape == got.shape, (ref.shape, got.shape, o)
        self.n += got.numel()
        self.host_sum += self.cs[o + m] - self.cs[o]
        self.starts[i] = pos
        if self.fmt == "f32":
            d = (got.double() - ref.double()).abs()
            self.percall[i] = (d / self.ulp[o:o + m].double()).max()
            self.sq += (d * d).sum()
            self.ne += (got.view(torch.int32) != ref.view(torch.int32)).sum()
        elif self.fmt == "f64":
            d = (got - ref).abs()
            self.percall[i] = d.max()
            self.sq += (d * d).sum()
            self.ne += (got != ref).sum()
        else:
            d = got.int() - ref.int()
            nz = d != 0
            self.percall[i] = d.abs().max().double()
            self.ne += nz.sum()
            self.unexcused += (nz & ~self.tie[o:o + m]).sum()

    def report(self):
        torch.cuda.synchronize()
        pc = self.percall.cpu().numpy()
        rep = {"n": self.n, "bit_equal_frac": 1.0 - int(self.ne) / max(self.n, 1)}
        if self.fmt == "f32":
            rep["max_ulp"], bar = float(pc.max()), 1.0
            rep["rel_rms"] = float(np.sqrt(float(self.sq) / max(self.n, 1)) / max(np.sqrt(self.host_sum / max(self.n, 1)), ULP_FLOOR))
        elif self.fmt == "f64":
            rep["e"], bar = float(pc.max()) / self.scale, 1e-13 * self.scale
            rep["rel_rms"] = float(np.sqrt(float(self.sq) / max(self.n, 1)) / self.scale)
        else:
            rep["max_abs_d"], bar = int(pc.max()), 1
            rep.update(differing=int(self.ne), unexcused=int(self.unexcused), in_window=int(round(self.host_sum)))
        bad = np.nonzero(pc > bar)[0]
        if bad.size:  # where the error first rises: the call, and the output position it began at
            rep["first_bad_call"], rep["first_bad_pos"] = int(bad[0]), self.starts.get(int(bad[0]))
        return rep

    def check(self, rep, what):
        assert rep["n"] > 0, what
        if self.fmt == "f32":
            assert rep["max_ulp"] <= 1.0 and rep["rel_rms"] <= 1e-7, (what, rep)
        elif self.fmt == "f64":
            assert rep["e"] <= 1e-13, (what, rep)
        else:
            try:
                assert_tie_rule(rep["n"], rep["in_window"], rep["max_abs_d"], rep["differing"], rep["unexcused"])
            except AssertionError as e:
                raise AssertionError((what, rep)) from e


def open_handle(case):
    r = F.Resampler(case.fi, case.fo, nch=case.nch, **OPEN[case.fmt], **case.kw)
    r.set_stream(torch.cuda.current_stream().cuda_stream)  # one stream for the handle and the comparison: no sync per push
    return r


def first_push_kernels(r, push):
    """the kernel names of one push, from the handle's own profile records"""
    r.profile(True)
    res = push()
    names = sorted({k["kernel"] for k in r.profile_report()})
    r.profile(False)
    return res, names


def assert_families(case, names):
    for fam in case.families:
        assert any(fam in k for k in names), (case.id, fam, names)


@pytest.mark.parametrize("cid", [c for c in FC.RATIONAL if c != "host"])
def test_far_positions(cid):
    """n_far pushes of one buffer through flow_device; every call compared with R by position on the device; the drained total
    is n_far * Wo exactly and the drained tail is the oracle's; the handle's own first window [Wo, 2Wo) is asserted apart, so
    that a failure far out can be told from a failure at the start."""
    t0 = time.perf_counter()
    case, ref = FC.BY_ID[cid], FC.reference(cid)
    geo = ref.geo
    Wi, Wo, n_far, nch = geo.Wi, geo.Wo, geo.n_far, case.nch
    r = open_handle(case)
    assert r.isamp_max == geo.isamp_max
    xin = torch.from_numpy(np.array(ref.x_handle)).cuda()  # (a copy: the shared reference is read-only)
    cap = 2 * Wo  # a call gives Wo frames give or take a block; slack: another Wo
    out = torch.zeros((cap, nch), dtype=TDT[case.fmt], device="cuda")
    far = Fold(case.fmt, np.tile(ref.R, (3, 1)), n_far)
    first = Fold(case.fmt, ref.R, n_far, scale=getattr(far, "scale", None))
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    pos = 0
    for i in range(n_far):
        if i == 0:
            (iu, m), names = first_push_kernels(r, lambda: r.flow_device(xin, Wi, out, cap))
        else:
            iu, m = r.flow_device(xin, Wi, out, cap)  # (the return code is checked inside: a host integer, no sync)
        assert iu == Wi and m < cap, (i, iu, m)
        a = max(pos, Wo)  # R speaks for positions from Wo on
        if pos + m > a:
            far.fold(i, out[a - pos:m], (a - Wo) % Wo, pos)
            if a < 2 * Wo:
                first.fold(i, out[a - pos:min(pos + m, 2 * Wo) - pos], a - Wo, pos)
        pos += m
    r.drain()
    og = r.pull_device(out, cap)
    tail = Fold(case.fmt, ref.y[3 * Wo - og:], 1, scale=getattr(far, "scale", None)) if 0 < og <= Wo else None
    if tail:
        tail.fold(0, out[:og], 0, pos)  # same phase as the oracle's drained tail: n_far * Wo = 3 Wo = 0 (mod Wo)
    r.sync()
    rep, rep1 = far.report(), first.report()
    rept = tail.report() if tail else None
    t2 = time.perf_counter()
    r.close()
    print("far %s: n_far %d Wi %d Wo %d seconds %.2f (pushes %.2f) far %s | first window %s | tail %d frames %s | kernels %s"
          % (cid, n_far, Wi, Wo, t2 - t0, t2 - t1, rep, rep1, og, rept, " ".join(names)))
    assert_families(case, names)
    assert pos + og == n_far * Wo, (pos, og, n_far * Wo)
    assert min(geo.counts) > case.limit and pos > case.limit
    first.check(rep1, "the handle's own frames [Wo, 2Wo) against R")
    assert rep1["n"] == Wo * nch
    far.check(rep, "every call against R by position")
    assert rep["n"] == (pos - Wo) * nch
    assert tail is not None, og
    tail.check(rept, "the drained tail against the oracle's")


def test_far_interp():
    """44100 -> 48001: the 32.32 clock.  Input 0.5 sin, a whole number of cycles per buffer near fi / 8; reference
    a sin(w t_j) + b cos(w t_j) on the stage's own grid t_j = (at0 + j step) / (2^32 F), a and b fitted on the oracle's fresh
    output, whose largest residual r_o is the measurement.  All calls of the last 64 pushes, of the 64 pushes around each of
    output index 2^31 and 2^32 and input index 2^31 and 2^32, and pushes 1 .. 3 must stay within 4 r_o (float32 rounding of
    other samples); a slip of one input frame is an error of 0.38.  The drained total is the reference's rate_flush count.
    Measured: r_o = 3.745e-08 (rms 1.014e-08) on the oracle, 4.063e-08 (rms 1.015e-08) on the GPU over the 259 checked calls."""
    t0 = time.perf_counter()
    case = FC.BY_ID["interp"]
    geo, ig, x, a, b, r_o, r_o_rms = FC.interp_reference()
    Wi, n_far = geo.Wi, geo.n_far
    per_push = Wi * float(geo.rates[-1])
    checked = set(range(1, 4)) | set(range(n_far - 64, n_far))
    crossings = {"in 2^31": (1 << 31) // Wi, "in 2^32": (1 << 32) // Wi, "out 2^31": int((1 << 31) / per_push), "out 2^32": int((1 << 32) / per_push)}
    for p in crossings.values():
        checked |= set(range(p - 32, p + 32))
    checked = {c for c in checked if 1 <= c < n_far}  # (input index 2^32 is passed inside the last 64 pushes)
    assert all(1 <= p < n_far for p in crossings.values()), crossings
    r = open_handle(case)
    xin = torch.from_numpy(np.array(x)).cuda()
    cap = int(per_push) + 65536
    out = torch.zeros((cap, 1), dtype=torch.float32, device="cuda")
    T0, T1 = (torch.from_numpy(t).cuda() for t in FC.interp_phase_tables(ig))
    nlo = T0.shape[0]
    assert cap <= nlo * nlo
    k = torch.arange(cap, dtype=torch.int64, device="cuda")
    k1, k0 = k // nlo, k % nlo
    percall = torch.zeros(n_far, dtype=torch.float64, device="cuda")
    sq = torch.zeros((), dtype=torch.float64, device="cuda")
    nres, starts, spans = 0, {}, []
    torch.cuda.synchronize()
    pos = 0
    for i in range(n_far):
        if i == 0:
            (iu, m), names = first_push_kernels(r, lambda: r.flow_device(xin, Wi, out, cap))
        else:
            iu, m = r.flow_device(xin, Wi, out, cap)
        assert iu == Wi and m < cap, (i, iu, m)
        if i in checked and m:
            rr = (FC.interp_phase_base(ig, pos) + T1[k1[:m]] + T0[k0[:m]]) % ig.period  # j * step in integers, reduced
            ph = rr.double() * (2.0 * np.pi / ig.period)
            res = (out[:m, 0].double() - (a * torch.sin(ph) + b * torch.cos(ph))).abs()
            percall[i] = res.max()
            sq += (res * res).sum()
            nres += m
            starts[i] = pos
            spans.append((pos, pos + m))
        pos += m
    r.drain()
    og = r.pull_device(out, cap)
    r.sync()
    torch.cuda.synchronize()
    pc = percall.cpu().numpy()
    r_g, r_g_rms = float(pc.max()), float(np.sqrt(float(sq) / nres))
    bad = np.nonzero(pc > 4 * r_o)[0]
    first_bad = (int(bad[0]), starts[int(bad[0])]) if bad.size else None
    r.close()
    print("far interp: n_far %d Wi %d seconds %.2f r_o %.3e (rms %.3e) r_gpu %.3e (rms %.3e) over %d calls, first bad (call, pos) %s, "
          "total %d, kernels %s" % (n_far, Wi, time.perf_counter() - t0, r_o, r_o_rms, r_g, r_g_rms, len(spans), first_bad, pos + og, " ".join(names)))
    assert_families(case, names)
    for X in (1 << 31, 1 << 32):  # the output crossings lie inside checked calls
        assert any(lo <= X < hi for lo, hi in spans), X
    assert pos > case.limit
    assert r_g <= 4 * r_o, (r_g, r_o, first_bad)
    factor = F.describe_plan(case.fi, case.fo, **case.kw)["factor"]
    assert pos + og == int(float(n_far * Wi) / factor + .5), (pos, og)


def test_far_host():
    """RR_push / RR_pull with the page-locked host mirror across the four crossings (input and output index 2^31 and 2^32): the
    handle moves by flow_device, and the four buffers around each crossing -- one before it, the one it lies in, two behind -- go
    through Resampler.push / pull_all in twelfths of the buffer, small enough for the push to be read in place and its output
    mirrored, so that the mirror's own range crosses too.  Those host arrays are held to R by position."""
    t0 = time.perf_counter()
    case, ref = FC.BY_ID["host"], FC.reference("host")
    geo = ref.geo
    Wi, Wo, nch = geo.Wi, geo.Wo, case.nch
    parts = 12
    sub = Wi // parts
    assert sub * parts == Wi
    assert sub * nch * 4 <= 1 << 20 and (sub * Wo // Wi + 4096) * nch * 4 <= 1 << 20  # a push and its output fit the in-place path
    crossings = {"in 2^31": (1 << 31) // Wi, "out 2^31": (1 << 31) // Wo, "in 2^32": (1 << 32) // Wi, "out 2^32": (1 << 32) // Wo}
    host = set()
    for p in crossings.values():
        host |= {p - 1, p, p + 1, p + 2}
    n = max(geo.n_far, max(host) + 1)
    r = open_handle(case)
    xin = torch.from_numpy(np.array(ref.x_handle)).cuda()  # (a copy: the shared reference is read-only)
    cap = 2 * Wo
    out = torch.zeros((cap, nch), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    R32 = ref.R.astype(np.float32)
    pos, spans, worst = 0, [], {"max_ulp": 0.0, "rel_rms": 0.0, "bit_equal_frac": 1.0}
    for i in range(n):
        if i not in host:
            iu, m = r.flow_device(xin, Wi, out, cap)
            assert iu == Wi and m < cap, (i, iu, m)
            pos += m
            continue
        for k in range(parts):
            r.push(ref.x_handle[k * sub:(k + 1) * sub])
            y = r.pull_all()
            m = y.shape[0]
            assert m > 0 and pos > Wo
            want = R32[(pos - Wo + np.arange(m)) % Wo]
            rep = assert_parity(y, want)
            worst = {"max_ulp": max(worst["max_ulp"], rep["max_ulp"]), "rel_rms": max(worst["rel_rms"], rep["rel_rms"]),
                     "bit_equal_frac": min(worst["bit_equal_frac"], rep["bit_equal_frac"])}
            spans.append((i * Wi + k * sub, i * Wi + (k + 1) * sub, pos, pos + m))
            pos += m
    r.drain()
    tail = r.pull_all()
    r.close()
    print("far host: pushes %d (%d by the host, in %d parts each) seconds %.2f worst %s" % (n, len(host), parts, time.perf_counter() - t0, worst))
    assert pos + tail.shape[0] == n * Wo
    for X in (1 << 31, 1 << 32):  # both crossings of both indices lie inside host calls
        assert any(a <= X < b for a, b, _, _ in spans), ("in", X)
        assert any(c <= X < d for _, _, c, d in spans), ("out", X)
