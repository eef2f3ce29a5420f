"""Streams held to the oracle past 2^31 and 2^32 frames of absolute position: the case table and its helpers.

Every stage of the engine works on absolute stream positions -- 64-bit on the host, narrowed in the kernels wherever the
operand is a difference.  A narrowing of something that is not a difference shows only once a position passes 2^31 or 2^32,
hours into a stream.  The tests of tests/test_gpu_far_positions.py run that distance; this module says what they run and
what the right answer is, and tests/test_far_cases_api.py pins the premise below on the oracle alone.

The premise.  A chain without an interpolated stage changes the rate by an exact rational.  With g = gcd(fi, fo), an input
that repeats every Wi = K * fi / g frames gives, after the start-up transient, an output that repeats every Wo = K * fo / g
frames: bit for bit in float32 on seven of the nine chains here, and to 0.25 ulp on one sample in a million on the other two
(96000 -> 44100 and 24000 -> 8000: FFT blocks are anchored at absolute positions, so a sample falls elsewhere in its block one
period on; tests/test_far_cases_api.py measures it).  The reference for ANY output position p >= Wo is therefore frame
Wo + (p - Wo) % Wo of a fresh oracle stream: its window R = y[Wo:2Wo].

The interpolated chain (44100 -> 48001) runs a 32.32 clock whose step is rounded: its ratio is step / 2^32, not fo / fi, and
its output is not periodic.  Its reference is analytic: a sine in, the same sine out on the grid t_j = (at0 + j * step) / (2^32 F)
(interp_times), with amplitude and phase fitted once on the oracle's fresh output.

Wall times (MI355X, one stream, whole test with its reference): beside each case, `seconds`."""
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

from oracle_binding import Oracle, lcg_noise

Case = namedtuple("Case", "id fi fo nch fmt kw limit families dispatch seconds")
# fmt: "f32" | "f64" | "s16".  limit: the position every fifo index must pass (2^32; 2^31 for a case that would take more than
# 10 s to 2^32).  families: substrings of the kernel names the first push must launch (the handle's own profile records).
# dispatch: what RRX_describe_plan / RRX_describe_dispatch must say of the chain (host-only; test_far_cases_api.py):
# stage kinds with the block length of every dft stage, then sub_blocked / nsub / two_round of the first stage pair.
BW99 = {"bandwidth": 99.0}
CASES = [
    Case("up", 44100, 96000, 2, "f32", {}, 1 << 32, ["rsmp::fused_fast_kernel<"],
         ([("dft", 4096), ("poly", 0)], False, 0, False), 2.3),
    Case("down", 96000, 44100, 2, "f32", {}, 1 << 32, ["rsmp::fused_fast_kernel<"],
         ([("dft", 4096), ("poly", 0)], False, 0, False), 1.6),
    Case("x4", 44100, 192000, 2, "f32", BW99, 1 << 32, ["rsmp::fused_split_kernel<", "rsmp::dftx_kernel<4>"],
         ([("dft", 16384), ("poly", 0), ("dft", 8192)], True, 3, False), 3.9),
    Case("half", 192000, 44100, 2, "f32", {}, 1 << 32, ["rsmp::half_kernel<"],
         ([("half", 0), ("dft", 4096), ("poly", 0)], False, 0, False), 3.0),
    Case("odd", 44100, 48000, 3, "f32", {}, 1 << 32, ["rsmp::fused_kernel<", "rsmp::seam_kernel"],
         ([("dft", 4096), ("poly", 0)], False, 0, False), 1.8),
    Case("f64", 44100, 48000, 2, "f64", {"phase": 25.0}, 1 << 32, ["_dio_kernel<"],
         ([("dft", 8192), ("poly", 0)], True, 1, True), 1.3),
    Case("s16", 44100, 96000, 2, "s16", {}, 1 << 32, ["rsmp::fused_fast_s16_kernel<"],
         ([("dft", 4096), ("poly", 0)], False, 0, False), 2.0),
    Case("long", 24000, 8000, 2, "f32", BW99, 1 << 32, ["big_cols_fwd_kernel"],
         ([("dft", 32768)], False, 0, False), 3.0),
    Case("interp", 44100, 48001, 1, "f32", {}, 1 << 32, ["rsmp::polyi_kernel<3>"],
         ([("dft", 4096), ("poly", 3)], False, 0, False), 1.6),
    Case("host", 44100, 96000, 2, "f32", {}, 1 << 32, ["rsmp::fused_fast_kernel<"],
         ([("dft", 4096), ("poly", 0)], False, 0, False), 1.0),
]
BY_ID = {c.id: c for c in CASES}
RATIONAL = [c.id for c in CASES if c.id != "interp"]
SEEDS = {c.id: 7001 + k for k, c in enumerate(CASES)}


def stage_ratios(plan):
    """out / in of every stage of Oracle.plan(), exact: a dft stage by L / step_int (zero stuffing over time-domain decimation,
    where the frequency-domain forms fold into L and step_int already), a half-band stage 1 / 2, a rational polyphase stage
    L / step_int, an interpolated one 2^32 / step."""
    out = []
    for s in plan:
        if s["kind"] == "half":
            out.append(Fraction(1, 2))
        elif s["kind"] == "poly" and s["interp_order"] > 0:
            out.append(Fraction(1 << 32, s["step"]))
        else:
            out.append(Fraction(s["L"], s["step_int"]))
    return out


def fifo_rates(plan):
    """items of every fifo (the input, between the stages, the output) per input frame, exact"""
    r = [Fraction(1)]
    for q in stage_ratios(plan):
        r.append(r[-1] * q)
    return r


Geometry = namedtuple("Geometry", "isamp_max K Wi Wo rates n_far counts")


def geometry(case):
    """Wi with the largest K such that Wi <= isamp_max, Wo, the fifo rates, the number of pushes n_far -- the first n at which
    the input count, the output count and every stage fifo's count exceed limit + Wi -- and those counts at n_far."""
    o = Oracle(case.fi, case.fo, case.nch, **case.kw)
    plan, isamp_max = o.plan(), o.isamp_max
    o.close()
    rates = fifo_rates(plan)
    if case.id == "interp":  # not periodic: the buffer is as long as a push may be, and Wo is only nominal
        K, Wi, Wo = 0, isamp_max, None
    else:
        g = math.gcd(case.fi, case.fo)
        K = isamp_max // (case.fi // g)
        Wi, Wo = K * (case.fi // g), K * (case.fo // g)
        assert rates[-1] == Fraction(case.fo, case.fi), (rates, case)
    slowest = min(rates)
    n_far = int((case.limit + Wi) / (Wi * slowest)) + 1
    while (n_far - 1) * Wi * slowest > case.limit + Wi:
        n_far -= 1
    counts = [n_far * Wi * r for r in rates]
    return Geometry(isamp_max, K, Wi, Wo, rates, n_far, counts)


def to_s16(x):
    """float noise -> 16-bit PCM, as tests/test_gpu_int_io.py::test_against_oracle makes its input"""
    return np.rint(np.asarray(x, np.float64) * 2.0 ** 15).astype(np.int16)


def input_buffer(case, Wi):
    """(what the oracle is pushed: float32 [Wi, nch]; what the handle is pushed: the case's format).  s16: the integers,
    and the oracle gets them scaled by 2^-15, which float32 holds exactly."""
    x = lcg_noise(Wi, case.nch, SEEDS[case.id]).reshape(Wi, case.nch) * np.float32(0.5)
    if case.fmt == "s16":
        s = to_s16(x)
        return (s.astype(np.float64) * 2.0 ** -15).astype(np.float32), s
    if case.fmt == "f64":
        return x, x.astype(np.float64)
    return x, x


def _take(o, nch):
    """everything the oracle has ready, as float64 [m, nch] straight from its output fifo; then pulled"""
    ns = len(o.plan())
    y = np.stack([o.stage_fifo(ch, ns) for ch in range(nch)], axis=1) if o.stage_fifo(0, ns).size else np.empty((0, nch))
    got = o.pull(y.shape[0]) if y.shape[0] else np.empty((0, nch), np.float32)
    assert got.shape[0] == y.shape[0] and np.array_equal(got, y.astype(np.float32))
    return y


Reference = namedtuple("Reference", "geo x_oracle x_handle y counts R tail")
_refs = {}


def reference(cid):
    """The oracle's run of a rational case, computed once per process and never written to: three pushes of the buffer, then a
    drain.  y: all of its output by position, float64 [3 Wo, nch] (float32 output is y.astype(float32), the oracle's own
    narrowing); counts: frames ready after each push and after the drain; R = y[Wo:2Wo]; tail: the drained frames."""
    if cid not in _refs:
        case = BY_ID[cid]
        geo = geometry(case)
        xo, xh = input_buffer(case, geo.Wi)
        o = Oracle(case.fi, case.fo, case.nch, **case.kw)
        parts = []
        for _ in range(3):
            o.push(xo)
            parts.append(_take(o, case.nch))
        o.drain()
        parts.append(_take(o, case.nch))
        o.close()
        y = np.concatenate(parts)
        for a in (xo, xh, y):
            a.setflags(write=False)
        _refs[cid] = Reference(geo, xo, xh, y, [p.shape[0] for p in parts], y[geo.Wo:2 * geo.Wo], parts[3])
    return _refs[cid]


# ---- the interpolated case ----
InterpGeo = namedtuple("InterpGeo", "at0 step F cycles period")


def interp_input(Wi, cycles):
    """0.5 * sin, `cycles` whole cycles in the buffer: every push continues the one before"""
    k = np.arange(Wi, dtype=np.int64) * cycles % Wi
    return (0.5 * np.sin(2.0 * np.pi * k.astype(np.float64) / Wi)).astype(np.float32).reshape(Wi, 1)


def interp_geometry(case, Wi):
    """the 32.32 clock of the interpolated stage (at0, step), the exact factor F of the stages in front of it, the cycles per
    buffer (near fi / 8) and the period of the phase in units of 1 / (2^32 F Wi) of a cycle ... all integers"""
    o = Oracle(case.fi, case.fo, case.nch, **case.kw)
    plan = o.plan()
    o.close()
    assert plan[-1]["kind"] == "poly" and plan[-1]["interp_order"] > 0, plan
    F = Fraction(1)
    for q in stage_ratios(plan[:-1]):
        F *= q
    assert F.denominator == 1, F
    return InterpGeo(plan[-1]["at"], plan[-1]["step"], int(F), Wi // 8, (1 << 32) * int(F) * Wi)


def interp_phase_tables(ig, lo_bits=11):
    """Phase of output j, in cycles, is cycles * (at0 + j * step) / (2^32 F Wi): j * step passes 2^64, so the product is formed
    in Python integers and reduced modulo the period before it becomes a float.  For j = j0 + k, k = 2^lo_bits * k1 + k0 the
    residue is base(j0) + T1[k1] + T0[k0] (mod period), each term below the period (< 2^53): int64 holds the sum.  Returns
    (T0, T1) as int64 arrays for k < 2^(2 lo_bits); interp_phase_base gives base(j0)."""
    s, n = ig.cycles * ig.step % ig.period, 1 << lo_bits
    assert ig.period < 1 << 53
    return (np.array([k * s % ig.period for k in range(n)], dtype=np.int64),
            np.array([(k << lo_bits) * s % ig.period for k in range(n)], dtype=np.int64))


def interp_phase_base(ig, j0):
    return ig.cycles * (ig.at0 + j0 * ig.step) % ig.period


def interp_times(ig, tables, j0, m):
    """phase of outputs [j0, j0 + m) in radians, float64 (numpy; the GPU test does the same sums in torch)"""
    T0, T1 = tables
    n = T0.shape[0]
    assert m <= n * n
    k = np.arange(m, dtype=np.int64)
    r = (interp_phase_base(ig, j0) + T1[k // n] + T0[k % n]) % ig.period
    return r.astype(np.float64) * (2.0 * np.pi / ig.period)


def interp_fit(y, ph):
    """least-squares a sin + b cos on samples y at phases ph: (a, b, largest residual, rms residual)"""
    A = np.stack([np.sin(ph), np.cos(ph)], axis=1)
    (a, b), *_ = np.linalg.lstsq(A, y.astype(np.float64), rcond=None)
    res = y.astype(np.float64) - A @ np.array([a, b])
    return float(a), float(b), float(np.abs(res).max()), float(np.sqrt(np.mean(res ** 2)))


INTERP_SKIP = 20000  # output frames left to the start-up transient before the fit (the filters span a few thousand)
_interp = {}


def interp_reference():
    """(geometry, InterpGeo, input buffer, a, b, r_o max, r_o rms): the oracle's fresh output of one push, fitted past its transient"""
    if not _interp:
        case = BY_ID["interp"]
        geo = geometry(case)
        ig = interp_geometry(case, geo.Wi)
        x = interp_input(geo.Wi, ig.cycles)
        o = Oracle(case.fi, case.fo, case.nch, **case.kw)
        o.push(x)
        y = o.pull_all()[:, 0]
        o.close()
        tabs = interp_phase_tables(ig)
        ph = interp_times(ig, tabs, INTERP_SKIP, y.shape[0] - INTERP_SKIP)
        a, b, rmax, rrms = interp_fit(y[INTERP_SKIP:], ph)
        x.setflags(write=False)
        _interp["v"] = (geo, ig, x, a, b, rmax, rrms)
    return _interp["v"]
