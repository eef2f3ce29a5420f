"""CPU-only: the product's host side (planner + filter design, C++) against the independent oracle
restatement and against the reference-run facts of SURVEY.md; and the C-ABI surface."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import foo_dsp_resampler_amd as F
from oracle_binding import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the plugin's rate list (dsp_config.cpp:22)
RATES = [8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 64000, 88200, 96000, 176400, 192000]


def test_library_exports_every_declared_symbol():
    assert F.available_symbols() == F.EXPECTED_SYMBOLS
    declared = set()
    for h in ("ratelib.h", "ratelib_amd.h"):
        txt = open(os.path.join(ROOT, "include", h)).read()
        txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
        txt = re.sub(r"^\s*#define.*$", "", txt, flags=re.M)   # macros (RRX_STREAM_OWN) are not exported symbols
        declared |= set(re.findall(r"\b((?:RRX?_|init_|close_)[A-Za-z_]+)\s*\(", txt))
    assert declared == set(F.EXPECTED_SYMBOLS), declared ^ set(F.EXPECTED_SYMBOLS)


def test_strerror_strings():
    L = F.lib()
    want = {0: "OK", 1: "Not enough memory", 2: "Internal error", 3: "NULL handle", 4: "Error in rate() functions",
            5: "Externals not initialized", 6: "Other error", 99: "Other error"}  # rate_uni.c:92-111
    for k, v in want.items():
        assert L.RR_strerror(k).decode() == v


def test_null_and_uninitialised_handling_without_gpu():
    L = F.lib()
    assert L.RR_push(None, None, 0) == 3 and L.RR_drain(None) == 3 and L.RR_pull(None, None, 0, None) == 3
    L.RR_close(None)
    h = C.c_void_p()
    L.RR_close(C.byref(h))
    cfg = F.RRConfig(44100, 48000, 50.0, 95.0, 0, 0)
    assert L.RR_open(C.byref(cfg), 2, None) == 6  # RR_INVPARAM, rate_uni.c:31
    assert L.init_ratelib(F.ratelib._ALLOC_CB()) == -1  # NULL handler, rate_uni.c:215


def plan_key(s):
    keys = {"dft": ["L", "step_int", "num_taps", "dft_length", "post_peak", "preload", "remL"],
            "poly": ["L", "step", "at", "n", "interp_order", "preload", "pre_post"],
            "half": ["n", "pre", "pre_post", "preload"]}[s["kind"]]
    if s["kind"] == "poly" and s["interp_order"] > 0:
        keys = keys + ["phase_bits"]
    return (s["kind"],) + tuple(s[k] for k in keys)


def check_against_oracle(fi, fo, tables=True, **kw):
    got = F.describe_plan(fi, fo, **kw)
    o = Oracle(fi, fo, 1, **kw)
    want = o.plan()
    assert got["isamp_max"] == o.isamp_max
    assert [plan_key(s) for s in got["stages"]] == [plan_key(s) for s in want], (fi, fo, kw)
    if tables:
        for which in (0, 1):
            a, b = F.plan_table(which, fi, fo, **kw), o.dft_taps(which)
            assert a.shape == b.shape
            if a.size:
                # Linear phase: same libm formulas on both sides -> identical bits.  Other phases go through the cepstral
                # minimum-phase construction (effects_i_dsp.c:181-278): log|H| of a -180 dB stop band amplifies the rounding
                # of whichever FFT produced the spectrum by ~1e9.  Both sides run that first transform in binary128 and the
                # rest in long double, with transforms of different structure: they agree to a few fp64 ulps of the peak
                # tap (fp64 on both sides: ~1e-7 ... 3e-6; long double alone: 1e-10 ... 9e-8).
                tol = 0 if kw.get("phase", 50.0) == 50.0 else 1e-15
                assert np.max(np.abs(a - b)) <= tol * max(1.0, np.max(np.abs(b))), (fi, fo, kw, which)
        a, b = F.plan_table(2, fi, fo, **kw), o.poly_table()
        assert a.shape == b.shape and (a.size == 0 or np.array_equal(a, b)), (fi, fo, kw)


@pytest.mark.parametrize("fi,fo", [(a, b) for a, b in itertools.product(RATES, RATES) if a != b])
def test_rate_matrix_plans_match_oracle(fi, fo):
    check_against_oracle(fi, fo, tables=False)


@pytest.mark.parametrize("fi,fo", [(44100, 48000), (44100, 96000), (44100, 192000), (96000, 44100), (192000, 44100),
                                   (88200, 44100), (44100, 48001), (48000, 44100), (32000, 96000), (48000, 32000),
                                   (8000, 192000), (192000, 8000), (44100, 44100), (11025, 44100), (96000, 32000)])
@pytest.mark.parametrize("kw", [dict(), dict(bandwidth=99.0), dict(bandwidth=90.0, allow_aliasing=1), dict(quality=1),
                                dict(phase=0.0), dict(phase=25.0), dict(phase=75.0), dict(phase=100.0)])
def test_tables_match_oracle(fi, fo, kw):
    check_against_oracle(fi, fo, **kw)


def test_phase_tables_agree_in_extended_precision():
    """phase != 50: product (design.cpp: first transform in binary128 by decimation in time, the rest in long double) against
    oracle (rate_oracle.c: the same precisions, decimation in frequency, twiddles from series): <= 1e-15 of the peak tap, i.e. the
    two tables differ by an fp64 ulp here and there.  The oracle's fp64 statement of the same function, which follows the
    reference line by line (orc_set_phase_arith(1)), differs from either by 3e-7 ... 3e-6: the reference's own
    irreproducibility, the reason phase != 50 is "parity unpinned" against the reference itself however well product and
    oracle agree."""
    import ctypes
    import oracle_binding
    L = oracle_binding.lib()
    L.orc_set_phase_arith.argtypes = [ctypes.c_int]
    worst_ld, worst_64, worst_64_steep = 0.0, 0.0, 0.0
    for fi, fo, kw in [(44100, 48000, {}), (44100, 96000, {}), (96000, 44100, {}), (44100, 192000, {"bandwidth": 99.0}),
                       (192000, 11025, {"bandwidth": 99.0})]:
        for phase in (0.0, 10.0, 25.0, 75.0, 100.0):
            a = F.plan_table(0, fi, fo, phase=phase, **kw)
            b = Oracle(fi, fo, 1, phase=phase, **kw).dft_taps(0)
            L.orc_set_phase_arith(1)
            try:
                c = Oracle(fi, fo, 1, phase=phase, **kw).dft_taps(0)
            finally:
                L.orc_set_phase_arith(0)
            assert a.shape == b.shape == c.shape
            pk = np.max(np.abs(b))
            worst_ld = max(worst_ld, np.max(np.abs(a - b)) / pk)
            if kw:
                worst_64_steep = max(worst_64_steep, np.max(np.abs(b - c)) / pk)
            else:
                worst_64 = max(worst_64, np.max(np.abs(b - c)) / pk)
    assert worst_ld <= 1e-15, worst_ld  # (2e-18 ... 5e-17 measured, the 4981-tap filter of 192k->11.025k at 99 % included)
    assert 1e-8 < worst_64 <= 1e-5, worst_64  # the fp64 construction really is that loose at the default passband ...
    # ... and at a 99 % passband with an intermediate phase it is not a function of its input any more: the stop-band bins of
    # the 2845-tap filter are rounding noise in fp64, their phase "wraps" are counted into the blend (effects_i_dsp.c:206-240),
    # and the fp64 result differs from the extended-precision one by a third of the peak tap (4e-5 at phase 0 / 100)
    assert worst_64_steep > 1e-5, worst_64_steep


def test_survey_facts(facts):
    for key, want in facts["plans"].items():
        if key.startswith("_"):
            continue
        c = facts["configs"][key]
        got = F.describe_plan(c["in_rate"], c["out_rate"], phase=c["phase"], bandwidth=c["bandwidth"],
                              allow_aliasing=c["allow_aliasing"], quality=c["quality"])["stages"]
        assert len(got) == len(want)
        for g, w in zip(got, want):
            for k, v in w.items():
                if k.startswith("_"):
                    continue
                if k == "step_fraction_u32_as_printed":
                    assert "%.8f" % ((g["step"] & 0xFFFFFFFF) / 1e10) == "0." + v
                else:
                    assert g[k] == v, (key, k, g, w)
    for key, want in facts["design_calls"].items():
        if key.startswith("_"):
            continue
        c = facts["configs"][key]
        got = F.describe_plan(c["in_rate"], c["out_rate"], bandwidth=c["bandwidth"])["design_calls"]
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g["k"] == w["k"] and g["num_taps"] == w["num_taps"]
            assert abs(g["Fp"] - w["Fp"]) < 1e-10 and abs(g["Fn"] - w["Fn"]) < 1e-9 and abs(g["att"] - w["att"]) < 1e-5
    assert F.describe_plan(44100, 96000)["isamp_max"] == facts["scalars"]["isamp_max_cfg2"]


def test_bad_ratio_is_rejected():
    with pytest.raises(F.RRError):
        F.describe_plan(1, 6000)  # factor < 1/5644.8, rate_base.h:528
    with pytest.raises(F.RRError):
        F.describe_plan(6000, 1)


def test_product_never_touches_the_oracle():
    """The oracle is test infrastructure: nothing under the product package or include/ may name it."""
    import glob
    offenders = []
    for pat in ("foo_dsp_resampler_amd/**/*.py", "foo_dsp_resampler_amd/csrc/*", "include/*.h"):
        for path in glob.glob(os.path.join(ROOT, pat), recursive=True):
            if os.path.isfile(path) and not path.endswith((".so", ".o")):
                txt = open(path, errors="ignore").read()
                if "oracle" in txt.lower():
                    offenders.append(os.path.relpath(path, ROOT))
    assert offenders == []


def test_no_cpu_fallback_without_a_gpu():
    """Without a HIP device the library must refuse to initialise (there is no CPU path to fall back to)."""
    import subprocess, sys
    code = (
        "import sys, ctypes as C; sys.path.insert(0, %r)\n"
        "import foo_dsp_resampler_amd as F\n"
        "L = F.lib(); cb = F.ratelib._ALLOC_CB(lambda: None)\n"
        "rc = L.init_ratelib(cb); h = C.c_void_p(); cfg = F.RRConfig(44100, 48000, 50.0, 95.0, 0, 0)\n"
        "print(rc, L.RR_open(C.byref(cfg), 2, C.byref(h)), bool(h.value))\n" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))
    assert out.returncode == 0, out.stderr
    rc, op, has = out.stdout.split()[-3:]
    assert rc == "-1" and op == "5" and has == "False"   # RR_EXTUNINIT, no handle


def test_open_without_a_device_is_refused_and_runs_no_handler():
    """No usable gfx950 device: init_ratelib refuses (-1), RR_open answers RR_EXTUNINIT (rate_uni.c:31-53) and the
    allocation handler is NOT invoked (nothing was allocated).  With a GPU this case cannot arise, so it is skipped."""
    import ctypes as C
    import foo_dsp_resampler_amd.ratelib as R
    L = F.lib()
    calls = []
    cb = R._ALLOC_CB(lambda: calls.append(1))
    if L.init_ratelib(cb) == 0:
        L.init_ratelib(R._alloc_cb)
        pytest.skip("a gfx950 device is present")
    cfg = F.RRConfig(44100, 96000, 50.0, 95.0, 0, 0)
    h = C.c_void_p(0x55)
    assert L.RR_open(C.byref(cfg), 2, C.byref(h)) == 5 and not h.value
    assert L.RRX_open_batch(C.byref(cfg), 2, 1 << 21, C.byref(h)) == 5 and not h.value
    assert not calls


def test_bench_config_table_matches_baseline_json():
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert sorted(bench.CONFIGS) == list(range(len(base["configs"])))
    want = {0: (44100, 48000, 2), 1: (44100, 96000, 2), 2: (44100, 192000, 8), 3: (96000, 44100, 32), 4: (44100, 48000, 2)}
    for k, (fi, fo, nch) in want.items():
        c = bench.CONFIGS[k]
        assert (c["fi"], c["fo"], c["nch"]) == (fi, fo, nch)
    assert bench.CONFIGS[2]["kw"]["bandwidth"] == 99.0 and bench.CONFIGS[4]["streams"] == 1024 and bench.CONFIGS[4]["total"]
    # fp64 work per unit of the headline chain (~212 flop per input sample)
    fl = bench.chain_flops_per_unit(F.describe_plan(44100, 96000), 44100)
    assert 205 < fl < 220


@pytest.mark.parametrize("fi,fo", [(8000, 352800), (8000, 705600), (8000, 2822400)])
def test_planner_agrees_with_oracle_on_large_upsampling(fi, fo):
    """pow2 L >= 8 DFT stages: the product's plan equals the oracle's."""
    from oracle_binding import Oracle
    plan = F.describe_plan(fi, fo)["stages"]
    ref = Oracle(fi, fo, 1).plan()
    assert [s["kind"] for s in plan] == [s["kind"] for s in ref]
    for a, b in zip(plan, ref):
        if a["kind"] == "dft":
            assert (a["L"], a["step_int"], a["num_taps"], a["dft_length"]) == (b["L"], b["step_int"], b["num_taps"], b["dft_length"])


def test_experiment_switches_cannot_reach_the_product_build():
    """The wrong-result timing switches are gone from the sources, not merely guarded: no file the library or its tools are
    built from names one (comments included), the Makefile sets none, and defining one changes nothing for knobs.hpp."""
    import glob
    import subprocess
    csrc = os.path.join(ROOT, "foo_dsp_resampler_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "-DRSMP_EXPERIMENTS" not in "\n".join(ln for ln in mk.splitlines() if not ln.lstrip().startswith("#"))
    assert "RSMP_EXP_" not in "\n".join(ln for ln in mk.splitlines() if not ln.lstrip().startswith("#"))
    names = ("RSMP_EXP", "RSMP_DBG", "RSMP_DFTX_SKIP", "RSMP_VCONST", "RSMP_EXPERIMENTS")
    files = [p for p in glob.glob(os.path.join(csrc, "*")) if p.endswith((".cpp", ".hip", ".hpp")) or os.path.basename(p) == "Makefile"]
    files += [p for p in glob.glob(os.path.join(ROOT, "tools", "**", "*"), recursive=True) if os.path.isfile(p) and not p.endswith(".md")]
    assert len(files) > 20
    hits = []
    for path in files:
        text = open(path, errors="replace").read()
        hits += ["%s: %s" % (os.path.relpath(path, ROOT), nm) for nm in names if nm in text]
    assert not hits, hits
    src = '#include "knobs.hpp"\nint main() { return int(sizeof(rsmp::Knobs)) == 0; }\n'
    def compiles(flags):
        return subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", csrc, "-x", "c++", "-"] + flags, input=src, text=True,
                              capture_output=True).returncode == 0
    assert compiles([])
    assert compiles(["-DRSMP_EXP_TAB=1"])                            # the name means nothing to the library any more


def test_environment_is_read_once():
    """No getenv on the launch path: the only reads are the one-time knobs() initialiser (engine.cpp) and init_ratelib's
    RATELIB_AMD_DEVICES (capi.cpp)."""
    import glob
    import re
    hits = []
    for path in glob.glob(os.path.join(ROOT, "foo_dsp_resampler_amd", "csrc", "*")):
        if path.endswith((".cpp", ".hip", ".hpp")):
            for n, ln in enumerate(open(path), 1):
                if re.search(r"\bgetenv\s*\(", ln) and not ln.lstrip().startswith("//"):
                    hits.append((os.path.basename(path), n))
    assert {f for f, _ in hits} <= {"engine.cpp", "capi.cpp"}, hits
    assert len([1 for f, _ in hits if f == "capi.cpp"]) == 1, hits


# ------------------------------------------------------------------------------------------------ sub-blocked dispatch (host side)
_SPLIT_RATES = [(44100, 48000), (44100, 96000), (44100, 192000), (48000, 44100), (22050, 64000), (8000, 44100), (11025, 64000),
                (44100, 88200), (96000, 44100), (32000, 44100), (44100, 64000), (16000, 88200)]


@pytest.mark.parametrize("bw", [90.0, 95.0, 97.0, 98.0, 99.0, 99.5, 99.7])
def test_sub_blocked_geometry_covers_each_block_exactly_and_stays_valid(bw):
    """RRX_describe_dispatch (host-only): for every chain the sub-blocked fused kernels would take, the sub-blocks tile the
    block's V valid samples without gap or overlap, have even lengths, read only inputs of the block's own span, and every
    sample lies where the two 4096-point component transforms are free of wrap-around (2 shift + len + taps - 1 <= 8192).
    The whole-block two-round form is chosen exactly for 8192-point blocks; chains the kernels do not cover are left alone."""
    seen = {"sub": 0, "two": 0, "plain": 0}
    for fi, fo in _SPLIT_RATES:
        st = F.describe_plan(fi, fo, bandwidth=bw)["stages"]
        for nch in (1, 2, 3, 6, 8):
            d = F.describe_dispatch(fi, fo, nch, bandwidth=bw)
            shaped = (len(st) >= 2 and st[0]["kind"] == "dft" and st[0]["L"] == 2 and st[0]["dft_length"] in (8192, 16384, 32768)
                      and st[1]["kind"] == "poly" and st[1]["interp_order"] == 0 and st[1]["L"] >= 64)
            if not d["sub_blocked"]:
                seen["plain"] += 1
                assert not (shaped and nch % 2 == 0), (fi, fo, bw, nch, st[0])  # every chain of this shape with an even channel count is covered
                continue
            assert shaped and nch % 2 == 0, (fi, fo, bw, nch)
            V, taps, N, Pref = d["V"], d["taps"], d["N"], d["Pref"]
            assert N == st[0]["dft_length"] and taps == st[0]["num_taps"] and V == N - (taps - 1) and Pref == N // 2
            sbs = d["sub_blocks"]
            assert len(sbs) == d["nsub"] >= 1
            pos = 0
            for sb in sbs:
                assert sb["off"] == pos and sb["len"] > 0 and sb["len"] % 2 == 0 and sb["off"] % 2 == 0
                assert 0 <= sb["win"] <= Pref - 4096 and sb["shift"] == sb["off"] // 2 - sb["win"] >= 0
                assert 2 * sb["shift"] + sb["len"] + (taps - 1) <= 8192, (fi, fo, bw, sb)
                pos += sb["len"]
            assert pos == V
            if d["two_round"]:
                seen["two"] += 1
                assert N == 8192 and d["nsub"] == 1 and d["Vs"] == V > 5056
            else:
                seen["sub"] += 1
                assert d["Vs"] <= 5056 and all(sb["len"] <= d["Vs"] for sb in sbs)
    if bw in (97.0, 98.0):
        assert seen["two"] > 0, seen
    if bw in (99.0, 99.5):
        assert seen["sub"] > 0, seen
    if bw in (90.0, 95.0, 99.7):
        assert seen["sub"] == seen["two"] == 0, seen  # 4096-point blocks are the lean kernel's; 65536-point ones stay four-step
