"""CPU checks of the knob table (tests/variants.py): the knob lists of the sources agree, every variant-selecting knob has a
row, every case plans to the stage its row is there for, and the host-side dispatch follows the knobs."""
import json
import os
import re
import subprocess
import sys

import pytest

import chain_ld
import foo_dsp_resampler_amd as F
from variants import NOT_VARIANTS, SCHEDULING, VARIANT_IDS, VARIANTS, child_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "foo_dsp_resampler_amd", "csrc")
BOUND = 1e-13
_NAME = r"((?:RSMP|RATELIB_AMD)_[A-Z0-9_]+)"
ROWS = {v[0]: v for v in VARIANTS}


def _documented():
    """The run-time names of knobs.hpp's header comment (up to its build-time part)."""
    head = open(os.path.join(CSRC, "knobs.hpp")).read().split("#pragma once")[0]
    assert "Build-time switch" in head
    return set(re.findall(r"\b" + _NAME + r"\b", head.split("Build-time switch")[0]))


def _read():
    """The names the library passes to getenv: directly, or through knobs()'s on("...") helper (engine.cpp); init_ratelib
    reads one more (capi.cpp).  test_environment_is_read_once (test_host_plan.py) holds that no other file reads any."""
    names = set()
    for f in ("engine.cpp", "capi.cpp"):
        text = open(os.path.join(CSRC, f)).read()
        if f == "engine.cpp":
            assert re.search(r"auto on = \[\]\(const char \*name\) \{ return getenv\(name\) != nullptr; \};", text)
            names |= set(re.findall(r"\bon\(\"" + _NAME + r"\"\)", text))
        names |= set(re.findall(r"\bgetenv\(\"" + _NAME + r"\"\)", text))
    return names


def test_documented_knobs_are_the_knobs_read():
    doc, read = _documented(), _read()
    assert len(read) >= 18
    assert doc == read, {"documented, never read": sorted(doc - read), "read, not documented": sorted(read - doc)}


def test_every_variant_knob_has_a_row():
    """A knob added to knobs.hpp without a row in tests/variants.py fails here (RATELIB_AMD_DEVICES places handles and selects
    no kernel: tests/test_gpu_round3.py)."""
    covered = set()
    for v in VARIANTS:
        covered |= set(v[1])
    for envs in SCHEDULING.values():
        for e in envs:
            covered |= set(e)
    want = {k for k in _read() if k.startswith("RSMP_")} - set(NOT_VARIANTS)
    assert want - covered == set(), sorted(want - covered)
    assert covered <= _read(), sorted(covered - _read())  # (a row that sets a name the library does not read tests nothing)
    for k in ("RSMP_NO_FUSE", "RSMP_NO_MFMA", "RSMP_NO_POLYMF", "RSMP_NO_FAST", "RSMP_NO_DFTX", "RSMP_NO_POLYI", "RSMP_NO_POLYCOOP",
              "RSMP_SPREAD_VECTOR", "RSMP_NO_SIDE", "RSMP_SLAB_MB"):
        assert k in covered


def test_child_environment():
    env = child_env({"PATH": "/bin", "RSMP_NO_FAST": "", "RSMP_SLAB_MB": "3", "RSMP_TEST_HOOKS": "1", "RATELIB_AMD_DEVICES": "all",
                     "RATELIB_AMD_SO": "x.so"}, {"RSMP_NO_POLYI": "1"})
    assert env == {"PATH": "/bin", "RSMP_TEST_HOOKS": "1", "RATELIB_AMD_SO": "x.so", "RSMP_NO_POLYI": "1"}


def test_table_is_well_formed():
    assert len(set(VARIANT_IDS)) == len(VARIANTS)
    known = {c[0]: c for c in chain_ld.CASES}
    for rid, env, cases, must, must_not in VARIANTS:
        ids = [c[0] for c in cases]
        assert len(set(ids)) == len(ids) and env
        for c in cases:
            assert c[7] in ("flow", "push") and (c[7] == "flow" or c[6] == 1)
            if c[0] in known:  # a shared id is the shared row: its reference comes from the same cache entry
                assert tuple(c) == tuple(known[c[0]]), (rid, c)
        for m in must:
            assert isinstance(m, str) or (m[0] in ids and len(m) in (2, 3) and all(n.startswith("rsmp::") for n in m[1:])), (rid, m)
    # one id, one chain across the rows
    seen = {}
    for v in VARIANTS:
        for c in v[2]:
            assert seen.setdefault(c[0], c[1:7]) == c[1:7], c


def _poly(case):
    st = [s for s in F.describe_plan(case[1], case[2], **case[3])["stages"] if s["kind"] == "poly"]
    assert len(st) == 1, (case, st)
    return st[0]


def _case(rid, cid):
    return [c for c in ROWS[rid][2] if c[0] == cid][0]


INTERPOLATED = {  # (row, case): (interpolation order, taps): n % 8 == 0 is what the eight-lane kernel needs
    ("no_polyi", "44k1_48001"): (3, 24), ("no_polyi", "96k_44101_norm"): (2, 16), ("no_polyi", "44k1_11027_norm"): (1, 12),
    ("no_polyi", "16k_11026"): (2, 20), ("no_polyi", "11k025_8007"): (3, 20),
    ("no_polyi_no_polycoop", "44k1_48001"): (3, 24), ("no_polyi_no_polycoop", "96k_44101_norm"): (2, 16),
    ("no_polyi_no_polycoop", "8k_8001_bw99"): (3, 28),
}


def test_interpolated_cases_plan_to_their_order_and_tap_count():
    assert {k for k in INTERPOLATED} == {(r, c[0]) for r in ("no_polyi", "no_polyi_no_polycoop") for c in ROWS[r][2]}
    for (rid, cid), (order, n) in INTERPOLATED.items():
        p = _poly(_case(rid, cid))
        assert (p["interp_order"], p["n"]) == (order, n), (rid, cid, p)
        assert n <= 32  # ... so the default build gives the stage to polyi_kernel, and only RSMP_NO_POLYI reaches these


def test_rational_table_in_lds_and_not():
    """launch_poly_stage keeps a rational stage's coefficient table in LDS up to 40 KB (engine.cpp)."""
    a, b = _poly(_case("no_fuse_no_polymf", "44k1_96k_generic")), _poly(_case("no_fuse_no_polymf", "8k_11k025"))
    assert a["interp_order"] == 0 and (a["L"], a["n"]) == (160, 24) and a["L"] * a["n"] * 8 <= 40960
    assert b["interp_order"] == 0 and (b["L"], b["n"]) == (441, 24) and b["L"] * b["n"] * 8 > 40960
    src = open(os.path.join(CSRC, "engine.cpp")).read()
    assert "tab_bytes <= 40 * 1024" in src


def test_no_dftx_cases_have_a_x4_stage_dftx_would_take():
    for c in ROWS["no_dftx"][2]:
        st = F.describe_plan(c[1], c[2], **c[3])["stages"]
        assert any(s["kind"] == "dft" and s["L"] == 4 and s["dft_length"] in (8192, 16384) for s in st), (c, st)


def test_spread_vector_cases_have_their_steps():
    """A step that is a multiple of 16 between two of a tile's four periods keeps the chain off the matrix pipe under
    RSMP_SPREAD_VECTOR (init_fused_pair): 320 and 160 do, 147 does not."""
    steps = {c[0]: _poly(c)["step_int"] for c in ROWS["spread_vector"][2]}
    assert steps == {"96k_44k1_2ch": 320, "48k_44k1": 320, "48k_88k2": 160, "44k1_96k_lean": 147}, steps
    for c in ROWS["spread_vector"][2]:
        st = F.describe_plan(c[1], c[2], **c[3])["stages"]
        assert st[0]["kind"] == "dft" and st[0]["dft_length"] == 4096 and st[1]["interp_order"] == 0 and st[1]["L"] >= 64, st
    firstL = {c[0]: F.describe_plan(c[1], c[2], **c[3])["stages"][0]["L"] for c in ROWS["spread_vector"][2]}
    assert firstL == {"96k_44k1_2ch": 1, "48k_44k1": 2, "48k_88k2": 2, "44k1_96k_lean": 2}, firstL


def test_4096_point_cases_plan_to_4096_points():
    """no_fast / no_mfma / no_fuse: the 12 000-frame chains are 4096-point blocks in front of a rational stage with enough
    phases for the matrix pipe, the 48 000-frame ones 16384-point blocks."""
    for rid in ("no_fast", "no_mfma", "no_fuse", "no_fuse_no_polymf"):
        for c in ROWS[rid][2]:
            st = F.describe_plan(c[1], c[2], **c[3])["stages"]
            assert [s["kind"] for s in st] == ["dft", "poly"] and st[1]["interp_order"] == 0 and st[1]["L"] >= 64, (c, st)
            assert st[0]["dft_length"] == (4096 if c[4] == 12000 else 16384), (c, st)


def _new_cases():
    known, out = {c[0] for c in chain_ld.CASES}, {}
    for v in VARIANTS:
        for c in v[2]:
            key = (c[1], c[2], tuple(sorted(c[3].items())), c[4], c[5] * c[6])
            if c[0] not in known and key not in out:
                out[key] = c
    return list(out.values())


@pytest.mark.parametrize("case", _new_cases(), ids=[c[0] for c in _new_cases()])
def test_new_chains_on_the_cpu(case):
    """The chains this table adds to chain_ld.CASES, as test_chain_ld.py holds those: the oracle within 1e-13 of the
    long-double model, and three blocks of the longest DFT stage before the drain."""
    _, fi, fo, kw, frames, nch, S, _ = case
    x, ld, ref, e_o, rms_o = chain_ld.case_reference(case)
    assert ref.shape == ld.shape
    print("%s e_o %.3e rms %.3e" % (case[0], e_o, rms_o))
    assert 0 < e_o <= BOUND, (e_o, rms_o)
    N, blocks = max(chain_ld.blocks_before_drain(fi, fo, kw, frames, nch * S))
    assert N >= 2048 and blocks >= 3, (N, blocks)


def _dispatch(extra):
    code = ("import sys, json; sys.path[:0] = [%r]\n"
            "import foo_dsp_resampler_amd as F\n"
            "print(json.dumps(F.describe_dispatch(44100, 48000, 2, bandwidth=99.0)))\n" % ROOT)
    p = subprocess.run([sys.executable, "-c", code], env=child_env(os.environ, extra), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_host_dispatch_follows_the_knobs():
    """RRX_describe_dispatch is host-only: 44.1k -> 48k at a 99 % passband is sub-blocked (three sub-blocks) in a clean
    environment and not under any knob that takes the sub-blocked kernel away.  A variable that is merely set counts."""
    d = _dispatch({})
    assert d["sub_blocked"] is True and d["nsub"] == 3, d
    for k, v in (("RSMP_NO_FUSE", "1"), ("RSMP_NO_MFMA", "1"), ("RSMP_NO_FAST", "1"), ("RSMP_NO_SPLIT", "1"), ("RSMP_NO_FAST", "")):
        assert _dispatch({k: v})["sub_blocked"] is False, k


def test_profile_lists_every_case():
    """profiles/fp64_parity_variants.jsonl holds the measured e_g / e_o of every case of every row, and a trailer."""
    with open(os.path.join(ROOT, "profiles", "fp64_parity_variants.jsonl")) as f:
        recs = [json.loads(ln) for ln in f if ln.strip()]
    assert recs[-1].get("trailer") and recs[-1]["lib_sha1"]
    rows = recs[:-1]
    assert sorted((r["variant"], r["case"]) for r in rows) == sorted((v[0], c[0]) for v in VARIANTS for c in v[2])
    assert all(0 < r["e_g"] <= BOUND and 0 < r["ratio"] <= 8 for r in rows)
    assert (recs[-1]["ratio_min"], recs[-1]["ratio_max"]) == (min(r["ratio"] for r in rows), max(r["ratio"] for r in rows))
