"""The fallback kernels behind the run-time knobs (csrc/knobs.hpp), held to the bars the default kernels meet.

One test per row of tests/variants.py, one child process per row (tests/variant_child.py: the knobs are read once per
process).  Every case of a row runs through a float32 and a float64 handle, and:

  bar 1  float32 output against Oracle(...).process on the same input and chunking: <= 1 float32 ulp, relative RMS <= 1e-7
         (parity.assert_parity), shapes equal;
  bar 2  float64 output y against the long-double chain model ld (tests/chain_ld.py):
           e_g = max|y - ld| / max|ld| <= 1e-13          the project's fp64 parity bound, and
           e_g <= R * e_o, R = 8                         e_o: the CPU oracle against the same model, same chain, same run,
         exactly as tests/test_gpu_fp64_parity.py holds the default kernels (R: its docstring);
  names  the kernels the child's profile reports name hold the row's must-launch names and none of its must-not fragments,
         in both formats: without this a test passes by running the default kernel.

e_g / e_o measured on an MI355X (profiles/fp64_parity_variants.jsonl): 0.96 .. 1.59 (RATIOS_MEASURED below).  Neither bar is
relaxed for a fallback.  That the bars see a wrong fallback was shown once with a build in which poly_kernel's interpolated
branch leaves out its last tap and poly_coop_kernel its last shuffle step: no_polyi and no_polyi_no_polycoop then fail with
e_g / e_o = 4.5e7 .. 1.3e15.

Two scheduling switches are tested by what they must not change: RSMP_NO_SIDE (seam kernels on the main stream) gives the
bytes of the side-stream run, a small RSMP_SLAB_MB (many time slabs per push) gives the float32 bytes of the one-slab run.

A child that ends by a signal, by exit status 134 or 139, or at its timeout has faulted or hung on the GPU: every later test
of this file then fails at once without starting another child, and nothing is retried.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import variant_child
from chain_ld import case_reference, distance
from oracle_binding import Oracle
from parity import assert_parity
from variants import CHILD_TIMEOUT, SCHEDULING, VARIANT_IDS, VARIANTS, child_env

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))

BOUND = 1e-13
R = 8.0
# e_g / e_o per row as measured (smallest, largest); the default families: 0.93 .. 1.50.  Largest 1.59 (dft_kernel<13, 11, 13> as
# the x4 stage), 4 x 1.59 = 6.4: R = 8 holds for the fallbacks by the rule that set it.  poly_coop_kernel's shuffle tree, the one
# reordered sum among them, gives 0.97 and 1.40 where polyi_kernel gives 0.99 and 1.45.
RATIOS_MEASURED = {"no_fast": (1.03, 1.44), "no_mfma": (1.03, 1.44), "no_fuse": (1.03, 1.43), "no_fuse_no_polymf": (1.08, 1.17),
                   "no_polyi": (0.96, 1.40), "no_polyi_no_polycoop": (0.99, 1.45), "no_dftx": (1.51, 1.59), "spread_vector": (1.12, 1.49)}

_fault = None      # why no further child is started
_children = {}     # row id -> loaded .npz (dict), one child per row and process
_names_seen = set()


def run_child(tag, job, env_extra, tmp_path):
    """Start one child, wait for it, load what it wrote.  Fails (and latches) on a fault or a hang."""
    global _fault
    if _fault:
        pytest.fail("no further child is started: " + _fault)
    jp, op = os.path.join(str(tmp_path), tag + ".json"), os.path.join(str(tmp_path), tag + ".npz")
    with open(jp, "w") as f:
        json.dump(job, f)
    cmd = [sys.executable, os.path.join(HERE, "variant_child.py"), jp, op]
    t0 = time.time()
    try:
        p = subprocess.run(cmd, env=child_env(os.environ, env_extra), capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        _fault = "child %s was still running after %d s" % (tag, CHILD_TIMEOUT)
        pytest.fail(_fault + "\n" + err[-2000:])
    if p.returncode < 0 or p.returncode in (134, 139):
        _fault = "child %s ended with status %d" % (tag, p.returncode)
        pytest.fail(_fault + "\n" + p.stderr[-2000:])
    assert p.returncode == 0, (tag, p.returncode, p.stderr[-2000:])
    print("variant child %s took %.1f s" % (tag, time.time() - t0))
    with np.load(op) as z:
        return {k: z[k] for k in z.files}


def row_result(row, tmp_path):
    rid, env, cases = row[0], row[1], row[2]
    if rid not in _children:
        _children[rid] = run_child(rid, {"mode": "cases", "cases": cases}, env, tmp_path)
    return _children[rid]


def has(names, name):
    return any(name in k for k in names)


@pytest.mark.parametrize("row", VARIANTS, ids=VARIANT_IDS)
def test_variant_meets_both_bars(row, tmp_path):
    rid, env, cases, must, must_not = row
    got = row_result(row, tmp_path)
    names = {}
    failures = []
    for case in cases:
        cid, fi, fo, kw, frames, nch, S, api = case
        x, ld, _, e_o, _ = case_reference(case)
        assert np.array_equal(x, variant_child.case_input(frames, nch, S)[0])  # the child ran the model's input
        n32, n64 = set(got[cid + "/names32"].tolist()), set(got[cid + "/names64"].tolist())
        names[cid] = (n32, n64)
        _names_seen.update(n32 | n64)
        print("variant %s %s (%.1f s on the GPU) kernels f32 %s | f64 %s" % (rid, cid, float(got[cid + "/seconds"]), " ".join(sorted(n32)), " ".join(sorted(n64))))
        # bar 1
        y32 = got[cid + "/f32"]
        ref = Oracle(fi, fo, nch * S, **kw).process(x, chunk=16384 if api == "flow" else 4096)
        ref = ref.reshape(ref.shape[0], S, nch).transpose(1, 0, 2)
        assert y32.dtype == np.float32 and y32.shape == ref.shape, (cid, y32.shape, ref.shape)
        # bar 2
        y64 = got[cid + "/f64"]
        want = ld.reshape(ld.shape[0], S, nch).transpose(1, 0, 2)
        assert y64.dtype == np.float64 and y64.shape == want.shape, (cid, y64.shape, want.shape)
        e_g, rms_g = distance(y64, want)
        print("fp64variant " + json.dumps({"variant": rid, "case": cid, "e_g": float("%.4e" % e_g), "rel_rms_g": float("%.4e" % rms_g),
                                           "e_o": float("%.4e" % e_o), "ratio": round(e_g / e_o, 3)}))
        try:
            assert_parity(y32, ref)
            assert e_g <= BOUND, (e_g, rms_g)
            assert e_g <= R * e_o, (e_g, e_o, e_g / e_o)
        except AssertionError as e:  # (every case of the row is measured and printed before the row fails)
            failures.append((cid, str(e)))
    assert not failures, failures
    # names: in both formats
    for m in must:
        cids, name = ([m[0]], m[1:]) if isinstance(m, tuple) else ([c[0] for c in cases], (m,))
        for k in (0, 1):  # (name[-1]: the float64 handle's name where the formats have kernels of their own)
            assert any(has(names[c][k], name[-k]) for c in cids), (rid, m, "f32" if k == 0 else "f64", {c: sorted(names[c][k]) for c in cids})
    for frag in must_not:
        for cid, both in names.items():
            for ns in both:
                assert not has(ns, frag), (rid, cid, frag, sorted(ns))


def _stream_oracle(fi, fo, nch, x, cuts):
    """One stream through the oracle, pushed and pulled as the child did: [sum(cuts), nch] float32."""
    o = Oracle(fi, fo, nch)
    n = x.shape[0] // 2
    parts = []
    for k in range(2):
        o.push(x[k * n:(k + 1) * n])
        parts.append(o.pull_all(1 << 22))
    o.drain()
    parts.append(o.pull_all(1 << 22))
    assert [p.shape[0] for p in parts] == list(cuts), ([p.shape[0] for p in parts], list(cuts))
    return np.concatenate(parts)


def test_side_stream_seams_change_no_sample(tmp_path):
    """A seam ring of 0.01 MB squeezes the block table of 44.1k -> 96k to its 64-block minimum (about 110 000 input frames per
    launch), so a 330 000-frame push is several launches of the lean kernel with a seam kernel behind each; in the second
    (unprofiled) push those seam kernels run on the side stream beside the next launch, ordered by events against the two
    halves of the block table.  RSMP_NO_SIDE keeps them on the main stream: the same launches on the same blocks, so the same
    bytes in both formats.  Both streams of the float32 run against the oracle over both pushes and the drain."""
    env_side, env_main = SCHEDULING["side_stream"]
    a = run_child("side_stream", {"mode": "side_stream"}, env_side, tmp_path)
    b = run_child("side_stream_no_side", {"mode": "side_stream"}, env_main, tmp_path)
    for tag in ("32", "64"):
        print("side_stream f%s: lean launches in the profiled push %d / %d, frames out per call %s" % (tag, a["lean" + tag], b["lean" + tag], a["cuts" + tag]))
        assert int(a["lean" + tag]) >= 3 and int(b["lean" + tag]) >= 3
        assert np.array_equal(a["cuts" + tag], b["cuts" + tag])
        assert a["f" + tag].shape == b["f" + tag].shape and a["f" + tag].tobytes() == b["f" + tag].tobytes()
    fi, fo, nch, S = variant_child.SIDE
    x = variant_child.side_input()
    for s in range(S):
        assert_parity(a["f32"][s], _stream_oracle(fi, fo, nch, x[s], a["cuts32"]))


def test_small_slabs_change_no_float32_sample(tmp_path):
    """RSMP_SLAB_MB=0.001 gives size_slabs' floor of 8192 frames per time slab: a 100 000-frame push of 192k -> 44.1k runs its
    half-band stage 13 times, and the three unfused stages of 44.1k -> 192k at a 99 % passband take six slabs.  Against the run
    with the default budget (one slab): float32 output byte for byte (as test_rechunk_is_bit_invariant has it for chunking);
    float64 output to max|a - b| / max|b| <= 1e-13, since slab cuts move blocks between the lean and the generic kernel.  The
    small-slab float32 output against the oracle at the parity bar."""
    env_small, env_default = SCHEDULING["slabs"]
    a = run_child("slabs", {"mode": "slabs"}, env_small, tmp_path)
    b = run_child("slabs_default", {"mode": "slabs"}, env_default, tmp_path)
    for tag in ("32", "64"):
        print("slabs f%s: half_kernel launches in the push %d (default budget: %d)" % (tag, a["a/half" + tag], b["a/half" + tag]))
        assert int(a["a/half" + tag]) >= 12
    for key, (fi, fo, kw, frames, nch) in (("a", variant_child.SLAB_A), ("b", variant_child.SLAB_B)):
        assert a[key + "/f32"].shape == b[key + "/f32"].shape and a[key + "/f32"].tobytes() == b[key + "/f32"].tobytes(), key
        ya, yb = a[key + "/f64"], b[key + "/f64"]
        assert ya.shape == yb.shape
        d = float(np.abs(ya - yb).max() / np.abs(yb).max())
        print("slabs %s: float64 max|a - b| / max|b| = %.3e" % (key, d))
        assert d <= BOUND, (key, d)
        x = variant_child.slab_input(frames, nch)
        assert_parity(a[key + "/f32"], Oracle(fi, fo, nch, **kw).process(x, chunk=frames))


# what only the knobs reach; checked against the union of the names the children reported
ONLY_BY_KNOB = ["rsmp::poly_coop_kernel<2>", "rsmp::poly_coop_kernel<3>", "rsmp::poly_kernel<0>", "rsmp::poly_kernel<1>",
                "rsmp::poly_kernel<2>", "rsmp::poly_kernel<3>", "rsmp::fused_kernel<12, 11, 2, 25, false>",
                "rsmp::fused_kernel<12, 12, 2, 27, false>", "rsmp::fused_kernel<12, 11, 2, 7, true>", "rsmp::polymf_kernel<",
                "rsmp::dft_kernel<12, 11, 12", "rsmp::dft_kernel<12, 12, 12", "rsmp::dft_kernel<13, 11, 13"]


def test_variant_kernel_families_covered(tmp_path):
    """The union of the kernel names of all rows holds every family that only a knob reaches.  (The row tests check which
    case launched what: poly_kernel<0> with its table in LDS and without, polymf_kernel behind dft_kernel<12, ..>, and
    dft_kernel<13, 11, 13> as the x4 stage.)"""
    for row in VARIANTS:
        got = row_result(row, tmp_path)
        for k, v in got.items():
            if "/names" in k:
                _names_seen.update(v.tolist())
    print("variant kernels " + " | ".join(sorted(_names_seen)))
    for fam in ONLY_BY_KNOB:
        assert has(_names_seen, fam), (fam, sorted(_names_seen))
