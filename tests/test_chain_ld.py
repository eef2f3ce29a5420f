"""The oracle's fp64 signal path against a long-double restatement of the same chain (tests/chain_ld.py), CPU only.

For every chain of the fp64 parity table: e_o = max|o - ld| / max|ld| <= 1e-13, the project's fp64 parity bound, where o is the
oracle's fp64 output fifo (one push, drain, never pulled) and ld the long-double model.  Measured: e_o 5.0e-16 .. 1.3e-15 on
every chain (profiles/fp64_parity_cpu.json), i.e. the oracle's own FFT and loops round like a good fp64 implementation.

Then the comparison is shown to see the mistakes it is there for: the model alone is perturbed once per stage kind (last
polyphase tap left out, one phase's linear / highest Horner coefficient zeroed, outermost half-band coefficient zeroed,
outermost DFT-filter tap zeroed, one spectrum bin turned by one twiddle step) and must move by >= 100 e_o."""
import json
import os

import numpy as np
import pytest

import chain_ld
from chain_ld import CASES, CASE_IDS, ChainLD, case_reference, distance
from oracle_binding import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-13


def test_long_double_is_extended():
    chain_ld.require()
    x = np.random.default_rng(0).standard_normal(131072).astype(np.longdouble)
    rt = np.fft.irfft(np.fft.rfft(x), 131072)
    assert float(np.abs(rt - x).max()) < 1e-17  # (fp64: ~2e-15)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_oracle_against_long_double(case):
    x, ld, ref, e_o, rms_o = case_reference(case)
    assert ref.shape == ld.shape, (ref.shape, ld.shape)
    print("%s e_o %.3e rms %.3e" % (case[0], e_o, rms_o))
    assert e_o <= BOUND, (e_o, rms_o)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_three_blocks_of_the_longest_stage(case):
    """A condition on the frame counts of the table: the longest DFT stage runs at least three blocks before the drain."""
    _, fi, fo, kw, frames, nch, S, _ = case
    N, blocks = max(chain_ld.blocks_before_drain(fi, fo, kw, frames, nch * S))
    assert N >= 2048 and blocks >= 3, (N, blocks)


def _perturbation_cases():
    seen, out = set(), []
    for case in CASES:
        key = (case[1], case[2], tuple(sorted(case[3].items())))
        if key in seen:
            continue
        seen.add(key)
        out.append(case)
    return out


@pytest.mark.parametrize("case", _perturbation_cases(), ids=[c[0] for c in _perturbation_cases()])
def test_named_mistakes_are_visible(case):
    """Each perturbation of the model (channel 0 of the case's input) against the unperturbed model: >= 100 e_o."""
    _, fi, fo, kw, frames, nch, S, _ = case
    x, ld, ref, e_o, _ = case_reference(case)
    assert e_o <= BOUND
    o = Oracle(fi, fo, 1, **kw)
    m = ChainLD(o)
    tried = 0
    for what in ChainLD.PERTURBATIONS:
        if not m.has(what):
            continue
        tried += 1
        moved, _ = distance(m.run(x[:, :1], perturb=what), ld[:, :1])
        print("%s %s moved %.3e = %.1e e_o" % (case[0], what, moved, moved / e_o))
        assert moved >= 100 * e_o, (what, moved, e_o)
    assert tried >= 2


def test_every_perturbation_is_exercised():
    have = set()
    for case in _perturbation_cases():
        o = Oracle(case[1], case[2], 1, **case[3])
        m = ChainLD(o)
        have |= {w for w in ChainLD.PERTURBATIONS if m.has(w)}
    assert have == set(ChainLD.PERTURBATIONS)


def test_profile_lists_every_chain():
    """profiles/fp64_parity_cpu.json holds the measured e_o of every chain of the table."""
    with open(os.path.join(ROOT, "profiles", "fp64_parity_cpu.json")) as f:
        rec = json.load(f)
    assert sorted(rec["chains"]) == sorted(CASE_IDS)
    assert all(0 < c["e_o"] <= BOUND for c in rec["chains"].values())


if __name__ == "__main__":  # python tests/test_chain_ld.py: measure again and rewrite profiles/fp64_parity_cpu.json
    chains = {}
    for case in CASES:
        _, ld, ref, e_o, rms_o = case_reference(case)
        chains[case[0]] = {"in_rate": case[1], "out_rate": case[2], "options": case[3], "frames": case[4], "channels": case[5] * case[6],
                           "frames_out": int(ld.shape[0]), "e_o": e_o, "rel_rms_o": rms_o}
    with open(os.path.join(ROOT, "profiles", "fp64_parity_cpu.json"), "w") as f:
        json.dump({"what": "oracle fp64 output fifo against the long-double chain model: e_o = max|o - ld| / max|ld|, lcg noise, "
                           "one push + drain", "bound": BOUND, "chains": chains}, f, indent=1)
        f.write("\n")
