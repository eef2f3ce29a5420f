"""The premise of tests/test_gpu_far_positions.py, on the oracle alone (no GPU): a periodic input gives, past the start-up
transient, a periodic output, so the oracle's window R = y[Wo:2Wo] of a fresh stream is the reference for any position; the
case table reaches past 2^32 with every fifo index; and each case's chain is the one its row names."""
from fractions import Fraction

import numpy as np
import pytest

import foo_dsp_resampler_amd as F
import far_cases as FC
from parity import assert_parity


@pytest.mark.parametrize("cid", FC.RATIONAL)
def test_output_repeats_every_wo(cid):
    """y[2Wo : 2Wo + m] against R[:m] at the project's bar for the format, and the total after the drain is 3 Wo"""
    case, ref = FC.BY_ID[cid], FC.reference(cid)
    Wo = ref.geo.Wo
    assert ref.y.shape == (3 * Wo, case.nch) and sum(ref.counts) == 3 * Wo, (ref.y.shape, ref.counts)
    m = sum(ref.counts[:3]) - 2 * Wo  # what the third push has made ready past 2 Wo
    assert m > Wo // 2, (m, ref.counts)
    a, b = ref.y[2 * Wo:2 * Wo + m], ref.R[:m]
    if case.fmt == "f64":
        e = np.abs(a - b).max() / np.abs(b).max()
        print("far premise %s: m %d e %.3e bit_equal_frac %.6f" % (cid, m, e, np.mean(a == b)))
        assert e <= 1e-13, e
    else:  # (s16: the oracle's float output; its integers follow from it)
        rep = assert_parity(a.astype(np.float32), b.astype(np.float32))
        print("far premise %s: m %d %s" % (cid, m, rep))
    # the first window is still inside the transient: R must not be taken from there
    assert not np.array_equal(ref.y[:Wo], ref.R)


@pytest.mark.parametrize("cid", [c.id for c in FC.CASES])
def test_every_index_passes_the_limit(cid):
    """n_far * Wi and every derived stage count exceed 2^32 (+ Wi), and one push fewer would not"""
    case = FC.BY_ID[cid]
    geo = FC.geometry(case)
    assert case.limit == 1 << 32  # (a case cut to 2^31 for its run time says so in its docstring: none is)
    assert geo.Wi <= geo.isamp_max
    if cid != "interp":
        assert geo.Wi + case.fi // np.gcd(case.fi, case.fo) > geo.isamp_max  # the largest K
        assert Fraction(geo.Wo, geo.Wi) == Fraction(case.fo, case.fi)
    assert len(geo.counts) == len(geo.rates) >= 2
    assert geo.n_far * geo.Wi > (1 << 32)
    assert all(c > case.limit + geo.Wi for c in geo.counts), geo.counts
    assert any((geo.n_far - 1) * geo.Wi * r <= case.limit + geo.Wi for r in geo.rates)
    print("far geometry %s: Wi %d Wo %s n_far %d counts %s" % (cid, geo.Wi, geo.Wo, geo.n_far, [float(c) for c in geo.counts]))


@pytest.mark.parametrize("cid", [c.id for c in FC.CASES])
def test_case_lands_on_its_chain(cid):
    """What the planner and RRX_describe_dispatch say of each case (host-only): the stage kinds and block lengths, and whether
    the first stage pair is sub-blocked, in how many sub-blocks, in two rounds.  The kernel names themselves are asserted on
    the GPU, from the handle's profile records of the first push (tests/test_gpu_far_positions.py)."""
    case = FC.BY_ID[cid]
    stages, sub, nsub, two = case.dispatch
    plan = F.describe_plan(case.fi, case.fo, **case.kw)
    got = [(s["kind"], s["dft_length"] if s["kind"] == "dft" else s.get("interp_order", 0)) for s in plan["stages"]]
    assert got == stages, got
    d = F.describe_dispatch(case.fi, case.fo, case.nch, **case.kw)
    assert d["sub_blocked"] == sub, d
    if sub:
        assert (d["nsub"], d["two_round"]) == (nsub, two), d
    assert case.families


def _block_model(g, k):
    """fused_block_info's i_lo, cnt, irel_lo, base_li and K in Python integers (kernels.hpp), for entry k of a table that
    starts at block g.B0"""
    b0, V = g.b_offset + (g.B0 + k) * g.V, g.V
    if g.nsub > 0:
        kr, i = divmod(k, g.nsub)
        b0, V = g.b_offset + (g.B0 + kr) * g.V + i * g.Vs, min(g.V - i * g.Vs, g.Vs)
    nlo, nhi = b0 * g.polyL - g.at0, (b0 + V - g.n + 1) * g.polyL - g.at0
    ilo, ihi = max(0, -(-nlo // g.step)), max(0, -(-nhi // g.step))
    cnt = max(ihi - ilo, 0)
    kk = ilo // g.polyL
    return {"i_lo": ilo, "cnt": cnt, "irel_lo": ilo - kk * g.polyL, "base_li": kk * g.step - b0,
            "K": (ihi - 1) // g.polyL - kk + 1 if cnt else 0}


@pytest.mark.parametrize("cid", ["up", "down", "x4", "f64"])
def test_block_table_at_far_positions(cid):
    """The lean fused pairs' block table (fused_block_info, the one closed form the device and the host share; through
    RRX_debug_tile_walk) where its 64-bit terms pass 2^31 and 2^32: the blocks around the points at which the stage-1 index b0
    and the output index i_lo cross, and the last block of the case's n_far pushes, against Python integers -- and every
    property tests/test_tile_walk.py holds a block to (each output once, windows inside their LDS image)."""
    from test_tile_walk import check_block, lean_chains
    case = FC.BY_ID[cid]
    geo = FC.geometry(case)
    plan, chains = lean_chains(case.fi, case.fo, case.nch, **case.kw)
    assert len(chains) == 1, plan
    g, ahead, dft_L = chains[0]
    per = max(1, g.nsub)
    last = int(geo.counts[1]) // g.V  # blocks of stage-1 samples in n_far pushes
    starts = {last - 2}
    for X in (1 << 31, 1 << 32):
        starts.add(X // g.V - 1)                              # b0 passes X
        starts.add(X * g.step // g.polyL // g.V - 1)          # i_lo passes X
    seen_b0 = seen_i = 0
    for B0 in sorted(starts):
        assert 0 < B0 < last
        g.B0 = B0
        prev_end = None
        for k in range(3 * per):
            h = check_block(g, k, (cid, B0))
            m = _block_model(g, k)
            assert {key: h[key] for key in m} == m, (cid, B0, k, h, m)
            if prev_end is not None:
                assert h["i_lo"] >= prev_end, (cid, B0, k)  # (the outputs between two blocks are the seam kernel's)
            prev_end = h["i_lo"] + h["cnt"]
            seen_b0 = max(seen_b0, g.b_offset + (B0 + k // per + 1) * g.V)
            seen_i = max(seen_i, prev_end)
    assert seen_b0 > 1 << 32 and seen_i > 1 << 32, (seen_b0, seen_i)


def test_interp_reference_fits_a_sine():
    """the oracle's fresh 44100 -> 48001 output is the input's sine on the grid of the stage's own 32.32 clock: the residual of
    the fit is at float32 rounding, and the NOMINAL grid j * fi / fo would already miss by far more at the end of one push"""
    geo, ig, x, a, b, rmax, rrms = FC.interp_reference()
    print("far interp: a %.9f b %.9f r_o max %.3e rms %.3e" % (a, b, rmax, rrms))
    assert abs(np.hypot(a, b) - 0.5) < 1e-6
    assert rmax < 1e-7, rmax  # 0.5 full scale: half a float32 ulp is 3e-8
    assert Fraction(1 << 32, ig.step) * ig.F != Fraction(48001, 44100)
    # phases reduced in integers agree with the plain float product while that is still exact enough
    ph = FC.interp_times(ig, FC.interp_phase_tables(ig), 5, 1000)
    j = np.arange(5, 1005, dtype=np.float64)
    plain = 2.0 * np.pi * ig.cycles * (ig.at0 + j * ig.step) / ig.period
    assert np.abs(np.angle(np.exp(1j * (ph - plain)))).max() < 1e-9
