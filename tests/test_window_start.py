"""CPU-only: the window start of a 4-residue block as the lean fused kernels compute it where a residue group becomes current
-- numerator at0 + rb * step, multiplied high by a 32-bit reciprocal of polyL and shifted (kernels.hpp: walk_rcp, walk_q_rcp) --
held against the host table `qtab` that the other kernels read (walk_q_table), through RRX_debug_window_start.

For every rational polyphase stage of the BASELINE configs and of the rate matrix that tests/test_host_plan.py plans: every
(group, block) gives the table's value, which is the plain quotient restated here; the largest numerator the hook reports is
the largest one a launch can form; and the multiplier and shift give floor(num / polyL) for EVERY num in [0, that numerator],
not only for the ones the groups produce.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import foo_dsp_resampler_amd as F
from foo_dsp_resampler_amd.ratelib import WalkGeom
from test_tile_walk import BASELINE, RATES


def poly_stages(fi, fo, **kw):
    """(polyL, step, at0) of every rational (order-0) polyphase stage of the chain."""
    out = []
    for p in F.describe_plan(fi, fo, **kw)["stages"]:
        if p["kind"] == "poly" and p["interp_order"] == 0:
            out.append((p["L"], p["step_int"], p["at"] >> 32))
    return out


def window_start(L, step, at0, g, bq):
    geom = WalkGeom(at0=at0, b_offset=0, B0=0, V=1, polyL=L, step=step, n=1, KS=7)
    arith, table, rcp = C.c_int(), C.c_int(), (C.c_uint * 3)()
    rc = F.lib().RRX_debug_window_start(C.byref(geom), g, bq, C.byref(arith), C.byref(table), rcp)
    return rc, arith.value, table.value, tuple(int(v) for v in rcp)


def check_stage(L, step, at0):
    ngrp = (L + 15) // 16
    m = s = nmax = None
    for g in range(ngrp):
        for bq in range(4):
            rc, arith, table, rcp = window_start(L, step, at0, g, bq)
            ctx = (L, step, at0, g, bq, rcp)
            assert rc == 0, ctx
            rb = 16 * g + 4 * bq
            want = (at0 + (rb if rb < L else 0) * step) // L  # engine.cpp, mf_operands: an idle block takes block 0's
            assert table == want and arith == want, (ctx, arith, table, want)
            assert m is None or (m, s, nmax) == rcp, ctx
            m, s, nmax = rcp
    assert nmax == at0 + ((L - 1) & ~3) * step, (L, step, at0, nmax)
    assert 0 < m < 2 ** 32 and 0 <= s < 32
    # every numerator up to the largest one: floor(num * m / 2^32) >> s in 32-bit arithmetic, as the kernel does it
    for lo in range(0, nmax + 1, 1 << 22):
        num = np.arange(lo, min(lo + (1 << 22), nmax + 1), dtype=np.uint64)
        q = ((num * np.uint64(m)) >> np.uint64(32)) >> np.uint64(s)
        bad = np.nonzero(q != num // np.uint64(L))[0]
        assert len(bad) == 0, (L, step, at0, m, s, int(num[bad[0]]))
    return nmax


@pytest.mark.parametrize("cfg", range(len(BASELINE)))
def test_baseline_polyphase_stages(cfg):
    fi, fo, nch, kw, _ = BASELINE[cfg]
    st = poly_stages(fi, fo, **kw)
    assert st, (fi, fo)  # every BASELINE chain has a rational polyphase stage
    for L, step, at0 in st:
        nmax = check_stage(L, step, at0)
        print("config %d: polyL %d step %d at0 %d: %d groups, numerators 0 .. %d" % (cfg, L, step, at0, (L + 15) // 16, nmax))


def test_rate_matrix_polyphase_stages():
    seen = set()
    for fi, fo in itertools.product(RATES, RATES):
        if fi == fo:
            continue
        for kw in ({}, {"bandwidth": 99.0}):
            seen.update(poly_stages(fi, fo, **kw))
    assert len(seen) >= 10, len(seen)  # (the matrix has 17 distinct ones; the sweep must not come out empty)
    total = 0
    for L, step, at0 in sorted(seen):
        total += check_stage(L, step, at0) + 1
    print("rate matrix: %d distinct polyphase stages, %d numerators" % (len(seen), total))


def test_partial_last_group_and_refusals():
    # polyL 147 (96k -> 44.1k): the last group has blocks 144 (live) and 148, 152, 156 (idle: block 0's window start)
    rc, a0, t0, _ = window_start(147, 320, 5, 0, 0)
    assert rc == 0 and a0 == t0 == 0
    rc, a, t, _ = window_start(147, 320, 5, 9, 0)
    assert rc == 0 and a == t == (5 + 144 * 320) // 147
    for bq in (1, 2, 3):
        rc, a, t, _ = window_start(147, 320, 5, 9, bq)
        assert rc == 0 and a == t == a0
    # no 32-bit multiplier: polyL 1; numerators beyond 31 bits; a group or block the stage does not have
    assert window_start(1, 1, 0, 0, 0)[0] == -2
    assert window_start(40000, 70000, 0, 0, 0)[0] == -2
    assert window_start(160, 147, 0, 10, 0)[0] == -2
    assert window_start(160, 147, 0, 0, 4)[0] == -2
