"""CPU-only: the start states of the lean fused kernels' tile walk (kernels.hpp: WalkStart, fused_walk_start), the record that
fused_prep_kernel writes beside every block-table entry and that the kernels begin their polyphase rounds from, read back on
the host through RRX_debug_walk_start and held against the slot-by-slot enumeration of RRX_debug_tile_walk.

What the enumeration cannot vouch for by itself (it starts every wave from the same record) is checked against the walk's
definition: a round's tiles come in group-major order, and wave w of 4 owns tiles [nt w / 4, nt (w + 1) / 4) of the round's nt.
tests/test_tile_walk.py asserts on the same enumeration that every output of a block is produced exactly once.
"""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import foo_dsp_resampler_amd as F
from foo_dsp_resampler_amd.ratelib import WalkStart
from test_tile_walk import BASELINE, RATES, ROOT, SLOT_CAP, blocks_per_push, lean_chains

_slots = np.empty((SLOT_CAP, 7), dtype=np.int32)
KEYS = ("i_lo", "cnt", "K", "KA", "per_group", "g_lo", "g_hi", "ka", "tiles", "tiles_uniform", "irel_lo", "base_li", "ngrp")


def walk(g, k):
    head = (C.c_longlong * 13)()
    n = F.lib().RRX_debug_tile_walk(C.byref(g), int(k), head, _slots.ctypes.data, SLOT_CAP)
    assert 0 <= n <= SLOT_CAP, n
    return dict(zip(KEYS, (int(v) for v in head))), _slots[:n]


def walk_start(g, k):
    ws = WalkStart()
    assert F.lib().RRX_debug_walk_start(C.byref(g), int(k), C.byref(ws)) == 0
    return ws


def round_ints(r):
    return ([r.kb, r.ke, r.cnt, r.b1, r.b2, r.pad] + list(r.p0) + list(r.pend)
            + [v for w in r.wave for v in (w.n, w.g, w.pc, w.pend)])


def check_block(g, k, tag):
    h, s = walk(g, k)
    ws = walk_start(g, k)
    ctx = (tag, k, h)
    assert len(s) == 64 * h["tiles"], ctx
    total = 0
    for rnd in (0, 1):
        r = ws.round[rnd]
        kb, ke = (h["ka"], h["K"]) if rnd else (0, h["ka"])
        tiles = s[s[:, 0] == rnd][::64]  # lane 0 of every tile: (round, group, column step, ...)
        if h["cnt"] == 0 or ke <= kb:  # a round the block does not have: nothing in the record, nothing walked
            assert not any(round_ints(r)), ctx
            assert len(tiles) == 0, ctx
            continue
        assert (r.kb, r.ke) == (kb, ke) and 0 <= r.b1 <= r.b2 <= h["ngrp"], ctx
        nt = len(tiles)
        gc = [(int(t[1]), int(t[2])) for t in tiles]
        assert gc == sorted(gc) and len(set(gc)) == nt, ctx  # group-major, each tile once
        for w in range(4):
            t0, t1 = (nt * w) >> 2, (nt * (w + 1)) >> 2
            e = r.wave[w]
            assert e.n == t1 - t0, (ctx, rnd, w)
            if e.n == 0:
                assert (e.g, e.pc, e.pend) == (0, 0, 0), (ctx, rnd, w)
                continue
            assert (e.g, e.pc >> 2) == gc[t0], (ctx, rnd, w)
            # pc = p0 + 4 column steps with the group's first period p0 < 2; the group's tiles end at pend
            run = 2 if e.g >= r.b2 else 1 if e.g >= r.b1 else 0
            assert e.pc & 3 == r.p0[run] and e.pend == r.pend[run], (ctx, rnd, w)
            assert e.pend - r.p0[run] == 4 * sum(1 for t in gc if t[0] == e.g), (ctx, rnd, w)
            total += e.n
        # outputs the round may store: everything it keeps lies below cnt, and the block's last round reaches its last output
        kept = s[(s[:, 0] == rnd) & (s[:, 5] == 1)]
        assert len(kept) == 0 or kept[:, 4].max() < r.cnt, ctx
        if ke == h["K"]:
            assert r.cnt == h["cnt"], ctx
    assert total == h["tiles"], ctx
    return h


@pytest.mark.parametrize("cfg", range(len(BASELINE)))
def test_every_block_of_a_baseline_push(cfg):
    fi, fo, nch, kw, frames = BASELINE[cfg]
    plan, chains = lean_chains(fi, fo, nch, **kw)
    assert chains
    frames = frames or plan["isamp_max"]
    for g, ahead, dft_L in chains:
        nb = blocks_per_push(g, ahead, dft_L, frames)
        if cfg == 1:
            assert nb >= 272, nb
        for k in range(nb):
            check_block(g, k, (fi, fo))
        print("config %d: %d -> %d, %d table entries checked" % (cfg, fi, fo, nb))


def test_first_blocks_of_the_rate_matrix():
    chains, entries, second = 0, 0, 0
    for fi, fo in itertools.product(RATES, RATES):
        if fi == fo:
            continue
        for kw in ({}, {"bandwidth": 99.0}, {"bandwidth": 97.0}):
            for g, _, _ in lean_chains(fi, fo, 2, **kw)[1]:
                chains += 1
                for k in range(40):
                    h = check_block(g, k, (fi, fo, kw))
                    entries += 1
                    second += h["cnt"] > 0 and h["ka"] < h["K"]
    assert chains >= 40, chains
    assert second > 0  # blocks with a second round are among them
    print("rate matrix: %d lean fused chains, %d table entries, %d with two rounds" % (chains, entries, second))


def test_hook_is_inert_without_test_hooks():
    """RRX_debug_walk_start answers only in a process started with RSMP_TEST_HOOKS (tests/conftest.py sets it)."""
    code = ("import sys, ctypes as C; sys.path.insert(0, %r)\n"
            "import foo_dsp_resampler_amd as F\n"
            "from foo_dsp_resampler_amd.ratelib import WalkGeom, WalkStart\n"
            "g = WalkGeom(at0=0, b_offset=0, B0=0, V=3542, polyL=160, step=147, n=24, KS=7, qb_min=0, qb_max=146, two_round=1)\n"
            "ws = WalkStart()\n"
            "print(F.lib().RRX_debug_walk_start(C.byref(g), 1, C.byref(ws)), sum(w.n for r in ws.round for w in r.wave))\n" % ROOT)
    env = {k: v for k, v in os.environ.items() if k != "RSMP_TEST_HOOKS"}
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-2:] == ["-1", "0"]
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(env, RSMP_TEST_HOOKS="1"))
    assert out.returncode == 0, out.stderr
    rc, tiles = out.stdout.split()[-2:]
    assert rc == "0" and int(tiles) > 0
