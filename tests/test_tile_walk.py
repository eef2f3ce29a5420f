"""CPU-only: the tile walk of the lean fused kernels' polyphase stage (fused_fast.hip: poly_round), enumerated slot by slot on
the host through RRX_debug_tile_walk -- the same closed forms (fused_block_info, fused_walk, walk_round, walk_seek, walk_ncs)
that the kernels and their block table use.

Every 16-residue group walks its own periods: a group whose residues all lie in front of the block's first output starts at
period 1, a group whose residues all lie behind the block's last partial period ends one period early.  For each block the
tests assert that
  * every output of [i_lo, i_lo + cnt) is produced exactly once, and no slot that the store's range check keeps is
    produced twice;
  * every kept slot's window (4 KS samples) lies inside the LDS image of its round;
  * the block has no more tiles than the uniform walk, ngrp x (ceil(KA / 4) + ceil((K - KA) / 4)); a block that keeps the
    uniform walk has exactly that many;
  * 44.1k -> 96k (polyL 160, step 147, V 3544, n 24): at most 62 tiles for every block of a 481 689-frame push (70 before).
The bound 62: a block's ~3829 outputs span 23.9 periods, so no residue owns more than 24 periods = 6 column steps of 4; only
the one or two groups that straddle the first output's residue or the last one's touch 25 periods = 7 column steps:
8 x 6 + 2 x 7 = 62 of the 10 groups' tiles.
"""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import foo_dsp_resampler_amd as F
from foo_dsp_resampler_amd.ratelib import WalkGeom

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = [8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 64000, 88200, 96000, 176400, 192000]
# the five BASELINE configs (bench.py CONFIGS): rates, channels, plan options, frames per push (None: isamp_max)
BASELINE = [(44100, 48000, 2, {}, None), (44100, 96000, 2, {}, None), (44100, 192000, 8, {"bandwidth": 99.0}, None),
            (96000, 44100, 32, {"allow_aliasing": 0, "phase": 50.0}, None), (44100, 48000, 2, {}, 240000)]
SLOT_CAP = 1 << 16


def mf_geom(L, step, at0, n):
    """Window geometry of the 4-residue blocks (engine.cpp, mf_geom), restated."""
    d4, qb_min = 0, at0 // L
    qb_max = qb_min
    for rb in range(0, L, 4):
        a0, a1 = at0 + rb * step, at0 + min(rb + 3, L - 1) * step
        d4 = max(d4, a1 // L - a0 // L)
        qb_max = max(qb_max, a0 // L)
    return max(7, (n + d4 + 3) // 4), qb_min, qb_max


def lean_chains(fi, fo, nch, **kw):
    """The dft -> rational polyphase pairs of a chain that run on the lean fused kernels, as (WalkGeom, frames ahead ratio,
    dft L): 4096-point blocks in two rounds (fused_fast_kernel), or the sub-blocked forms of longer x2 blocks."""
    plan = F.describe_plan(fi, fo, **kw)
    st = plan["stages"]
    out, ahead = [], 1.0
    for i in range(len(st) - 1):
        d, p = st[i], st[i + 1]
        if (d["kind"] == "dft" and p["kind"] == "poly" and p["interp_order"] == 0 and d["step_int"] == 1 and d["L"] in (1, 2, 4)
                and p["L"] >= 64 and nch % 2 == 0):
            L, step, at0, n = p["L"], p["step_int"], p["at"] >> 32, p["n"]
            KS, qb_min, qb_max = mf_geom(L, step, at0, n)
            N = d["dft_length"]
            V = N - (d["num_taps"] - 1)
            g = WalkGeom(at0=at0, b_offset=p["preload"], B0=0, V=V, polyL=L, step=step, n=n, KS=KS, qb_min=qb_min, qb_max=qb_max,
                         two_round=0, ra_end=0, rb_start=0, nsub=0, Vs=0)
            kmax = (V * L // step + L - 1) // L + 2
            if N == 4096 and d["L"] in (1, 2):
                if KS in (7, 8) and (qb_max - qb_min) + 4 * KS + 4 <= 2 * 256 + 32 and kmax <= 32:
                    g.two_round = 1
                    out.append((g, ahead, d["L"]))
            elif i == 0:
                disp = F.describe_dispatch(fi, fo, nch, **kw)
                if disp["sub_blocked"]:
                    g.nsub, g.Vs = disp["nsub"], disp["Vs"]
                    if disp["two_round"]:
                        g.two_round, g.ra_end, g.rb_start = 1, 2 * 9 * 256, 2 * 8 * 256
                    out.append((g, ahead, d["L"]))
        ahead *= 0.5 if st[i]["kind"] == "half" else st[i]["L"] / st[i]["step_int"]
    return plan, out


def walk(g, k):
    head = (C.c_longlong * 13)()
    slots = np.empty((SLOT_CAP, 7), dtype=np.int32)
    n = F.lib().RRX_debug_tile_walk(C.byref(g), int(k), head, slots.ctypes.data, SLOT_CAP)
    assert 0 <= n <= SLOT_CAP, n
    keys = ("i_lo", "cnt", "K", "KA", "per_group", "g_lo", "g_hi", "ka", "tiles", "tiles_uniform", "irel_lo", "base_li", "ngrp")
    return dict(zip(keys, (int(v) for v in head))), slots[:n]


def check_block(g, k, tag):
    """All assertions for one table entry; returns its head."""
    h, s = walk(g, k)
    ctx = (tag, k, h)
    cnt, K, KA, ngrp = h["cnt"], h["K"], h["KA"], h["ngrp"]
    assert ngrp == (g.polyL + 15) // 16
    old = ngrp * ((KA + 3) // 4 + ((K - KA + 3) // 4 if KA < K else 0)) if cnt > 0 else 0
    assert h["tiles_uniform"] == old, ctx
    assert h["tiles"] <= old, ctx
    if not h["per_group"]:
        assert h["tiles"] == old and (h["g_lo"], h["g_hi"], h["ka"]) == (0, ngrp, KA), ctx
    assert len(s) == 64 * h["tiles"], ctx
    if cnt == 0:
        return h
    kept = s[s[:, 5] == 1]
    ib = np.sort(kept[:, 4])
    # every output exactly once; nothing the store keeps is produced twice
    assert len(ib) == cnt and np.array_equal(ib, np.arange(cnt, dtype=ib.dtype)), ctx
    # a (round, group, column step, lane) slot is visited once
    key = ((s[:, 0].astype(np.int64) * 4096 + s[:, 1]) * 4096 + s[:, 2]) * 64 + s[:, 3]
    assert len(np.unique(key)) == len(key), ctx
    # the windows of the kept slots lie inside their round's LDS image (32 guard samples on either side)
    V = g.V
    if g.nsub > 0:
        i = k % g.nsub
        V = min(g.V - i * g.Vs, g.Vs)
    ra_end, rb_start = (g.ra_end, g.rb_start) if g.ra_end > 0 else (12 * 256, 10 * 256)
    two = g.two_round and V > ra_end
    a, b = kept[kept[:, 0] == 0], kept[kept[:, 0] == 1]
    if len(a):
        assert a[:, 6].min() >= -32 and a[:, 6].max() + 4 * g.KS <= (min(V, ra_end) if two else V) + 32, ctx
    if len(b):
        assert two, ctx
        assert b[:, 6].min() >= rb_start and b[:, 6].max() + 4 * g.KS <= V + 32, ctx
    return h


def blocks_per_push(g, ahead, dft_L, frames):
    """Table entries of one push of `frames` chain-input frames: blocks of V stage samples, nsub sub-blocks each."""
    return (int(frames * ahead * dft_L) // g.V + 2) * max(1, g.nsub)


@pytest.mark.parametrize("cfg", range(len(BASELINE)))
def test_baseline_chains_at_bench_geometry(cfg):
    fi, fo, nch, kw, frames = BASELINE[cfg]
    plan, chains = lean_chains(fi, fo, nch, **kw)
    assert chains, (fi, fo, plan["stages"])  # every BASELINE chain has a lean fused pair
    frames = frames or plan["isamp_max"]
    for g, ahead, dft_L in chains:
        nb = blocks_per_push(g, ahead, dft_L, frames)
        tiles, old, uni = 0, 0, 0
        for k in range(3 * nb):  # three pushes: a handle's block index keeps counting from push to push
            h = check_block(g, k, (fi, fo))
            tiles += h["tiles"]
            old += h["tiles_uniform"]
            uni += not h["per_group"]
        print("config %d: %d -> %d, polyL %d step %d V %d n %d KS %d nsub %d: %d entries, tiles %d (uniform walk %d, %.1f %% fewer), "
              "uniform fallback %.1f %%" % (cfg, fi, fo, g.polyL, g.step, g.V, g.n, g.KS, g.nsub, 3 * nb, tiles, old,
                                            100.0 * (old - tiles) / max(old, 1), 100.0 * uni / (3 * nb)))


@pytest.mark.parametrize("V", [3544, 3542])
def test_headline_chain_has_at_most_62_tiles_per_block(V):
    """configs[1], 44.1k -> 96k: polyL 160, step 147, n 24; every block of a 481 689-frame push.  The chain's blocks have
    V = 4096 - (553 - 1) = 3544 valid samples; V = 3542 is the same geometry with the block length the bound was first
    stated for.  70 tiles with the uniform walk."""
    plan, chains = lean_chains(44100, 96000, 2)
    assert plan["isamp_max"] == 481689 and len(chains) == 1
    g, ahead, dft_L = chains[0]
    assert (g.polyL, g.step, g.V, g.n, g.KS, g.two_round, g.nsub) == (160, 147, 3544, 24, 7, 1, 0)
    g.V = V
    nb = blocks_per_push(g, ahead, dft_L, 481689)
    worst, hist = 0, {}
    for k in range(nb):
        h = check_block(g, k, "headline")
        worst = max(worst, h["tiles"])
        key = (h["tiles"], h["tiles_uniform"])
        hist[key] = hist.get(key, 0) + 1
    print("headline chain, V %d: %d blocks, (tiles, tiles of the uniform walk) per block: %s" % (V, nb, sorted(hist.items())))
    assert worst <= 62, hist


def test_rate_matrix_sweep():
    """Every lean fused chain of the 13 x 13 rate matrix (default options and a 99 % passband, stereo): the first blocks of the
    stream and a seeded sample of later ones.  Nothing is skipped: a block that keeps the uniform walk is checked like any
    other, and the share of such blocks is printed."""
    rng = np.random.default_rng(20240613)
    chains, entries, uni, tiles, old = 0, 0, 0, 0, 0
    for fi, fo in itertools.product(RATES, RATES):
        if fi == fo:
            continue
        for kw in ({}, {"bandwidth": 99.0}, {"bandwidth": 97.0}):
            for g, _, _ in lean_chains(fi, fo, 2, **kw)[1]:
                chains += 1
                ks = list(range(4)) + sorted(int(v) for v in rng.integers(4, 200000, 20))
                for k in ks:
                    h = check_block(g, k, (fi, fo, kw))
                    entries += 1
                    uni += not h["per_group"]
                    tiles += h["tiles"]
                    old += h["tiles_uniform"]
    assert chains >= 40, chains
    print("rate matrix: %d lean fused chains, %d table entries, tiles %d against %d of the uniform walk (%.1f %% fewer), "
          "uniform fallback %.1f %%" % (chains, entries, tiles, old, 100.0 * (old - tiles) / old, 100.0 * uni / entries))


def test_hook_is_inert_without_test_hooks():
    """RRX_debug_tile_walk answers only in a process started with RSMP_TEST_HOOKS (tests/conftest.py sets it)."""
    import subprocess
    import sys
    code = ("import sys, ctypes as C; sys.path.insert(0, %r)\n"
            "import foo_dsp_resampler_amd as F\n"
            "from foo_dsp_resampler_amd.ratelib import WalkGeom\n"
            "g = WalkGeom(at0=0, b_offset=0, B0=0, V=3542, polyL=160, step=147, n=24, KS=7, qb_min=0, qb_max=146, two_round=1)\n"
            "head = (C.c_longlong * 13)()\n"
            "print(F.lib().RRX_debug_tile_walk(C.byref(g), 1, head, None, 0))\n" % ROOT)
    env = {k: v for k, v in os.environ.items() if k != "RSMP_TEST_HOOKS"}
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-1] == "-1"
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(env, RSMP_TEST_HOOKS="1"))
    assert out.returncode == 0, out.stderr
    assert int(out.stdout.split()[-1]) > 0
