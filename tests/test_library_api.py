"""Reusable handles, host side ("Libraries"): the four new symbols, the process-wide plan cache behind every call that
needs a plan, and RRX_tracks_batches against a restatement in Python and against the brute-force optimum.  CPU only."""
import ctypes as C
import functools
import itertools
import json
import os
import threading

import numpy as np
import pytest

import foo_dsp_resampler_amd as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RR_OK, RR_NULLHANDLE, RR_INVPARAM = 0, 3, 6
NEW = ("RRX_reset", "RRX_tracks_batches", "RRX_plan_cache_clear", "RRX_plan_cache_stats")


def cfg(fs, fo, phase=50.0, bandwidth=95.0, aliasing=0, quality=F.RR_BEST):
    return F.RRConfig(fs, fo, phase, bandwidth, aliasing, quality)


def describe(c):
    buf = C.create_string_buffer(1 << 16)
    n = F.lib().RRX_describe_plan(C.byref(c), buf, len(buf))
    return n, buf.value.decode()


def table(c, which):
    n = C.c_size_t(0)
    assert F.lib().RRX_plan_table(C.byref(c), which, None, 0, C.byref(n)) == RR_OK
    out = np.full(n.value, np.nan)
    if n.value:
        assert F.lib().RRX_plan_table(C.byref(c), which, out.ctypes.data, n.value, C.byref(n)) == RR_OK
    return out


def test_symbols_are_exported_and_listed():
    header = open(os.path.join(ROOT, "include", "ratelib_amd.h")).read()
    for name in NEW:
        assert name in F.EXPECTED_SYMBOLS and name in F.available_symbols()
        assert name in header
    for name in ("tracks_batches", "plan_cache_clear", "plan_cache_stats"):
        assert callable(getattr(F, name))
    assert hasattr(F.Resampler, "reset") and hasattr(F.Resampler, "convert_library_to_pcm")
    assert F.lib().RRX_reset(None) == RR_NULLHANDLE


def test_second_lookup_is_a_hit_with_the_same_plan():
    F.plan_cache_clear()
    assert F.plan_cache_stats() == (0, 0, 0)
    c = cfg(44100, 48000, phase=25.0)
    n1, text1 = describe(c)
    assert n1 > 0 and F.plan_cache_stats() == (0, 1, 1)
    n2, text2 = describe(c)
    assert (n2, text2) == (n1, text1) and F.plan_cache_stats() == (1, 1, 1)
    assert json.loads(text1)["stages"]
    # any of the three pointers may be NULL
    h, e = C.c_ulonglong(9), C.c_int(9)
    assert F.lib().RRX_plan_cache_stats(C.byref(h), None, None) == RR_OK and h.value == 1
    assert F.lib().RRX_plan_cache_stats(None, None, C.byref(e)) == RR_OK and e.value == 1
    assert F.lib().RRX_plan_cache_stats(None, None, None) == RR_OK


def test_tables_are_the_same_bits_from_a_miss_and_from_a_hit():
    c = cfg(44100, 48000, phase=25.0)
    for which in (0, 1, 2):
        F.plan_cache_clear()
        cold = table(c, which)                        # (the count, then the values: the first call misses, the second is served)
        calls = 2 if len(cold) else 1
        assert F.plan_cache_stats() == (calls - 1, 1, 1)
        warm = table(c, which)
        assert F.plan_cache_stats() == (2 * calls - 1, 1, 1)
        F.plan_cache_clear()
        n = C.c_size_t(0)
        miss = np.full(len(cold), np.nan)             # ONE call on an empty cache: the designed plan itself
        assert F.lib().RRX_plan_table(C.byref(c), which, miss.ctypes.data, len(miss), C.byref(n)) == RR_OK
        assert F.plan_cache_stats() == (0, 1, 1) and n.value == len(cold)
        assert cold.tobytes() == warm.tobytes() == miss.tobytes()
        assert which == 1 or len(cold)
        assert not np.isnan(cold).any()


def test_a_config_that_differs_in_one_field_misses():
    F.plan_cache_clear()
    base = dict(fs=44100, fo=48000, phase=50.0, bandwidth=95.0, aliasing=0, quality=F.RR_BEST)
    assert describe(cfg(**base))[0] > 0
    others = [dict(base, fs=44101), dict(base, fo=48001), dict(base, phase=49.0), dict(base, bandwidth=94.0),
              dict(base, aliasing=1), dict(base, quality=F.RR_NORM)]
    for k, o in enumerate(others):
        assert describe(cfg(**o))[0] > 0
        assert F.plan_cache_stats() == (0, 2 + k, 2 + k), o
    assert describe(cfg(**base))[0] > 0
    assert F.plan_cache_stats() == (1, 7, 7)
    # the doubles are compared by bit pattern: -0.0 is not 0.0
    assert describe(cfg(**dict(base, phase=0.0)))[0] > 0 and describe(cfg(**dict(base, phase=-0.0)))[0] > 0
    assert F.plan_cache_stats() == (1, 9, 9)


def test_a_refused_config_is_not_cached():
    F.plan_cache_clear()
    for bad in (cfg(1, 100000), cfg(0, 48000), cfg(44100, 48000, phase=101.0), cfg(44100, 48000, bandwidth=20.0)):
        for _ in range(2):
            assert describe(bad)[0] == -RR_INVPARAM
    hits, misses, entries = F.plan_cache_stats()
    assert (hits, entries) == (0, 0) and misses == 8


def test_seventeen_configs_leave_sixteen_and_the_oldest_is_gone():
    F.plan_cache_clear()
    cfgs = [cfg(44100, 48000, bandwidth=90.0 + 0.25 * k) for k in range(17)]
    texts = [describe(c) for c in cfgs]
    assert all(n > 0 for n, _ in texts)
    assert F.plan_cache_stats() == (0, 17, 16)
    assert describe(cfgs[16]) == texts[16] and F.plan_cache_stats() == (1, 17, 16)     # the newest is there
    assert describe(cfgs[0]) == texts[0] and F.plan_cache_stats() == (1, 18, 16)       # the first one was evicted: designed again
    # least recently USED: that insertion took 1, so 2 is now the oldest entry; touching it saves it from the next eviction, which takes 3
    assert describe(cfgs[2]) == texts[2] and F.plan_cache_stats() == (2, 18, 16)
    assert describe(cfg(44100, 48000, bandwidth=99.0))[0] > 0 and F.plan_cache_stats() == (2, 19, 16)
    assert describe(cfgs[2]) == texts[2] and F.plan_cache_stats() == (3, 19, 16)
    assert describe(cfgs[3]) == texts[3] and F.plan_cache_stats() == (3, 20, 16)


def test_eight_threads_on_four_configs_get_the_right_text():
    cfgs = [cfg(44100, 48000), cfg(44100, 96000), cfg(96000, 44100), cfg(44100, 48000, phase=25.0)]
    want = [describe(c) for c in cfgs]
    assert len({t for _, t in want}) == 4
    F.plan_cache_clear()                              # the threads start on an empty cache: misses, hits and insertions side by side
    wrong, start = [], threading.Barrier(8)

    def work(t):
        start.wait()
        for r in range(12):
            k = (t + r) % 4
            if describe(cfgs[k]) != want[k]:
                wrong.append((t, r, k))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not wrong
    hits, misses, entries = F.plan_cache_stats()
    assert entries == 4 and hits + misses == 96 and 4 <= misses <= 32


# ---- RRX_tracks_batches

FS, FO = 44100, 48000
# shuffled, with a tie (65 twice), both sides of the 64-frame branch and an empty track
POOL = [65, 0, 3000, 64, 20011, 65, 40]


@functools.lru_cache(maxsize=None)
def ext_frames(frames):
    return F.track_geometry(FS, FO, frames)[1]


def restated(lengths, nstreams):
    """RRX_tracks_batches in Python over RRX_track_geometry: (order, row_frames, resampled, useful)"""
    order = sorted(range(len(lengths)), key=lambda i: (-lengths[i], i))
    rows = [max(ext_frames(lengths[i]) for i in order[k:k + nstreams]) for k in range(0, len(order), nstreams)]
    return order, rows, nstreams * sum(rows), sum(ext_frames(v) for v in lengths)


def partitions(items, most):
    """every partition of `items` into blocks of at most `most`"""
    if not items:
        yield []
        return
    first, rest = items[0], items[1:]
    for k in range(0, most):
        for mates in itertools.combinations(range(len(rest)), k):
            left = [v for i, v in enumerate(rest) if i not in mates]
            for p in partitions(left, most):
                yield [[first] + [rest[i] for i in mates]] + p


def test_partitions_helper_counts_bell_numbers():
    assert sum(1 for _ in partitions(list(range(7)), 7)) == 877
    assert sum(1 for _ in partitions(list(range(4)), 2)) == 10


def test_batches_agree_with_the_restatement():
    lengths = [100, 0, 1500, 64, 65, 0, 0, 30000, 1500, 40, 100000]
    for nstreams in (1, 2, 3, 4, 11, 64):
        tb = F.tracks_batches(FS, FO, lengths, nstreams)
        order, rows, resampled, useful = restated(lengths, nstreams)
        assert (tb.order, tb.row_frames, tb.resampled, tb.useful) == (order, rows, resampled, useful)
        assert len(tb) == -(-len(lengths) // nstreams) and tb.batches == [order[k:k + nstreams] for k in range(0, len(order), nstreams)]
        for b, idx in enumerate(tb.batches):          # row_frames[b] IS RRX_tracks_plan's answer for the batch
            assert F.tracks_plan(FS, FO, [lengths[i] for i in idx]).row_frames == tb.row_frames[b]
        assert tb.padding == 1 - useful / resampled
    only_empty = F.tracks_batches(FS, FO, [0, 0, 0], 2)
    assert (only_empty.row_frames, only_empty.resampled, only_empty.useful, only_empty.padding) == ([0, 0], 0, 0, 0.0)


@pytest.mark.parametrize("nstreams", [2, 3])
def test_the_split_is_optimal_by_brute_force(nstreams):
    """every sub-list of POOL (in POOL's order, 127 of them, up to all 7 tracks): sum(row_frames) is the minimum over all set
    partitions with blocks of at most nstreams"""
    checked = 0
    for k in range(1, len(POOL) + 1):
        for pick in itertools.combinations(range(len(POOL)), k):
            lengths = [POOL[i] for i in pick]
            tb = F.tracks_batches(FS, FO, lengths, nstreams)
            order, rows, resampled, useful = restated(lengths, nstreams)
            assert (tb.order, tb.row_frames, tb.resampled, tb.useful) == (order, rows, resampled, useful), lengths
            exts = [ext_frames(v) for v in lengths]
            best = min(sum(max(block) for block in p) for p in partitions(exts, nstreams))
            assert sum(tb.row_frames) == best, (lengths, tb.row_frames, best)
            checked += 1
    assert checked == 127


def batches_raw(c, lengths, nstreams, ntracks=None, null=()):
    n = len(lengths)
    fr = (C.c_size_t * max(n, 1))(*lengths)
    order = (C.c_int * max(n, 1))(*([-7] * max(n, 1)))
    rows = (C.c_size_t * max(n, 1))(*([0xdead] * max(n, 1)))
    nb, res, use = C.c_int(-7), C.c_ulonglong(0xdead), C.c_ulonglong(0xdead)
    args = dict(config=C.byref(c) if c is not None else None, frames=fr, order=order, rows=rows, nb=C.byref(nb), res=C.byref(res), use=C.byref(use))
    for k in null:
        args[k] = None
    rc = F.lib().RRX_tracks_batches(args["config"], args["frames"], n if ntracks is None else ntracks, nstreams, args["order"], args["rows"],
                                    args["nb"], args["res"], args["use"])
    return rc, list(order), list(rows), nb.value, res.value, use.value


def test_every_refusal_is_returned():
    good = cfg(FS, FO)
    rc, order, rows, nb, res, use = batches_raw(good, [100, 200, 50], 2)
    assert (rc, order, nb) == (RR_OK, [1, 0, 2], 2) and rows[:2] == [ext_frames(200), ext_frames(50)]
    for k in ("config", "frames", "order", "nb"):
        rc, _, _, nb, res, use = batches_raw(good, [100, 200, 50], 2, null=(k,))
        assert rc == RR_INVPARAM, k
        assert (nb, res, use) == (-7, 0xdead, 0xdead), k          # a refused call reports nothing
    for k in ("rows", "res", "use"):                               # these three may be NULL
        rc, order, _, nb, _, _ = batches_raw(good, [100, 200, 50], 2, null=(k,))
        assert (rc, order, nb) == (RR_OK, [1, 0, 2], 2), k
    assert batches_raw(good, [100], 2, ntracks=0)[0] == RR_INVPARAM
    assert batches_raw(good, [100], 2, ntracks=-1)[0] == RR_INVPARAM
    assert batches_raw(good, [100], 0)[0] == RR_INVPARAM
    assert batches_raw(good, [100], -3)[0] == RR_INVPARAM
    assert batches_raw(cfg(1, 100000), [100], 2)[0] == RR_INVPARAM      # a ratio the planner refuses (rate_base.h:528)
    assert batches_raw(cfg(0, 48000), [100], 2)[0] == RR_INVPARAM
    assert batches_raw(good, [2 ** 64 - 1], 2)[0] == RR_INVPARAM
    assert batches_raw(good, [100, 2 ** 36 + 1], 2)[0] == RR_INVPARAM   # above what the call walks
    assert batches_raw(good, [2 ** 63, 5, 2 ** 63], 2)[0] == RR_INVPARAM
    with pytest.raises(ValueError):
        F.tracks_batches(FS, FO, [], 2)
    with pytest.raises(ValueError):
        F.tracks_batches(FS, FO, [10, -1], 2)
    with pytest.raises(F.RRError):
        F.tracks_batches(FS, FO, [10], 0)
