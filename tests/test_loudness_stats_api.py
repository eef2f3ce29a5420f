"""The loudness meter's host side (RRX_loudness_blocks_device / RRX_loudness_gate_groups_device / RRX_loudness_range_groups_device
and their host twins): the symbols, the refusals that need no device, the Python wrappers' checks, the arithmetic -- the twins are
serial loops over the very functions the kernels call -- against the numpy restatement in loudness_stats_model.py, bit for bit, the
one-stream identity with RRX_debug_loudness_gate_host, and known answers (EBU Tech 3342, album gating).  CPU only."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import foo_dsp_resampler_amd as F
import loudness_model as M
import loudness_stats_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RR_OK, RR_EXTUNINIT, RR_INVPARAM = 0, 5, 6
GUARD = 777.25
NGUARD = 12345
NAMES = ("RRX_loudness_blocks_device", "RRX_loudness_groups_work_doubles", "RRX_loudness_gate_groups_device",
         "RRX_loudness_range_groups_device", "RRX_debug_loudness_blocks_host", "RRX_debug_loudness_gate_groups_host",
         "RRX_debug_loudness_range_groups_host")
SHAPES = [(1, 1), (4, 1), (30, 1), (30, 10), (3, 2), (5, 7)]
W6 = [1.0, 1.0, 1.0, 0.0, 1.41, 1.41]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """equal bit patterns, or NaN in both: the T of an empty group is 0 / 0, whose sign is the processor's"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def ptr(a):
    return None if a is None else a.ctypes.data


def blocks_host(energy, hop, L, P, hops=None, weights=None, nhops=None, stride=None, blocks=True, nblocks=True, top=True):
    """RRX_debug_loudness_blocks_host on energy [nstreams, nch, energy_stride]: (blocks [nstreams, stride] with the guard value
    where nothing was written, nblocks, max), None for an output that was not asked for; every output lies under guards"""
    ns, nch, es = energy.shape
    energy = np.ascontiguousarray(energy)
    nhops = es if nhops is None else nhops
    stride = max(S.count(nhops, L, P), 1) if stride is None else stride
    b = np.full(ns * stride + 3, GUARD)
    nb = np.full(ns + 2, NGUARD, np.uint64)
    mx = np.full(ns + 2, GUARD)
    h = None if hops is None else np.ascontiguousarray(hops, dtype=np.uint64)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    rc = F.lib().RRX_debug_loudness_blocks_host(energy.ctypes.data, es, ns, nch, nhops, ptr(h), ptr(w), hop, L, P, b.ctypes.data if blocks else None,
                                                stride if blocks else 0, nb.ctypes.data if nblocks else None, mx.ctypes.data if top else None)
    assert rc == RR_OK
    assert np.all(b[ns * stride:] == GUARD) and np.all(nb[ns:] == NGUARD) and np.all(mx[ns:] == GUARD)
    if not blocks:
        assert np.all(b == GUARD)
    return (b[:ns * stride].reshape(ns, stride) if blocks else None, nb[:ns] if nblocks else None, mx[:ns] if top else None)


def groups_host(rows, nblocks, group, ngroups, abs_threshold, rel_factor, percentiles=None, extra_work=3):
    """the gate (percentiles None) or the range twin on blocks [nstreams, stride]: [ngroups, 4], with result and work under guards"""
    ns, stride = rows.shape
    rows = np.ascontiguousarray(rows)
    need = F.lib().RRX_loudness_groups_work_doubles(ns, ngroups)
    assert need == 2 * ns + ngroups
    work = np.full(need + extra_work, GUARD)
    res = np.full(ngroups * 4 + 2, GUARD)
    nb = np.ascontiguousarray(nblocks, dtype=np.uint64)
    gr = np.ascontiguousarray(group, dtype=np.int32)
    if percentiles is None:
        rc = F.lib().RRX_debug_loudness_gate_groups_host(rows.ctypes.data, stride, ns, nb.ctypes.data, gr.ctypes.data, ngroups, abs_threshold, rel_factor,
                                                         res.ctypes.data, work.ctypes.data, need)
    else:
        rc = F.lib().RRX_debug_loudness_range_groups_host(rows.ctypes.data, stride, ns, nb.ctypes.data, gr.ctypes.data, ngroups, abs_threshold, rel_factor,
                                                          percentiles[0], percentiles[1], res.ctypes.data, work.ctypes.data, need)
    assert rc == RR_OK
    assert np.all(work[need:] == GUARD) and np.all(res[ngroups * 4:] == GUARD)
    return res[:ngroups * 4].reshape(ngroups, 4)


def test_symbols_are_exported_listed_and_declared():
    header = open(os.path.join(ROOT, "include", "ratelib_amd.h")).read()
    for name in NAMES:
        assert name in F.EXPECTED_SYMBOLS and name in F.available_symbols()
        assert name + "(" in header
    for name in ("loudness_blocks_device", "loudness_gate_groups_device", "loudness_range_device", "loudness_range_lu", "loudness_meter_device"):
        assert callable(getattr(F, name))
    assert "has the bits of RRX_loudness_gate_device" in header and "costs its longest stream's serial walk" in header
    hpp = open(os.path.join(ROOT, "foo_dsp_resampler_amd", "csrc", "loudness_stats.hpp")).read()
    assert "has the bits of loudness.hpp's loudness_block" in hpp
    L = F.lib()
    assert L.RRX_loudness_groups_work_doubles(3, 2) == 8 and L.RRX_loudness_groups_work_doubles(256, 256) == 768
    assert L.RRX_loudness_groups_work_doubles(0, 2) == 0 and L.RRX_loudness_groups_work_doubles(3, 0) == 0 and L.RRX_loudness_groups_work_doubles(-1, -1) == 0


CHILD = r"""
import sys, ctypes as C
sys.path.insert(0, %r)
import foo_dsp_resampler_amd as F
L = F.lib()
cb = F.ratelib._ALLOC_CB(lambda: None)
p = 0x10000  # never dereferenced: every call below is answered from its arguments, or from the library's state, alone
nan, inf = float("nan"), float("inf")
bgood = dict(device=-1, stream=None, energy=p, es=40, nstreams=3, nch=2, nhops=40, hops=None, weights=None, hop=100, L=4, P=1, blocks=p, bs=37,
             nblocks=p, max=p)
def bcall(**kw):
    a = dict(bgood, **kw)
    return L.RRX_loudness_blocks_device(a["device"], a["stream"], a["energy"], a["es"], a["nstreams"], a["nch"], a["nhops"], a["hops"], a["weights"],
                                        a["hop"], a["L"], a["P"], a["blocks"], a["bs"], a["nblocks"], a["max"])
ggood = dict(device=-1, stream=None, blocks=p, bs=37, nstreams=3, nblocks=p, group=p, ngroups=2, abs=1e-7, rel=0.1, low=10, high=95, result=p, work=p,
             wd=8)
def gcall(**kw):
    a = dict(ggood, **kw)
    return L.RRX_loudness_gate_groups_device(a["device"], a["stream"], a["blocks"], a["bs"], a["nstreams"], a["nblocks"], a["group"], a["ngroups"],
                                             a["abs"], a["rel"], a["result"], a["work"], a["wd"])
def rcall(**kw):
    a = dict(ggood, **kw)
    return L.RRX_loudness_range_groups_device(a["device"], a["stream"], a["blocks"], a["bs"], a["nstreams"], a["nblocks"], a["group"], a["ngroups"],
                                              a["abs"], a["rel"], a["low"], a["high"], a["result"], a["work"], a["wd"])
print("uninit", bcall(), gcall(), rcall())                # before init_ratelib
print("init", L.init_ratelib(cb))                         # no device: refuses
print("uninit", bcall(), gcall(), rcall())
for name, kw in [("energy", dict(energy=None)), ("nstreams0", dict(nstreams=0)), ("nstreams-1", dict(nstreams=-1)), ("nch0", dict(nch=0)),
                 ("hop0", dict(hop=0)), ("nhops", dict(nhops=41)), ("energy2^60", dict(es=2**58, nhops=0)), ("L0", dict(L=0)), ("P0", dict(P=0)),
                 ("no-output", dict(blocks=None, nblocks=None, max=None)), ("stride0", dict(bs=0)), ("blocks2^60", dict(bs=2**59)),
                 ("blocks2^60-unused", dict(blocks=None, bs=2**59)), ("device-2", dict(device=-2))]:
    print("binv", name, bcall(**kw))
for name, kw in [("hops", dict(hops=p)), ("weights", dict(weights=p)), ("max-only", dict(blocks=None, bs=0, nblocks=None)), ("no-max", dict(max=None)),
                 ("no-count", dict(nblocks=None)), ("range-blocks", dict(L=30, P=10)), ("longer-than-the-stream", dict(L=100)),
                 ("short-rows", dict(bs=1)), ("nhops0", dict(nhops=0))]:
    print("bok", name, bcall(**kw))
common = [("blocks", dict(blocks=None)), ("nblocks", dict(nblocks=None)), ("group", dict(group=None)), ("result", dict(result=None)),
          ("work", dict(work=None)), ("nstreams0", dict(nstreams=0)), ("ngroups0", dict(ngroups=0)), ("ngroups-1", dict(ngroups=-1)),
          ("nan-abs", dict(abs=nan)), ("nan-rel", dict(rel=nan)), ("work-short", dict(wd=7)), ("blocks2^60", dict(bs=2**59)), ("device-2", dict(device=-2))]
for name, kw in common:
    print("ginv", name, gcall(**kw))
for name, kw in [("more-work", dict(wd=100)), ("one-group", dict(ngroups=1, wd=7)), ("no-abs-gate", dict(abs=-inf)), ("stride0", dict(bs=0)),
                 ("many-groups", dict(ngroups=1000, wd=1006))]:
    print("gok", name, gcall(**kw))
for name, kw in common + [("low-1", dict(low=-1)), ("low101", dict(low=101)), ("high-1", dict(high=-1)), ("high101", dict(high=101)),
                          ("abs-negative", dict(abs=-1e-9)), ("abs-inf", dict(abs=-inf))]:
    print("rinv", name, rcall(**kw))
for name, kw in [("more-work", dict(wd=100)), ("all", dict(low=0, high=100)), ("crossed", dict(low=95, high=10)), ("median", dict(low=50, high=50)),
                 ("abs0", dict(abs=0.0)), ("abs-0", dict(abs=-0.0)), ("abs+inf", dict(abs=inf))]:
    print("rok", name, rcall(**kw))
"""


def test_invalid_parameters_are_refused_without_a_device():
    out = subprocess.run([sys.executable, "-c", CHILD % ROOT], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))
    assert out.returncode == 0, out.stderr
    kinds = ("uninit", "init", "binv", "bok", "ginv", "gok", "rinv", "rok")
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.split() and ln.split()[0] in kinds]
    assert ["init", "-1"] in lines
    uninit = [ln for ln in lines if ln[0] == "uninit"]
    assert len(uninit) == 2 and all(int(v) == RR_EXTUNINIT for ln in uninit for v in ln[1:])
    for kind, count, want in (("binv", 14, RR_INVPARAM), ("bok", 9, RR_EXTUNINIT), ("ginv", 13, RR_INVPARAM), ("gok", 5, RR_EXTUNINIT),
                              ("rinv", 19, RR_INVPARAM), ("rok", 7, RR_EXTUNINIT)):
        got = [ln for ln in lines if ln[0] == kind]
        assert len(got) == count and all(int(ln[2]) == want for ln in got), got


def test_host_twins_refuse_as_the_device_calls_do_and_leave_the_results_alone():
    L = F.lib()
    energy = np.full((2, 2, 40), 3.0)
    b, nb, mx = np.full((2, 37), 5.0), np.full(2, 6, np.uint64), np.full(2, 7.0)

    def bcall(**kw):
        return L.RRX_debug_loudness_blocks_host(kw.get("energy", energy.ctypes.data), kw.get("es", 40), kw.get("ns", 2), kw.get("nch", 2),
                                                kw.get("nhops", 40), None, None, kw.get("hop", 100), kw.get("L", 4), kw.get("P", 1),
                                                kw.get("blocks", b.ctypes.data), kw.get("bs", 37), kw.get("nblocks", nb.ctypes.data),
                                                kw.get("max", mx.ctypes.data))

    for kw in (dict(energy=None), dict(ns=0), dict(nch=0), dict(hop=0), dict(nhops=41), dict(L=0), dict(P=0), dict(blocks=None, nblocks=None, max=None),
               dict(bs=0), dict(bs=2 ** 59)):
        assert bcall(**kw) == RR_INVPARAM, kw
        assert np.all(b == 5.0) and np.all(nb == 6) and np.all(mx == 7.0), kw
    assert bcall() == RR_OK and np.all(nb == 37) and np.all(b == 24.0 * (1.0 / 400.0)) and np.all(mx == 24.0 * (1.0 / 400.0))
    group = np.array([0, 1], np.int32)
    res, work = np.full((2, 4), 8.0), np.full(6, 9.0)

    def gcall(fn, **kw):
        head = (kw.get("blocks", b.ctypes.data), kw.get("bs", 37), kw.get("ns", 2), kw.get("nblocks", nb.ctypes.data), kw.get("group", group.ctypes.data),
                kw.get("ngroups", 2), kw.get("abs", 1e-7), kw.get("rel", 0.1))
        tail = (kw.get("result", res.ctypes.data), kw.get("work", work.ctypes.data), kw.get("wd", 6))
        if fn is L.RRX_debug_loudness_range_groups_host:
            return fn(*(head + (kw.get("low", 10), kw.get("high", 95)) + tail))
        return fn(*(head + tail))

    refused = [dict(blocks=None), dict(nblocks=None), dict(group=None), dict(result=None), dict(work=None), dict(ns=0), dict(ngroups=0),
               dict(abs=float("nan")), dict(rel=float("nan")), dict(wd=5), dict(bs=2 ** 59)]
    for fn, more in ((L.RRX_debug_loudness_gate_groups_host, []),
                     (L.RRX_debug_loudness_range_groups_host, [dict(low=-1), dict(high=101), dict(abs=-1e-9)])):
        for kw in refused + more:
            assert gcall(fn, **kw) == RR_INVPARAM, kw
            assert np.all(res == 8.0) and np.all(work == 9.0), kw
        assert gcall(fn) == RR_OK and not np.any(res == 8.0)
        res[:] = 8.0
        work[:] = 9.0
    code = ("import sys; sys.path.insert(0, %r)\nimport foo_dsp_resampler_amd as F\nL = F.lib()\n"
            "print(L.RRX_debug_loudness_blocks_host(None, 0, 1, 1, 0, None, None, 1, 1, 1, None, 0, None, None))\n"
            "print(L.RRX_debug_loudness_gate_groups_host(None, 0, 1, None, None, 1, 0.0, 0.1, None, None, 0))\n"
            "print(L.RRX_debug_loudness_range_groups_host(None, 0, 1, None, None, 1, 0.0, 0.1, 10, 95, None, None, 0))\n" % ROOT)
    env = {k: v for k, v in os.environ.items() if k != "RSMP_TEST_HOOKS"}
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-3:] == ["-1", "-1", "-1"]


def test_python_wrappers_check_on_the_host():
    class Fake:  # stands in for a device tensor: the wrapper must refuse before any C call
        is_cuda = True
        device = "cuda:0"

        def __init__(self, shape, dtype=torch.float64, contiguous=True):
            self.shape, self.dtype, self._c = shape, dtype, contiguous

        def dim(self):
            return len(self.shape)

        def is_contiguous(self):
            return self._c

        def data_ptr(self):
            raise AssertionError("the arguments are checked before the pointer is taken")

    e = Fake((3, 2, 40))
    with pytest.raises(TypeError):
        F.loudness_blocks_device(torch.zeros((3, 2, 40), dtype=torch.float64), 4800, 4)  # not on the device
    with pytest.raises(TypeError):
        F.loudness_blocks_device(Fake((3, 2, 40), dtype=torch.float32), 4800, 4)
    with pytest.raises(TypeError):
        F.loudness_blocks_device(Fake((3, 40)), 4800, 4)
    with pytest.raises(TypeError):
        F.loudness_blocks_device(Fake((3, 2, 40), contiguous=False), 4800, 4)
    for kw in (dict(hop=0, block_hops=4), dict(hop=4800, block_hops=0), dict(hop=4800, block_hops=4, step_hops=0)):
        with pytest.raises(ValueError):
            F.loudness_blocks_device(e, **kw)
    with pytest.raises(TypeError):
        F.loudness_blocks_device(e, 4800, 4, hops=Fake((2,), dtype=torch.int64))
    with pytest.raises(TypeError):
        F.loudness_meter_device(torch.zeros((3, 2, 40), dtype=torch.float64), 4800)
    b, nb = Fake((3, 37)), Fake((3,), dtype=torch.int64)
    for fn in (F.loudness_gate_groups_device, F.loudness_range_device):
        with pytest.raises(TypeError):
            fn(torch.zeros((3, 37), dtype=torch.float64), torch.zeros(3, dtype=torch.int64), [0, 0, 1], 2)  # not on the device
        with pytest.raises(TypeError):
            fn(Fake((3, 37), dtype=torch.float32), nb, [0, 0, 1], 2)
        with pytest.raises(TypeError):
            fn(b, Fake((2,), dtype=torch.int64), [0, 0, 1], 2)
        with pytest.raises(TypeError):
            fn(b, Fake((3,), dtype=torch.int32), [0, 0, 1], 2)
        with pytest.raises(ValueError):
            fn(b, nb, [0, 0, 1], None)  # groups without their number
        with pytest.raises(TypeError):
            fn(b, nb, Fake((3,), dtype=torch.int64), 2)
    for low, high in ((-1, 95), (10, 101)):
        with pytest.raises(ValueError):
            F.loudness_range_device(b, nb, low=low, high=high)
    r = torch.tensor([[1.0, 10.0, 5.0, 0.1], [0.0, 0.0, 0.0, float("nan")]], dtype=torch.float64)
    assert F.loudness_range_lu(r).tolist() == [10.0, 0.0] and F.loudness_range_lu(r.numpy()).tolist() == [10.0, 0.0]


def lengths(L, P):
    return [0, L - 1, L, L + 1, L + P - 1, L + P, 300, 601]


def energies(nch, seed, ns=8, nh=601):
    """hop energies with a quiet stretch the relative gate removes and one under the absolute gate"""
    rng = np.random.default_rng(seed)
    e = rng.uniform(1.0, 50.0, (ns, nch, nh))
    e[:, :, 100:220] *= 0.01
    e[:, :, 250:290] *= 1e-12
    return e


def weights_of(nch):
    return {1: [1.41], 2: [0.0, 1.41], 6: W6}[nch]


@pytest.mark.parametrize("L,P", SHAPES)
@pytest.mark.parametrize("nch", [1, 2, 6])
def test_host_twins_equal_the_model_bit_for_bit(nch, L, P):
    hop = 4800
    e = energies(nch, nch * 100 + L * 10 + P)
    hops = lengths(L, P)  # ragged d_hops: one stream per length
    groups = [2, 0, -1, 0, 2, 5, 1, 0]
    for weights in (None, weights_of(nch)):
        zs, nbs, top = S.blocks(e, hop, L, P, hops=hops, weights=weights)
        b, nb, mx = blocks_host(e, hop, L, P, hops=hops, weights=weights)
        assert np.array_equal(nb, nbs) and list(nb) == [S.count(n, L, P) for n in hops]
        assert np.array_equal(bits(b), bits(S.as_rows(zs, b.shape[1], GUARD)))  # the blocks, and the guard value where there is none
        assert np.array_equal(bits(mx), bits(top)) and mx[0] == 0.0 and mx[1] == 0.0 and np.all(mx[2:] > 0)
        only, _, _ = blocks_host(e, hop, L, P, hops=hops, weights=weights, nblocks=False, top=False)
        assert np.array_equal(bits(only), bits(b))
        _, nb1, mx1 = blocks_host(e, hop, L, P, hops=hops, weights=weights, blocks=False)  # without d_blocks nothing clamps the count
        assert np.array_equal(nb1, nbs) and np.array_equal(bits(mx1), bits(top))
        for stride in (1, 50):  # blocks_stride smaller than nb: the count, the rows and the maximum stop there
            zc, nbc, topc = S.blocks(e, hop, L, P, hops=hops, weights=weights, stride=stride)
            bc, nc, mc = blocks_host(e, hop, L, P, hops=hops, weights=weights, stride=stride)
            assert np.array_equal(nc, nbc) and nc.max() == stride
            assert np.array_equal(bits(bc), bits(S.as_rows(zc, stride, GUARD))) and np.array_equal(bits(mc), bits(topc))
        for thresholds, low, high in ((S.gate_thresholds(), 10, 95), (S.gate_thresholds(-70.0, -20.0), 10, 95), (S.gate_thresholds(-30.0, -3.0), 0, 100),
                                      (S.gate_thresholds(-70.0, -20.0), 95, 10), ((0.0, 0.5), 50, 50)):
            for gr, ng in ((groups, 4), ([0] * 8, 1), (list(range(8)), 8)):
                got = groups_host(b, nb, gr, ng, *thresholds)
                want = S.gate_groups(zs, gr, ng, *thresholds)
                assert np.array_equal(bits(got), bits(want)), (thresholds, gr)
                got = groups_host(b, nb, gr, ng, *thresholds, percentiles=(low, high))
                want = S.range_groups(zs, gr, ng, *thresholds, low=low, high=high)
                assert same(got, want), (thresholds, gr, low, high)
        res = groups_host(b, nb, groups, 4, *S.gate_thresholds())
        assert not bits(res[3]).any()  # no stream names group 3: {+0.0, 0, +0.0, 0}


def test_nblocks_are_read_clamped_and_foreign_groups_are_ignored():
    e = energies(2, 7, ns=3, nh=120)
    zs, nbs, _ = S.blocks(e, 4800, 4, 1)
    b, nb, _ = blocks_host(e, 4800, 4, 1)
    thresholds = S.gate_thresholds()
    want = S.gate_groups(zs, [0, 0, 0], 1, *thresholds)
    assert np.array_equal(bits(groups_host(b, [10 ** 9, 117, 2 ** 63], [0, 0, 0], 1, *thresholds)), bits(want))
    want = S.gate_groups(zs, [0, -1, -1], 1, *thresholds)
    for foreign in ([0, -1, 1], [0, 2 ** 31 - 1, -2 ** 31]):
        assert np.array_equal(bits(groups_host(b, nb, foreign, 1, *thresholds)), bits(want))
    want = S.range_groups(zs, [0, -1, -1], 1, *S.gate_thresholds(-70.0, -20.0))
    assert np.array_equal(bits(groups_host(b, [10 ** 9, 5, 5], [0, 7, -7], 1, *S.gate_thresholds(-70.0, -20.0), percentiles=(10, 95))), bits(want))


def gate_host(energy, hop, hops=None, weights=None):
    ns, nch, stride = energy.shape
    energy = np.ascontiguousarray(energy)
    res = np.full((ns, 4), GUARD)
    h = None if hops is None else np.ascontiguousarray(hops, dtype=np.uint64)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    a, r = F.loudness_gate()
    assert F.lib().RRX_debug_loudness_gate_host(energy.ctypes.data, stride, ns, nch, stride, ptr(h), ptr(w), hop, a, r, res.ctypes.data) == RR_OK
    return res


@pytest.mark.parametrize("nch", [1, 2, 6])
def test_one_stream_groups_over_400_ms_blocks_have_the_bits_of_the_stream_gate(nch):
    e = energies(nch, nch)
    e[5, nch - 1, 400] = np.nan  # four blocks to skip
    hops = [0, 3, 4, 5, 300, 601, 601, 601]
    for weights in (None, weights_of(nch)):
        b, nb, _ = blocks_host(e, 4800, 4, 1, hops=hops, weights=weights)
        got = groups_host(b, nb, list(range(8)), 8, *F.loudness_gate())
        want = gate_host(e, 4800, hops=hops, weights=weights)
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(want), bits(M.gate(e, 4800, hops=hops, weights=weights)))
        assert got[1, 3] == 0 and got[2, 3] == 1 and got[3, 3] == 2  # three, four and five hops: no block, one, two


RATE, HOP = 8000, 800


def tone(pieces, seconds=20.0):
    """one phase-continuous 1 kHz stereo sine at RATE with `seconds` at each level of `pieces` (dBFS)"""
    amp = np.concatenate([np.full(int(round(seconds * RATE)), 10.0 ** (db / 20.0)) for db in pieces])
    t = np.arange(amp.size) / RATE
    return np.repeat((amp * np.sin(2 * np.pi * 1000.0 * t))[:, None], 2, axis=1)


def hop_energies(x):
    """RRX_debug_loudness_host on one stream x [frames, 2]: [1, 2, frames // HOP]"""
    x = np.ascontiguousarray(x[None])
    n = x.shape[1] // HOP
    work = np.zeros(F.lib().RRX_loudness_work_doubles(1, 2, x.shape[1], HOP))
    energy = np.zeros((1, 2, n))
    co = np.array(F.k_weighting(RATE))
    rc = F.lib().RRX_debug_loudness_host(1, x.ctypes.data, x.shape[1], 1, x.shape[1], 2, None, 0, co.ctypes.data, HOP, None, None, energy.ctypes.data, n,
                                         work.ctypes.data, work.size)
    assert rc == RR_OK
    return energy


_tones = {}


def tone_energies(pieces):
    if pieces not in _tones:
        _tones[pieces] = hop_energies(tone(pieces))
    return _tones[pieces]


@pytest.mark.parametrize("pieces,want,n30_10,n30_1", [((-20.0, -30.0), 10.0, 38, 371), ((-20.0, -15.0), 5.0, 38, 371), ((-40.0, -20.0), 20.0, 38, 371),
                                                      ((-50.0, -35.0, -20.0, -35.0, -50.0), 15.0, 62, 627)], ids=["1", "2", "3", "4"])
def test_ebu_tech_3342_sequences(pieces, want, n30_10, n30_1):
    """EBU Tech 3342 test cases 1 to 4 with a 1 kHz stereo tone at a rate of 8000, 20 s per level: the standard allows +-1 LU;
    this arithmetic gives the steps to 1e-13 LU, because both percentiles land on blocks that lie wholly inside one level"""
    e = tone_energies(pieces)
    thresholds = S.gate_thresholds(-70.0, -20.0)
    for (L, P), count in (((30, 10), n30_10), ((30, 1), n30_1)):
        b, nb, _ = blocks_host(e, HOP, L, P)
        res = groups_host(b, nb, [0], 1, *thresholds, percentiles=(10, 95))
        zs, _, _ = S.blocks(e, HOP, L, P)
        assert np.array_equal(bits(res), bits(S.range_groups(zs, [0], 1, *thresholds)))
        lra = float(F.loudness_range_lu(torch.from_numpy(res))[0])
        print("%r on (%d, %d) blocks: LRA %.13f LU, N2 %d" % (pieces, L, P, lra, res[0, 2]))
        assert abs(lra - want) <= 1e-6 and res[0, 2] == count
        assert abs(float(S.range_lu(res)[0]) - lra) <= 1e-12


def integrated(energy_rows, groups, ngroups):
    """LUFS per group over the (4, 1) blocks of streams given as a list of [1, 2, n] energies of unequal length"""
    n = max(e.shape[2] for e in energy_rows)
    e = np.zeros((len(energy_rows), 2, n))
    for s, row in enumerate(energy_rows):
        e[s, :, :row.shape[2]] = row[0]
    b, nb, _ = blocks_host(e, HOP, 4, 1, hops=[row.shape[2] for row in energy_rows])
    res = groups_host(b, nb, groups, ngroups, *F.loudness_gate())
    return F.integrated_lufs(torch.from_numpy(res)).numpy()


def test_momentary_short_term_and_album_known_answers():
    x = tone((-20.0, -30.0))
    whole, first, second = tone_energies((-20.0, -30.0)), hop_energies(x[:20 * RATE]), hop_energies(x[20 * RATE:])
    _, _, m4 = blocks_host(whole, HOP, 4, 1, blocks=False)
    _, _, m30 = blocks_host(whole, HOP, 30, 1, blocks=False)
    momentary, short_term = S.power_lufs(m4)[0], S.power_lufs(m30)[0]
    a, b = integrated([first, second], [0, 1], 2)
    print("momentary max %.6f, short-term max %.6f, first half %.6f, second half %.6f LUFS" % (momentary, short_term, a, b))
    assert abs(momentary - short_term) <= 1e-3 and abs(momentary - a) <= 1e-3 and abs(short_term - a) <= 1e-3
    assert abs(a - -19.980) <= 2e-3 and abs(b - -29.980) <= 2e-3
    album = integrated([first, second], [0, 0], 1)[0]
    one = integrated([whole], [0], 1)[0]
    pooled = 10.0 * np.log10((10.0 ** (a / 10.0) + 10.0 ** (b / 10.0)) / 2.0)
    print("album %.6f LUFS, the 40 s stream %.6f, the mean of the two tracks' powers %.6f" % (album, one, pooled))
    assert abs(album - pooled) <= 1e-3 and abs(album - -22.5768) <= 1e-3 and abs(one - -22.5768) <= 1e-3
    assert abs(album - a) > 1.0 and abs(album - b) > 1.0


def test_maximum_edge_cases():
    e = energies(2, 11, ns=4, nh=64)
    e[1, 0, 10] = np.nan    # poisons the blocks it enters, which the maximum skips
    e[2, 1, 20] = np.inf    # +inf is a value: the maximum
    e[3] = 0.0              # silence: +0.0
    for L, P in ((4, 1), (30, 10)):
        zs, nbs, top = S.blocks(e, 4800, L, P)
        b, nb, mx = blocks_host(e, 4800, L, P)
        assert np.array_equal(bits(mx), bits(top)) and np.array_equal(bits(b), bits(S.as_rows(zs, b.shape[1], GUARD)))
        assert np.isfinite(mx[1]) and mx[1] > 0 and np.isnan(b[1]).any() and mx[2] == np.inf and bits(mx[3:])[0] == 0
    neg = [-1.0, -1.0]      # weights may be anything: negative blocks never beat +0.0
    _, _, mx = blocks_host(e, 4800, 4, 1, weights=neg)
    assert np.array_equal(bits(mx[[0, 3]]), bits(np.zeros(2))) and np.array_equal(bits(mx), bits(S.blocks(e, 4800, 4, 1, weights=neg)[2]))
