"""Every device allocation of an operation fails once, and the replica, its handles and device memory survive it.

The library's device allocations all go through one function (speq_amd/csrc/dev_mem.cpp), which counts them and can
make the nth from now throw OutOfDeviceMemory before the device is asked (speq_debug_fail_alloc: a host exception, no
device memory is exhausted). Each case runs its operation once on a fresh replica to count the allocations N it makes
(1 <= N <= 64), then for every n in 1 .. N arms the nth allocation on another fresh replica and runs it again:

* it raises (at least one n must): the status is the one its entry point returns for a failed allocation (SPEQ_E_NOMEM
  from the marker, bootstrap and dedup entry points, SPEQ_E_DEVICE from every other), and the same operation then
  succeeds on the same replica with the results of the clean run (which are the oracle's where the oracle has them);
* or it succeeds, where a failure is caught and worked around (the suffix sort inside build_ax): same results;
* either way, once the handles and the replica are closed, as many allocations are alive as before it was opened.

Reference: the small reference of tests/test_gpu_ax.py (96 k text positions, 4 groups), 2,000 reads of 100 bases."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from oracle.oracle import Oracle
from speq_amd import Bootstrap, Dedup, DeviceIndex, EmHistogram, FmIndex, Markers, synth
from speq_amd._lib import SPEQ_E_DEVICE, SPEQ_E_NOMEM, SpeqError, check, lib

pytestmark = pytest.mark.gpu

G = 4
KS = (21, 70)


def counters():
    live, made = C.c_uint64(), C.c_uint64()
    fn = lib().speq_debug_allocs
    fn.argtypes, fn.restype = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)], None
    fn(C.byref(live), C.byref(made))
    return live.value, made.value


def arm(nth):
    fn = lib().speq_debug_fail_alloc
    fn.argtypes, fn.restype = [C.c_int64], None
    fn(nth)


@pytest.fixture(scope="module")
def world():
    ref = synth.make_reference(G, 2, 6_000, ref_n_rate=0.002)
    idx = FmIndex.build(ref.records, ref.groups, G, prefix_q=8, pair_steps=True, triple_steps=True)
    reads = synth.make_reads(ref, 2_000, read_len=100, err_rate=0.003, n_rate=0.002, lowq_rate=0.01)
    w = {"ref": ref, "idx": idx, "seq": reads.seq.tobytes(), "qual": reads.qual.tobytes(), "off": reads.offsets,
         "n": len(reads.offsets) - 1, "reads": reads}
    for k in KS:
        orc = Oracle(ref.records, ref.groups, G, k)
        T, amb, U, _ = orc.scan(reads.seq, reads.qual, reads.offsets)
        u_ref, tot_ref = orc.ref_unique()
        w[k] = {"scan": (int(T), int(amb), [int(x) for x in U]),
                "ref": ([int(x) for x in u_ref], [int(x) for x in tot_ref])}
    return w


def same(a, b):
    if dataclasses.is_dataclass(a):
        return type(a) is type(b) and same(dataclasses.asdict(a), dataclasses.asdict(b))
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[x], b[x]) for x in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and np.array_equal(a, b)
    return a == b


def scan_of(dev, w, k):
    got = dev.scan(w["seq"], w["qual"], w["off"], k=k)
    return int(got.total), int(got.ambiguous), [int(x) for x in got.unique]


def every_allocation_fails_once(w, op, code, prep=None, oracle=None, opens=False):
    """op(dev, ctx) -> result, closing every handle it made, by an exception too; prep(dev) -> ctx with close(), made
    un-injected before the count starts. opens: the operation is the opening of the replica itself (op(None, None))."""
    live0, _ = counters()

    def fresh():
        if opens:
            return None, None
        dev = DeviceIndex(w["idx"])
        return dev, (prep(dev) if prep else None)

    def done(dev, ctx):
        if ctx is not None:
            ctx.close()
        if dev is not None:
            dev.close()
        assert counters()[0] == live0, "device allocations alive after the replica was closed"

    dev, ctx = fresh()
    made0 = counters()[1]
    clean = op(dev, ctx)
    N = counters()[1] - made0
    done(dev, ctx)
    print(f"{N} allocations in the clean run")
    assert 1 <= N <= 64, N
    if oracle is not None:
        assert oracle(clean), clean
    raised = []
    for n in range(1, N + 1):
        dev, ctx = fresh()
        arm(n)
        try:
            try:
                got = op(dev, ctx)
            except SpeqError as e:
                arm(0)
                assert e.code == code, (n, e)
                raised.append(n)
                got = op(dev, ctx)  # the same replica, un-injected
        finally:
            arm(0)
        assert same(got, clean), n
        done(dev, ctx)
    print(f"raised at n = {raised}")
    assert raised, "no allocation of the operation was reached"


def test_device_open(world):
    def op(_dev, _ctx):
        dev = DeviceIndex(world["idx"])  # (a failed open leaves no handle to close)
        try:
            return scan_of(dev, world, 21)
        finally:
            dev.close()

    every_allocation_fails_once(world, op, SPEQ_E_DEVICE, opens=True, oracle=lambda r: r == world[21]["scan"])


@pytest.mark.parametrize("k,tune", [(21, {}), (70, {}), (21, {"ax_scan": 0}), (21, {"ax_scan": 0, "kt_compact": 0})],
                         ids=["k21", "k70", "k21-compact-table", "k21-wide-table"])
def test_prepare(world, k, tune):
    def prep(dev):
        dev.tune(**tune)

    def op(dev, _ctx):
        info = dev.prepare(k)
        return info["distinct_kmers"], info["table_bytes"], scan_of(dev, world, k), dev.tuning("last_kernel")

    # "last_kernel": 3 the anchor kernel, 1 and 2 the two k-mer-table kernels
    kernels = (1, 2) if tune else (3,)
    every_allocation_fails_once(world, op, SPEQ_E_DEVICE, prep=prep,
                                oracle=lambda r: r[1] > 0 and r[2] == world[k]["scan"] and r[3] in kernels)


class Closing:
    def __init__(self, *handles):
        self.handles = handles

    def close(self):
        for h in self.handles:
            h.close()


def test_em_scan_and_finalize(world):
    """EM scan of k = 21 (the EM-only arrays of the per-k structures, ensure_ax_em), then speq_em_finalize."""
    def prep(dev):
        dev.prepare(21)

    def op(dev, _ctx):
        em = EmHistogram(dev)
        try:
            got = em.scan(world["seq"], world["qual"], world["off"], k=21)
            em.finalize()
            return (int(got.total), int(got.ambiguous), [int(x) for x in got.unique]), em.rows()
        finally:
            em.close()

    every_allocation_fails_once(world, op, SPEQ_E_DEVICE, prep=prep,
                                oracle=lambda r: r[0] == world[21]["scan"] and len(r[1]) > 0)


def test_em_merge_on_one_device(world):
    half = world["n"] // 2
    off = world["off"]
    cut = int(off[half])
    parts = [(world["seq"][:cut], world["qual"][:cut], off[:half + 1]),
             (world["seq"][cut:], world["qual"][cut:], off[half:] - off[half])]

    def prep(dev):
        dev.prepare(21)

    def op(dev, _ctx):
        ems = []
        try:
            for _ in parts:
                ems.append(EmHistogram(dev))
            for em, (s, q, o) in zip(ems, parts):
                em.scan(s, q, o, k=21)
            check(lib().speq_em_merge(ems[0]._h, ems[1]._h))
            ems[0].finalize()
            return ems[0].rows()
        finally:
            for em in ems:
                em.close()

    def whole(rows):  # the merged histogram is the histogram of all the reads
        dev = DeviceIndex(world["idx"])
        em = EmHistogram(dev)
        try:
            em.scan(world["seq"], world["qual"], world["off"], k=21)
            em.finalize()
            return sorted(em.rows()) == sorted(rows)
        finally:
            em.close()
            dev.close()

    every_allocation_fails_once(world, op, SPEQ_E_DEVICE, prep=prep, oracle=whole)


@pytest.mark.parametrize("k", KS)
def test_ref_unique(world, k):
    def op(dev, _ctx):
        u, t = dev.count_unique_kmers_per_group(k)
        return [int(x) for x in u], [int(x) for x in t]

    every_allocation_fails_once(world, op, SPEQ_E_DEVICE, oracle=lambda r: r == world[k]["ref"])


@pytest.mark.parametrize("k", KS)
def test_ref_unique_shard(world, k):
    def op(dev, _ctx):
        parts = [dev.count_unique_kmers_per_group_shard(k, s, 3) for s in range(3)]
        return [[int(sum(p[i][g] for p in parts)) for g in range(G)] for i in range(2)]

    every_allocation_fails_once(world, op, SPEQ_E_DEVICE, oracle=lambda r: (r[0], r[1]) == world[k]["ref"])


def test_stats_scan(world):
    import torch
    reads = world["reads"]
    d_seq, d_qual = torch.from_numpy(reads.seq).cuda(), torch.from_numpy(reads.qual).cuda()
    d_off = torch.from_numpy(reads.offsets.astype(np.int64)).cuda()

    def prep(dev):
        dev.prepare(21)

    def op(dev, _ctx):
        d_counts = torch.zeros(G + 2, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        st = dev.scan_device_stats(d_seq.data_ptr(), d_qual.data_ptr(), d_off.data_ptr(), world["n"], 21,
                                   d_counts.data_ptr())
        c = d_counts.cpu().tolist()
        return (c[0], c[1], c[2:]), st["waves"] > 0

    every_allocation_fails_once(world, op, SPEQ_E_DEVICE, prep=prep, oracle=lambda r: r == (world[21]["scan"], True))


@pytest.mark.parametrize("k", KS)
def test_markers(world, k):
    def op(dev, _ctx):
        m = Markers(dev, k)
        try:
            m.add(world["seq"], world["qual"], world["off"])
            return m.finalize(), m.list()
        finally:
            m.close()

    # (the depths add up to the scan's unique windows)
    every_allocation_fails_once(world, op, SPEQ_E_NOMEM,
                                oracle=lambda r: [int(x) for x in r[0].hits] == world[k]["scan"][2] and len(r[1][0]))


def test_bootstrap_with_em(world):
    def prep(dev):
        em = EmHistogram(dev)
        em.scan(world["seq"], world["qual"], world["off"], k=21)
        em.finalize()
        return Closing(em)

    def op(dev, ctx):
        b = Bootstrap(dev, 21, replicates=8, seed=3)
        try:
            b.attach_em(ctx.handles[0])
            b.add(world["seq"], world["qual"], world["off"])
            counts, _ = b.finalize()
            mult, missed = b.finalize_em()
            return counts, mult, missed
        finally:
            b.close()

    def row0(r):  # replicate 0 is the sample itself: the scan's counters, the histogram's multiplicities, none missed
        T, amb, U = world[21]["scan"]
        return [int(x) for x in r[0][0]] == [T, amb] + U and r[2] == 0 and int(r[1][0].sum()) > 0

    every_allocation_fails_once(world, op, SPEQ_E_NOMEM, prep=prep, oracle=row0)


@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
def test_dedup(world, paired):
    # every read twice: 2,000 duplicates among 4,000 units (paired: 1,000 among 2,000)
    seq, off = world["seq"] * 2, np.concatenate([world["off"], world["off"][1:] + world["off"][-1]])
    units = (len(off) - 1) // (2 if paired else 1)

    def op(dev, _ctx):
        h = Dedup(dev, paired=paired)
        try:
            h.add(seq, off)
            return h.finalize(), h.representatives(0, units)
        finally:
            h.close()

    def halves(r):
        rep = r[1]
        h = units // 2
        return r[0].units == units and r[0].distinct <= h and np.array_equal(rep[h:], rep[:h])

    every_allocation_fails_once(world, op, SPEQ_E_NOMEM, oracle=halves)


@pytest.mark.parametrize("k", KS)
def test_read_report(world, k):
    def op(dev, _ctx):
        return dev.report(world["seq"], world["qual"], world["off"], k=k)

    def totals(r):  # the report's windows add up to the scan's
        T, _amb, U = world[k]["scan"]
        return int(r.passing.sum()) == T and int(r.unique.sum()) == sum(U)

    every_allocation_fails_once(world, op, SPEQ_E_DEVICE, oracle=totals)
