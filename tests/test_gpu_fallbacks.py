"""Every path the library takes because device memory is short or an index is large, against the C hash oracle.

The decisions are host arithmetic (speq_amd/csrc/build_limits.hpp; tests/test_build_limits_cpu.py checks it without a
GPU). Here two test switches of dev_mem.cpp make them come out the other way on a small index, and each resulting state
is scanned: speq_debug_free_bytes makes the nth free-memory query answer at most a given figure (the library believes
memory is short: none is taken), speq_debug_offset_limit stands for 2^32 in the offset decisions of the host (a
structure is left out as it would be beyond 2^32: the kernels address what is left exactly as before). The state is
read through speq_device_build_facts, the kernel through "last_kernel" (3 anchor-and-extend, 2 / 1 the k-mer-table
kernels, 0 LF steps).

Every state's scan is compared with the oracle (oracle/kmer_oracle.c), never with another run of the library: T,
ambiguous units and U[g] exactly, W[g] within (3 k + 2 U[g] + 2) 2^-53 W_ref; EM rows and info() with the exact
histogram of tests/em_reference.py. Every switch is reset in a `finally`, and once a replica is closed as many
allocations are alive as before it was opened.

Reference and reads: those of tests/test_gpu_alloc_failures.py (96 k text positions, 4 groups, 2,000 reads of 100
bases, also taken as 1,000 pairs), k = 21 and 70; for k = 130, where a read of 100 bases has no window, 400 reads of
250 bases of the same reference. EM: the `std` reference and `mixed` reads of tests/em_cases.py."""
import numpy as np
import pytest

import em_cases as ec
import em_reference as er
import variant_table as vt
from oracle.oracle import Oracle
from speq_amd import DeviceIndex, EmHistogram, FmIndex, synth
from speq_amd.api import debug_allocs, debug_free_bytes, debug_free_queries, debug_offset_limit

pytestmark = pytest.mark.gpu

G = 4
KS = (21, 70)
MODES = [(False, False), (True, False), (False, True), (True, True)]  # (paired, local)
MODE_IDS = ["single-global", "paired-global", "single-local", "paired-local"]
U53 = 2.0 ** -53
BUILT, DEFERRED, REFUSED = 1, 2, 3   # build_facts()["ax"]
KT_NONE = 3                          # build_facts()["ktab"]: no table, kept for the replica's life


class Inputs:
    def __init__(self, ref, reads):
        self.seq, self.qual, self.off = reads.seq.tobytes(), reads.qual.tobytes(), reads.offsets
        self.reads = reads
        self.ref = ref
        self.expected = {}

    def oracle(self, k, paired, local):
        key = (k, paired, local)
        if key not in self.expected:
            orc = Oracle(self.ref.records, self.ref.groups, G, k)
            T, amb, U, W = orc.scan(self.reads.seq, self.reads.qual, self.reads.offsets, paired=paired, local=local)
            assert T > 0 and int(U.sum()) > 0, key
            self.expected[key] = (int(T), int(amb), U, W)
        return self.expected[key]


@pytest.fixture(scope="module")
def world():
    ref = synth.make_reference(G, 2, 6_000, ref_n_rate=0.002)
    idx = FmIndex.build(ref.records, ref.groups, G, prefix_q=8, pair_steps=True, triple_steps=True)
    short = Inputs(ref, synth.make_reads(ref, 2_000, read_len=100, err_rate=0.003, n_rate=0.002, lowq_rate=0.01))
    long_ = Inputs(ref, synth.make_reads(ref, 400, read_len=250, err_rate=0.003, n_rate=0.002, lowq_rate=0.01))
    return {"ref": ref, "idx": idx, "short": short, "long": long_,
            "idx2": FmIndex.build(ref.records, ref.groups, G, prefix_q=8, pair_steps=True, triple_steps=False),
            "idx1": FmIndex.build(ref.records, ref.groups, G, prefix_q=8, pair_steps=False, triple_steps=False)}


class Replica:
    """A fresh replica; on exit the switches are reset, it is closed, and its allocations must be gone."""

    def __init__(self, idx, limit_at_open=0, **tune):
        self.idx, self.tune, self.limit_at_open = idx, tune, limit_at_open

    def __enter__(self):
        self.live0 = debug_allocs()[0]
        debug_offset_limit(self.limit_at_open)
        try:
            self.dev = DeviceIndex(self.idx)
        finally:
            debug_offset_limit(0)
        self.dev.tune(**self.tune)
        return self.dev

    def __exit__(self, *exc):
        debug_free_bytes(0)
        debug_offset_limit(0)
        self.dev.close()
        assert debug_allocs()[0] == self.live0, "device allocations alive after the replica was closed"
        return False


def scan_equals_oracle(dev, inp, k, paired, local, tag=""):
    got = dev.scan(inp.seq, inp.qual, inp.off, k=k, paired=paired, local=local)
    T, amb, U, W = inp.oracle(k, paired, local)
    assert (got.total, got.ambiguous, got.unique.tolist()) == (T, amb, U.tolist()), (tag, k, paired, local)
    if local:
        tol = (3 * k + 2 * U.astype(np.float64) + 2) * U53 * W
        assert (np.abs(got.weights - W) <= tol).all(), (tag, k, paired, got.weights, W)
    else:
        assert got.weights is None
    return got


def all_modes_equal_oracle(dev, inp, k, tag=""):
    return [scan_equals_oracle(dev, inp, k, p, l, tag) for p, l in MODES]


def armed(nth, nbytes=0):
    debug_free_bytes(nth, nbytes)


# ---------------------------------------------------------------------------------------------------------------
# every free-memory query answers 0 once
# ---------------------------------------------------------------------------------------------------------------
# build_ax asks three times, in this order: before anything is allocated (short: the build is deferred), before the
# suffix sort (short: first claimants represent the k-mers), before the table and the filter (short: deferred, with the
# 2-bit text already the replica's)
AX_QUERIES = {1: "deferred", 2: "no-sort", 3: "deferred"}


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("k", KS)
def test_every_query_of_a_first_scan_answers_zero_once(world, k, mode):
    inp = world["short"]
    paired, local = mode
    with Replica(world["idx"]) as dev:
        q0 = debug_free_queries()
        scan_equals_oracle(dev, inp, k, paired, local, "clean")
        N = debug_free_queries() - q0
        f = dev.build_facts(k)
        assert (f["ax"], f["sa_reps"], dev.tuning("last_kernel")) == (BUILT, 1, 3)
    assert N == len(AX_QUERIES), N
    for n in range(1, N + 1):
        with Replica(world["idx"]) as dev:
            try:
                armed(n)
                scan_equals_oracle(dev, inp, k, paired, local, f"query {n}")
            finally:
                armed(0)
            f = dev.build_facts(k)
            if AX_QUERIES[n] == "no-sort":
                assert (f["ax"], f["sa_reps"]) == (BUILT, 0), (n, f)
                assert dev.tuning("last_kernel") == 3
            else:
                assert f["ax"] == DEFERRED, (n, f)
                assert dev.tuning("last_kernel") == (2 if k == 21 else 0)  # the compact k-mer table; k > 31: LF steps
            # the same replica, nothing armed: a deferred build is tried again and the anchor kernel takes the scan
            scan_equals_oracle(dev, inp, k, paired, local, f"after query {n}")
            f = dev.build_facts(k)
            assert f["ax"] == BUILT and dev.tuning("last_kernel") == 3, (n, f)
            assert f["sa_reps"] == (0 if AX_QUERIES[n] == "no-sort" else 1)
            all_modes_equal_oracle(dev, inp, k, f"after query {n}")


def em_case():
    return ec.Case(ec.Inputs("std", "mixed"), 21, False)


@pytest.fixture(scope="module")
def em_world():
    case = em_case()
    rs = ec.ref("std")
    idx = FmIndex.build(rs.records, rs.groups, rs.G, prefix_q=8, pair_steps=True, triple_steps=True)
    return {"case": case, "rs": rs, "rd": ec.reads(case.inp), "h": ec.histogram(case.inp, case.k), "idx": idx}


def em_scan(em, rd, k, a=0, b=None):
    b = rd.n if b is None else b
    lo, hi = int(rd.offsets[a]), int(rd.offsets[b])
    return em.scan(rd.seq[lo:hi].tobytes(), rd.qual[lo:hi].tobytes(), rd.offsets[a:b + 1] - rd.offsets[a], k=k,
                   phred_cutoff=ec.CUTOFF)


def histogram_equals_reference(em, ew, unique):
    case, rs, h = ew["case"], ew["rs"], ew["h"]
    em.finalize()
    assert em.info() == (h.n_intervals, h.n_entries, h.n_windows)
    rows = em.rows()
    assert len({content for _, content in rows}) == len(rows), "equal rows left unmerged"
    assert {content: m for m, content in rows} == h.merged
    bound = (h.n_intervals + 2 * rs.G + 80) * U53  # one rounding per row added (tests/test_gpu_em_rows.py)
    for which, percent in ec.percents(rs.G).items():
        got = em.step(percent, rs.counts, unique)
        np.testing.assert_allclose(got, ec.oracle_em_pass(case.inp, case.k, False, which), rtol=1e-9, atol=0)
        assert er.max_relative_deviation(got, ec.exact_step(case.inp, case.k, which)) <= bound, which


def em_counters_equal_oracle(r, ew):
    T, amb, Uo, _ = ec.oracle_scan(ew["case"].inp, ew["case"].k, False)
    assert (r.total, r.ambiguous, r.unique.tolist()) == (T, amb, Uo.tolist())


def test_every_query_of_a_first_em_scan_answers_zero_once(em_world):
    ew = em_world
    rd, k = ew["rd"], ew["case"].k
    with Replica(ew["idx"]) as dev:
        q0 = debug_free_queries()
        em = EmHistogram(dev)
        try:
            r = em_scan(em, rd, k)
            N = debug_free_queries() - q0
            em_counters_equal_oracle(r, ew)
            assert dev.tuning("last_kernel") == 3 and dev.build_facts(k)["em_arrays"] == 1
            histogram_equals_reference(em, ew, r.unique)
        finally:
            em.close()
    assert N == len(AX_QUERIES) + 1, N  # ensure_ax_em asks once
    for n in range(1, N + 1):
        with Replica(ew["idx"]) as dev:
            em = EmHistogram(dev)
            try:
                try:
                    armed(n)
                    r = em_scan(em, rd, k)
                finally:
                    armed(0)
                em_counters_equal_oracle(r, ew)
                f = dev.build_facts(k)
                if n == 2:
                    assert (f["ax"], f["sa_reps"], f["em_arrays"], dev.tuning("last_kernel")) == (BUILT, 0, 1, 3)
                elif n == N:  # the EM arrays do not fit: the table is there, the EM scan goes to the k-mer table
                    assert (f["ax"], f["em_arrays"]) == (BUILT, 0) and dev.tuning("last_kernel") in (1, 2), f
                else:
                    assert f["ax"] == DEFERRED and dev.tuning("last_kernel") in (1, 2), (n, f)
                histogram_equals_reference(em, ew, r.unique)
            finally:
                em.close()
            em = EmHistogram(dev)  # the same replica, nothing armed
            try:
                r = em_scan(em, rd, k)
                em_counters_equal_oracle(r, ew)
                f = dev.build_facts(k)
                assert (f["ax"], f["em_arrays"], dev.tuning("last_kernel")) == (BUILT, 1, 3), (n, f)
                histogram_equals_reference(em, ew, r.unique)
            finally:
                em.close()


def test_one_histogram_filled_by_two_kernels(em_world):
    """The EM arrays do not fit for the first piece of a read set and do for the second: the histogram is the whole
    set's, and a plain scan in between stays on the anchor kernel."""
    ew = em_world
    rd, k = ew["rd"], ew["case"].k
    cut = rd.n // 2
    with Replica(ew["idx"]) as dev:
        dev.prepare(k)  # build_ax's three queries are made: the next one is ensure_ax_em's
        assert dev.build_facts(k)["ax"] == BUILT
        em = EmHistogram(dev)
        try:
            try:
                armed(1)
                r1 = em_scan(em, rd, k, 0, cut)
            finally:
                armed(0)
            assert dev.tuning("last_kernel") != 3 and dev.build_facts(k)["em_arrays"] == 0
            plain = dev.scan(rd.seq.tobytes(), rd.qual.tobytes(), rd.offsets, k=k, phred_cutoff=ec.CUTOFF)
            assert dev.tuning("last_kernel") == 3
            em_counters_equal_oracle(plain, ew)
            r2 = em_scan(em, rd, k, cut, rd.n)
            assert dev.tuning("last_kernel") == 3 and dev.build_facts(k)["em_arrays"] == 1
            T, amb, Uo, _ = ec.oracle_scan(ew["case"].inp, k, False)
            assert (r1.total + r2.total, r1.ambiguous + r2.ambiguous, (r1.unique + r2.unique).tolist()) == \
                (T, amb, Uo.tolist())
            histogram_equals_reference(em, ew, r1.unique + r2.unique)
        finally:
            em.close()


# ---------------------------------------------------------------------------------------------------------------
# build_ktab
# ---------------------------------------------------------------------------------------------------------------
def smallest_free_for(x):
    """The smallest answer whose usable nine tenths (free // 10 * 9) reach x."""
    return (x + 8) // 9 * 10


def test_a_k_mer_table_that_does_not_fit_is_never_tried_again(world):
    """build_ktab asks once; short: no table, LF steps. Unlike build_ax's deferred build the null table is kept for the
    replica's life: the second scan, with nothing armed, still runs on LF steps."""
    inp, k = world["short"], 21
    with Replica(world["idx"], ax_scan=0) as dev:
        q0 = debug_free_queries()
        all_modes_equal_oracle(dev, inp, k, "clean")
        assert debug_free_queries() - q0 == 1
        assert dev.build_facts(k)["ktab"] == 2 and dev.tuning("last_kernel") == 2  # compact, pipelined
    with Replica(world["idx"], ax_scan=0) as dev:
        try:
            armed(1)
            scan_equals_oracle(dev, inp, k, False, False, "armed")
        finally:
            armed(0)
        assert dev.build_facts(k)["ktab"] == KT_NONE and dev.tuning("last_kernel") == 0
        q0 = debug_free_queries()
        all_modes_equal_oracle(dev, inp, k, "after")
        assert dev.build_facts(k)["ktab"] == KT_NONE and dev.tuning("last_kernel") == 0
        assert debug_free_queries() == q0, "the null table is cached: nothing is asked again"


def test_the_compact_table_has_a_check_of_its_own():
    """An answer that passes build_ktab's first check (key set + wide table) and fails its second (key set + compact
    table, scratch array and its exact copy), restated here. It needs a reference whose windows are nearly all distinct
    k-mers (the synthetic variants share most of theirs): four unrelated random records; and at kt_load8 = 10 a compact
    table takes 96 B per distinct k-mer. One more usable byte and the table is built."""
    k, load8, kt_slots = 21, 10, 2
    rng = np.random.default_rng(41)
    records = [bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=6_000)) for _ in range(G)]
    ref = synth.Reference(records, list(range(G)), G, 1, 6_000)
    idx = FmIndex.build(ref.records, ref.groups, G, prefix_q=8, pair_steps=True, triple_steps=True)
    inp = Inputs(ref, synth.make_reads(ref, 1_000, read_len=100, err_rate=0.003, n_rate=0.002, lowq_rate=0.01))
    ts = idx.array("text_start", np.uint64).astype(np.int64)
    total = int(np.maximum(ts[1:] - ts[:-1] - 1 - k + 1, 0).sum())
    # the distinct N-free k-mers of the texts, counted here: the edge is placed without asking the library
    text = idx.array("text", np.uint8)
    acgt = (text >= 2) & (text <= 5)  # text codes: # $ A C G T N = 0..6
    bad = np.concatenate([[0], np.cumsum(~acgt)])
    starts = np.flatnonzero(bad[k:] == bad[:-k])
    kmers = np.zeros(len(starts), dtype=np.uint64)
    for j in range(k):
        kmers = (kmers << np.uint64(2)) | (text[starts + j] - 2).astype(np.uint64)
    distinct = len(np.unique(kmers))
    assert len(starts) == total
    with Replica(idx, ax_scan=0) as dev:
        assert dev.prepare(k)["distinct_kmers"] == distinct

    def pow2(x):
        return 1 << max(0, (x - 1).bit_length())

    keys = pow2(max(2 * total, 64)) * 8 + len(ts) * 8 + 16
    need1 = keys + pow2(max(1, (total * kt_slots + 3) // 4)) * 64
    nb8 = max(1, int(distinct * 100.0 / (8.0 * load8)) + 1)
    need2 = keys + nb8 * 64 + 2 * max(distinct, 1) * 8 + 16
    print(f"total {total} distinct {distinct}: first check {need1} B, compact check {need2} B")
    assert need2 > need1, "vacuous: the compact check cannot fire alone on this reference"
    for free, ktab, kernel in ((smallest_free_for(need2) - 1, KT_NONE, 0), (smallest_free_for(need2), 2, 2)):
        assert free // 10 * 9 >= need1
        with Replica(idx, ax_scan=0, kt_load8=load8, kt_slots=kt_slots) as dev:
            try:
                armed(1, free)
                scan_equals_oracle(dev, inp, k, False, False, f"free {free}")
            finally:
                armed(0)
            assert (dev.build_facts(k)["ktab"], dev.tuning("last_kernel")) == (ktab, kernel), free
            all_modes_equal_oracle(dev, inp, k, f"free {free}")


# ---------------------------------------------------------------------------------------------------------------
# 32-bit buffer offsets
# ---------------------------------------------------------------------------------------------------------------
def test_offset_limit_drops_the_bitmap_the_filter_then_the_table(world):
    """build_ax's four inequalities (ax_scan.hip, restated): with `beyond(x) = x >= limit - 64`,
      the m-mer filter is dropped when beyond(nb 64 + nmf 8 + 16),
      the table is refused when beyond(nb 64) or beyond(nf 8)   (nf 8 is a quarter of nb 64 at most: one edge),
      the bitmap is dropped when beyond(s_off + s_words 8 + 16).
    So the smallest limit that keeps a structure is its end + 65."""
    inp = world["short"]
    free = {}
    for k in KS:
        with Replica(world["idx"]) as dev:
            dev.prepare(k)
            free[k] = dev.build_facts(k)
            all_modes_equal_oracle(dev, inp, k, "unlimited")
            sp = vt.unpack(dev.tuning("last_variant")).sproof
            assert (free[k]["ax"], sp, free[k]["m"] != 0) == (BUILT, k == 21, k == 70)  # production: one or the other
    seen = set()
    for k in KS:
        f0 = free[k]
        assert f0["nf"] * 8 < f0["nb"] * 64
        ends = {"table": f0["nb"] * 64, "bitmap": f0["s_off"] + f0["s_words"] * 8 + 16}
        if f0["m"]:
            ends["filter"] = f0["nb"] * 64 + f0["nmf"] * 8 + 16
        for what, end in ends.items():
            for limit, kept in ((end + 65, True), (end + 64, False)):
                with Replica(world["idx"]) as dev:  # (opened before the limit: the planes are not the subject)
                    try:
                        debug_offset_limit(limit)
                        got = scan_equals_oracle(dev, inp, k, False, False, f"{what} {limit}")
                    finally:
                        debug_offset_limit(0)
                    f = dev.build_facts(k)
                    kernel, variant = dev.tuning("last_kernel"), vt.unpack(dev.tuning("last_variant"))
                    tag = (k, what, limit, f)
                    if what == "table":
                        assert f["ax"] == (BUILT if kept else REFUSED), tag
                        assert (kernel == 3) == kept, tag
                        if kept:  # nothing but the buckets
                            assert (f["nb"], f["m"], f["s_words"]) == (f0["nb"], 0, 0), tag
                    elif what == "filter":
                        assert (f["ax"], f["nb"], kernel) == (BUILT, f0["nb"], 3), tag
                        assert (f["m"], f["nmf"]) == ((f0["m"], f0["nmf"]) if kept else (0, 0)), tag
                    else:
                        assert (f["ax"], f["nb"], f["m"], f["nmf"], kernel) == (BUILT, f0["nb"], f0["m"], f0["nmf"], 3), tag
                        assert f["s_words"] == (f0["s_words"] if kept else 0), tag
                        assert variant.sproof == (kept and k == 21), tag
                    if f["ax"] == REFUSED:
                        seen.add("refused")
                        # the limit is back at 2^32: a refusal is structural, the same replica does not try again
                        all_modes_equal_oracle(dev, inp, k, "refused, limit restored")
                        assert dev.build_facts(k)["ax"] == REFUSED and dev.tuning("last_kernel") != 3, tag
                        # build_ktab reads the same limit for its slot and bucket counts (262,144 slots here, far
                        # below it): the scan fell back to the compact table it built under the limit; k > 31 has none
                        assert dev.build_facts(k)["ktab"] == (2 if k == 21 else 0), tag
                        assert dev.tuning("last_kernel") == (2 if k == 21 else 0), tag
                    else:
                        if k == 21 and f["s_words"] == 0 and f["nb"] == f0["nb"] and what == "bitmap":
                            seen.add("bitmap dropped only")
                        if k == 70 and f["m"] == 0 and f0["m"] != 0:
                            seen.add("filter dropped")
                        all_modes_equal_oracle(dev, inp, k, str(tag))
                        assert dev.tuning("last_kernel") == 3 and dev.build_facts(k) == f, tag
                    assert got.total > 0
    assert seen == {"bitmap dropped only", "filter dropped", "refused"}, seen
    for k in KS:  # a fresh replica builds what the other refused
        with Replica(world["idx"]) as dev:
            scan_equals_oracle(dev, inp, k, False, False)
            assert dev.build_facts(k) == dict(free[k], em_arrays=0)


PLANES = {7: "idx", 3: "idx2", 1: "idx1"}  # published families -> the index built with exactly those


@pytest.mark.parametrize("published", [7, 3, 1], ids=["all", "no-occ3", "no-occ3-no-occ2"])
def test_plane_families_beyond_the_limit_are_not_published(world, published):
    """speq_device_open publishes a plane family only when 32-bit offsets reach all of it (planes nb 16 <= limit - 16):
    the searches of the scans, of the structure builds and of the reference pass then step by fewer symbols. Results are
    the oracle's, and bit for bit those of an index built without the planes."""
    nb = int(world["idx"].info().n) // 96 + 1
    limit = {7: 64 * nb * 16 + 16, 3: 64 * nb * 16 + 15, 1: 16 * nb * 16 + 15}[published]
    orc_ref = {k: Oracle(world["ref"].records, world["ref"].groups, G, k).ref_unique() for k in (21,)}
    results = {}
    for which, idx, lim in (("limited", world["idx"], limit), ("built without", world[PLANES[published]], 0)):
        out = []
        for tune in ({}, dict(ax_scan=0, kmer_table=0), dict(ax_scan=0)):
            with Replica(idx, limit_at_open=lim, **tune) as dev:
                assert dev.build_facts(21)["planes"] == published, (which, dev.build_facts(21))
                for k, inp in ((21, world["short"]), (130, world["long"])):
                    got = all_modes_equal_oracle(dev, inp, k, f"{which} {tune}")
                    expect = 0 if (k == 130 or "kmer_table" in tune) else 2 if tune else 3
                    assert dev.tuning("last_kernel") == expect, (which, tune, k)
                    out += [(g.total, g.ambiguous, g.unique.tolist()) for g in got]  # (W is summed in any order)
                u, t = dev.count_unique_kmers_per_group(21)
                assert (u.tolist(), t.tolist()) == (orc_ref[21][0].tolist(), orc_ref[21][1].tolist())
                out.append((u.tolist(), t.tolist()))
        results[which] = out
    assert results["limited"] == results["built without"]
