"""GPU: speq_em_finalize and the histogram merges on an index of more than 1,024 tiles.

speq_em_finalize runs k_em_count, k_em_scan and k_em_compact over tiles of 4,096 SA positions; k_em_scan is one
workgroup of 1,024 threads that carries its running sum into a second trip from tile 1,024 on, i.e. for every index of
more than 4,194,304 positions (config 3 and up). The other EM tests stay below 45 tiles. Here n = 4,240,009 (1,036
tiles; tests/em_large_reference.py, whose inputs tests/test_em_large_reference_cpu.py checks without a GPU): 3,163
expected intervals start at or after position 1,024 x 4,096 and 289,201 before it, 9 tiles hold no interval (a
one-group interval spans them), and the last tile, 649 positions, holds 51.

Expected: every interval start, its multiplicity and its (group, count) entries, by numpy from the index's sa, text,
text_start and text_group arrays, independent of the FM search. Compared exactly with em.intervals(), em.rows_csr()
and em.info(), unmerged (SPEQ_EM_MERGE_ROWS=0) and merged; then the same histogram recorded by two replicas and
folded (k_em_merge over 4.2 M positions), and passed through speq_em_allreduce on a one-member communicator.

Not reached here: k_em_merge's second grid-stride trip (n > 16,777,216)."""
import numpy as np
import pytest

import em_large_reference as elr
from speq_amd import Comm, DeviceIndex, EmHistogram, Node

pytestmark = pytest.mark.gpu
K = elr.LARGE_K


@pytest.fixture(scope="module")
def world():
    _, idx, reads, exp = elr.large_inputs()
    c = exp.conditions()
    assert c["tiles"] > elr.SCAN_TILES and c["beyond_first_trip"] > 0 and c["within_first_trip"] > 0
    assert c["empty_tiles"] > 0 and c["in_last_partial_tile"] > 0
    dev = DeviceIndex(idx)
    yield {"idx": idx, "reads": reads, "exp": exp, "dev": dev}
    dev.close()


def scan(em, reads, a=0, b=None):
    b = reads.n if b is None else b
    lo, hi = int(reads.offsets[a]), int(reads.offsets[b])
    return em.scan(reads.seq[lo:hi].tobytes(), reads.qual[lo:hi].tobytes(), reads.offsets[a:b + 1] - reads.offsets[a],
                   k=K)


def histogram_equals_expected(em, exp, merged):
    em.finalize()
    assert em.info() == exp.info
    lo, row = em.intervals()
    assert np.array_equal(lo.astype(np.int64), exp.lo), "the set of interval starts"
    mult, ptr, grp, cnt = em.rows_csr()
    ptr = ptr.astype(np.int64)
    n_rows, row = len(mult), row.astype(np.int64)
    used = np.bincount(row, minlength=n_rows)
    assert len(used) == n_rows and (used > 0).all()
    # every interval's row holds the interval's entries
    exp_len = np.diff(exp.ptr)
    assert np.array_equal((ptr[1:] - ptr[:-1])[row], exp_len)
    at = np.repeat(ptr[:-1][row] - exp.ptr[:-1], exp_len) + np.arange(exp.ptr[-1])
    assert np.array_equal(grp[at].astype(np.int64), exp.grp) and np.array_equal(cnt[at].astype(np.int64), exp.cnt)
    # ... and a row's multiplicity is the sum over its intervals
    total = np.zeros(n_rows, dtype=np.int64)
    np.add.at(total, row, exp.mult)
    assert np.array_equal(mult.astype(np.int64), total)
    contents = {(tuple(grp[a:b].tolist()), tuple(cnt[a:b].tolist())) for a, b in zip(ptr[:-1].tolist(), ptr[1:].tolist())}
    if merged:
        assert len(contents) == n_rows < len(exp.lo), "equal rows left unmerged"
    else:
        assert n_rows == len(exp.lo) and (used == 1).all(), "one row per interval"


def counters_equal_expected(results, exp):
    assert sum(r.total for r in results) == exp.total
    assert sum(r.unique.astype(np.int64) for r in results).tolist() == exp.unique.tolist()


@pytest.mark.parametrize("merge_rows", ["0", None], ids=["unmerged", "merged"])
def test_finalize_past_1024_tiles(world, monkeypatch, merge_rows):
    if merge_rows is None:
        monkeypatch.delenv("SPEQ_EM_MERGE_ROWS", raising=False)
    else:
        monkeypatch.setenv("SPEQ_EM_MERGE_ROWS", merge_rows)
    em = EmHistogram(world["dev"])
    try:
        counters_equal_expected([scan(em, world["reads"])], world["exp"])
        assert world["dev"].tuning("last_kernel") == 3
        histogram_equals_expected(em, world["exp"], merged=merge_rows is None)
    finally:
        em.close()


def test_two_replicas_folded_with_merge_em(world, monkeypatch):
    monkeypatch.delenv("SPEQ_EM_MERGE_ROWS", raising=False)
    reads, half = world["reads"], world["reads"].n // 2
    other = DeviceIndex(world["idx"])
    ems = [EmHistogram(world["dev"]), EmHistogram(other)]
    try:
        counters_equal_expected([scan(ems[0], reads, 0, half), scan(ems[1], reads, half, reads.n)], world["exp"])
        histogram_equals_expected(Node.merge_em(ems), world["exp"], merged=True)
    finally:
        for em in ems:
            em.close()
        other.close()


def test_allreduce_on_a_one_member_communicator(world, monkeypatch):
    monkeypatch.setenv("SPEQ_EM_MERGE_ROWS", "0")
    em = EmHistogram(world["dev"])
    comm = Comm(1, 0, Comm.unique_id())
    try:
        counters_equal_expected([scan(em, world["reads"])], world["exp"])
        em.allreduce(comm)
        histogram_equals_expected(em, world["exp"], merged=False)
    finally:
        comm.close()
        em.close()
