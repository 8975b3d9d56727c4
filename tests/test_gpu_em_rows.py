"""GPU: the EM histogram, row by row, against the exact pure-Python reference (tests/em_reference.py).

`speq scan` always allocates an EM histogram, so the kernels a user runs are the EM = true instantiations; they record
every multi-group window from sites of their own (k_scan_ax: the run loop and the deferred-window pass, both through
the EM-only mlo / mhi arrays; the table kernel and the LF kernel have one each), and em_build_rows /
merge_equal_rows turn the device arrays into the CSR rows every EM step reads. The histogram is integers, so it is
pinned exactly: which rows, which (group, count) entries, which multiplicities (EmHistogram.rows()), unmerged
(SPEQ_EM_MERGE_ROWS=0) and merged; em.info(); the scan counters against the oracle; and em.step against the oracle's
literal fp64 pass (rtol 1e-9) and against the exact rational step within (n_intervals + 2 G + 80) * 2^-53 relative
(one rounding per row added, speq_em_step's 64 chunk partial sums, a few constant roundings per term).

The inputs (tests/em_cases.py; validated without a GPU by tests/test_em_reference_cpu.py) aim at each recording site:
error-free reads and reads of several chunks / segments (run loop), error-heavy and random reads (deferred windows),
chimeric reads and reads over a reference N (windows after a stop are not recorded, windows before it are), poly-A /
tandem-repeat / reverse-palindromic k-mers (occurrence counts above 1), G = 1, 2, 300, one read 5,000 times
(contention), tiny grids, several scan calls into one histogram, the device-buffer entry point, the hash-collision
fallback of the row merge (SPEQ_EM_MERGE_ROWS=2) and the IEEE branch of speq_em_step."""
import ctypes as C
from collections import Counter
from functools import lru_cache

import numpy as np
import pytest

import em_cases as ec
import em_reference as er
from speq_amd import DeviceIndex, EmHistogram, FmIndex
from speq_amd._lib import SPEQ_MODE_GLOBAL, SPEQ_MODE_LOCAL, ScanParams, check, lib

pytestmark = pytest.mark.gpu
RTOL = 1e-9       # em.step against the oracle's literal pass (the project's bound, tests/test_gpu_em.py)
U = 2.0 ** -53


@lru_cache(maxsize=None)
def fm_index(ref_name: str) -> FmIndex:
    rs = ec.ref(ref_name)
    return FmIndex.build(rs.records, rs.groups, rs.G, prefix_q=8, pair_steps=True, triple_steps=True,
                         label_table=ref_name != "g2")  # (g2: the rows walk the run bitvector's rank path)


def device(case: ec.Case) -> DeviceIndex:
    dev = DeviceIndex(fm_index(case.inp.ref))
    dev.tune(**ec.TUNE[case.kernel], **dict(case.tune))
    return dev


def scan_into(em: EmHistogram, rd, k, paired, local, pieces=1):
    """em.scan in `pieces` calls (cut at unit boundaries); returns (T, ambiguous, U, W) summed over the calls."""
    unit = 2 if paired else 1
    cuts = [rd.n // unit * i // pieces * unit for i in range(pieces + 1)]
    T = amb = 0
    Us = np.zeros(em.n_groups, dtype=np.uint64)
    W = np.zeros(em.n_groups) if local else None
    for a, b in zip(cuts, cuts[1:]):
        lo, hi = int(rd.offsets[a]), int(rd.offsets[b])
        r = em.scan(rd.seq[lo:hi].tobytes(), rd.qual[lo:hi].tobytes(), rd.offsets[a:b + 1] - rd.offsets[a], k=k,
                    phred_cutoff=ec.CUTOFF, paired=paired, local=local)
        T, amb, Us = T + r.total, amb + r.ambiguous, Us + r.unique
        if local:
            W += r.weights
    return T, amb, Us, W


def check_counters(got, inp, k, local):
    T, amb, Uo, Wo = ec.oracle_scan(inp, k, local)
    assert (got[0], got[1], got[2].tolist()) == (T, amb, Uo.tolist())
    if local:
        np.testing.assert_allclose(got[3], Wo, rtol=1e-10, atol=0)


def check_rows_unmerged(em: EmHistogram, h: er.Histogram):
    rows = em.rows()
    for _, content in rows:
        assert [g for g, _ in content] == sorted({g for g, _ in content}), "groups ascending, each once"
        assert len(content) >= 2, "a k-mer of one group is a U[g] window, however often that group holds it"
    assert Counter((content, m) for m, content in rows) == h.unmerged


def check_rows_merged(em: EmHistogram, h: er.Histogram):
    rows = em.rows()
    assert len({content for _, content in rows}) == len(rows), "equal rows left unmerged"
    assert {content: m for m, content in rows} == h.merged


def check_steps(em: EmHistogram, case: ec.Case, unique):
    rs, h = ec.ref(case.inp.ref), ec.histogram(case.inp, case.k)
    bound = (h.n_intervals + 2 * rs.G + 80) * U
    for which, percent in ec.percents(rs.G).items():
        got = em.step(percent, rs.counts, unique)
        exp = ec.oracle_em_pass(case.inp, case.k, case.local, which)
        np.testing.assert_allclose(got, exp, rtol=RTOL, atol=0, err_msg=which)
        dev = er.max_relative_deviation(got, ec.exact_step(case.inp, case.k, which))
        print(f"{case.id} {which}: deviation from the exact step {dev:.3e}, bound {bound:.3e}")
        assert dev <= bound, (which, dev, bound)


@pytest.mark.parametrize("case", ec.CASES, ids=[c.id for c in ec.CASES])
def test_rows_equal_the_exact_reference(case, monkeypatch):
    inp, k = case.inp, case.k
    rs, rd, h = ec.ref(inp.ref), ec.reads(inp), ec.histogram(inp, k)
    dev = device(case)
    # one row per interval
    monkeypatch.setenv("SPEQ_EM_MERGE_ROWS", "0")
    em = EmHistogram(dev)
    check_counters(scan_into(em, rd, k, inp.paired, case.local), inp, k, case.local)
    assert dev.tuning("last_kernel") in ec.KERNEL_CODES[case.kernel]
    em.finalize()
    assert em.info() == (h.n_intervals, h.n_entries, h.n_windows)
    check_rows_unmerged(em, h)
    em.close()
    # merged (the default)
    monkeypatch.delenv("SPEQ_EM_MERGE_ROWS")
    em = EmHistogram(dev)
    got = scan_into(em, rd, k, inp.paired, case.local)
    check_counters(got, inp, k, case.local)
    em.finalize()
    assert em.info() == (h.n_intervals, h.n_entries, h.n_windows)
    check_rows_merged(em, h)
    check_steps(em, case, got[2])
    if rs.G == 1:  # nothing is shared between groups: the histogram is empty and a step returns the unique windows
        assert em.info() == (0, 0, 0) and em.rows() == []
        np.testing.assert_array_equal(em.step([25.0], rs.counts, got[2]), got[2].astype(np.float64))
        np.testing.assert_array_equal(em.step([0.0], rs.counts, got[2]), [0.0])
    em.close()
    dev.close()


@pytest.mark.parametrize("pieces", [1, 2, 7])
def test_several_scan_calls_fill_one_histogram(pieces):
    case = ec.Case(ec.Inputs("std", "mixed", 150, True), 31, True)
    rd, h = ec.reads(case.inp), ec.histogram(case.inp, case.k)
    dev = device(case)
    em = EmHistogram(dev)
    T, amb, Us, W = scan_into(em, rd, case.k, True, True, pieces=pieces)
    To, ambo, Uo, Wo = ec.oracle_scan(case.inp, case.k, True)
    assert (T, amb, Us.tolist()) == (To, ambo, Uo.tolist())
    np.testing.assert_allclose(W, Wo, rtol=1e-10, atol=0)
    em.finalize()
    assert em.info() == (h.n_intervals, h.n_entries, h.n_windows)
    check_rows_merged(em, h)
    check_steps(em, case, Us)


def test_device_buffer_entry_point():
    """speq_em_scan_reads_device: reads, counters and weights in HBM."""
    import torch
    case = ec.Case(ec.Inputs("std", "mixed"), 21, True)
    rs, rd, h = ec.ref("std"), ec.reads(case.inp), ec.histogram(case.inp, case.k)
    dev = device(case)
    em = EmHistogram(dev)
    d_seq = torch.from_numpy(rd.seq.copy()).cuda()
    d_qual = torch.from_numpy(rd.qual.copy()).cuda()
    d_off = torch.from_numpy(rd.offsets.astype(np.int64)).cuda()
    cnt = torch.zeros(rs.G + 2, dtype=torch.int64, device="cuda")
    w = torch.zeros(rs.G, dtype=torch.float64, device="cuda")
    p = ScanParams(case.k, ec.CUTOFF, 0, SPEQ_MODE_LOCAL)
    check(lib().speq_em_scan_reads_device(em._h, d_seq.data_ptr(), d_qual.data_ptr(), d_off.data_ptr(), rd.n,
                                          C.byref(p), cnt.data_ptr(), w.data_ptr(), None))
    torch.cuda.synchronize()
    c = cnt.cpu().numpy().astype(np.uint64)
    check_counters((int(c[0]), int(c[1]), c[2:], w.cpu().numpy()), case.inp, case.k, True)
    assert dev.tuning("last_kernel") == 3
    em.finalize()
    assert em.info() == (h.n_intervals, h.n_entries, h.n_windows)
    check_rows_merged(em, h)
    check_steps(em, case, c[2:])


MERGE_CASES = [ec.Case(ec.Inputs("std", "mixed"), 21, False), ec.Case(ec.Inputs("lowcx", "lowcx"), ec.LOWCX_K, True),
               ec.Case(ec.Inputs("g300", "mixed"), 21, False)]


@pytest.mark.parametrize("case", MERGE_CASES, ids=[c.id for c in MERGE_CASES])
def test_merged_rows_by_hash_and_by_the_collision_fallback(case, monkeypatch):
    """SPEQ_EM_MERGE_ROWS unset (rows matched by hash, then verified), 0 (no merging) and 2 (one hash for every row:
    the assignment by hash alone is wrong, the verification notices, and the exact assignment runs)."""
    rs, rd, h = ec.ref(case.inp.ref), ec.reads(case.inp), ec.histogram(case.inp, case.k)
    assert len(h.merged) < h.n_intervals, "nothing to merge"
    print(f"{case.id}: {h.n_intervals} unmerged rows, {len(h.merged)} merged")
    dev = device(case)
    out = {}
    for env in (None, "0", "2"):
        if env is None:
            monkeypatch.delenv("SPEQ_EM_MERGE_ROWS", raising=False)
        else:
            monkeypatch.setenv("SPEQ_EM_MERGE_ROWS", env)
        em = EmHistogram(dev)
        got = scan_into(em, rd, case.k, case.inp.paired, case.local)
        em.finalize()
        out[env] = (em.info(), em.rows(), [em.step(p, rs.counts, got[2]) for p in ec.percents(rs.G).values()])
        em.close()
    assert out[None][0] == out["0"][0] == out["2"][0] == (h.n_intervals, h.n_entries, h.n_windows)
    assert out[None][1] == out["2"][1]                    # the same rows in the same order
    assert len(out["0"][1]) == h.n_intervals and len(out[None][1]) == len(h.merged)
    for env in ("0", "2"):
        for a, b in zip(out[None][2], out[env][2]):
            np.testing.assert_allclose(b, a, rtol=1e-12, atol=0)  # (only m * (a / norm) is re-associated)
    for a, b in zip(out[None][2], out["2"][2]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("local", [False, True])
def test_step_ieee_branch_matches_the_literal_pass(local):
    """A group count of 0 and non-finite or negative percentages: speq_em_step replays the reference's arithmetic
    row by row, zero terms included (0 * inf, x / 0), so NaNs land where the literal pass puts them."""
    case = ec.Case(ec.Inputs("std", "mixed"), 21, local)
    rs, rd = ec.ref("std"), ec.reads(case.inp)
    dev = device(case)
    em = EmHistogram(dev)
    got = scan_into(em, rd, case.k, False, local)
    em.finalize()
    orc = ec.oracle("std", case.k)
    inf, nan = float("inf"), float("nan")
    n_nan = 0
    for counts, percent in (((3, 0, 2, 3, 1), (20.0, 10.0, 5.0, 1.0, 2.0)),
                            ((3, 0, 2, 3, 1), (20.0, 0.0, 5.0, 1.0, 2.0)),
                            ((0, 0, 2, 0, 1), (1.0, 2.0, 3.0, 4.0, 5.0)),
                            (rs.counts, (inf, 10.0, 5.0, 1.0, 2.0)),
                            (rs.counts, (20.0, 10.0, nan, 1.0, 2.0)),
                            (rs.counts, (20.0, -10.0, 5.0, 1.0, 2.0)),
                            (rs.counts, (-1.0, -10.0, -5.0, -1.0, -2.0)),
                            (rs.counts, (0.0, inf, 0.0, 0.0, 0.0)),
                            ((3, 0, 2, 3, 1), (-inf, 10.0, nan, 1.0, 2.0))):
        with np.errstate(all="ignore"):
            step = em.step(percent, counts, got[2])
            exp = orc.em_pass(rd.seq, rd.qual, rd.offsets, percent, counts, phred_cutoff=ec.CUTOFF, local=local)
        assert np.isnan(step).tolist() == np.isnan(exp).tolist(), (counts, percent, step, exp)
        np.testing.assert_allclose(step, exp, rtol=RTOL, atol=0, equal_nan=True, err_msg=str((counts, percent)))
        n_nan += int(np.isnan(exp).sum())
    assert n_nan > 0
