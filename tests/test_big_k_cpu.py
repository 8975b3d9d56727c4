"""No GPU: the inputs of tests/test_gpu_big_k.py (tests/big_k_inputs.py) hold what the GPU tests rely on, by the oracle
alone, and every k_scan launch past k = 128 fits the 160 KiB of LDS a workgroup may ask for.

The conditions are conditions, not measurements: a read set on which every window passes, no group is named, no unit is
ambiguous or every weight is tiny would let a wrong kernel agree with the oracle on zeros."""
from itertools import product

import numpy as np
import pytest

import big_k_inputs as bk
import variant_table as vt
from oracle.oracle import Oracle
from test_scan_plan_cpu import BASE, GLOBAL, LOCAL, NONE, REF, plan_check  # noqa: F401  (plan_check: a fixture)


@pytest.mark.parametrize("k", bk.KS)
def test_inputs_hold_the_conditions_the_gpu_tests_rely_on(k):
    rd = bk.reads(k)
    lens = np.diff(rd.offsets).astype(np.int64)
    assert rd.n % 2 == 0 and rd.n // 4 >= bk.RUN + 1, "a quarter of the units holds a run and one read more"
    assert (lens[:bk.RUN] == k).all() and (lens[-bk.RUN - 1:-1] == k - 1).all() and lens[-1] > k
    assert {0, k - 1, k, k + 1, k + 63, k + 64, k + 65, 2 * k + 130, 3 * (64 * 2 + k)} <= set(lens.tolist())
    n_win = bk.windows(k)
    for paired in (False, True):
        T, amb, U, W = bk.oracle_scan3(k, paired, True)
        Tg, ambg, Ug, _ = bk.oracle_scan3(k, paired, False)
        print(f"k {k} {'paired' if paired else 'single'}: windows {n_win} T {T} ambiguous {amb} U {U.tolist()} "
              f"W {W.tolist()}")
        assert (T, U.tolist()) == (Tg, Ug.tolist())
        assert 4 * T >= n_win, "at least a quarter of the windows pass the filter"
        assert 10 * (n_win - T) >= n_win, "at least a tenth fail it"
        assert (U > 0).all()
        assert amb > 0 and ambg > 0
        assert T - int(U.sum()) > 0, "shared or absent windows"
        assert np.isfinite(W).all() and (W < 1e300).all() and (W >= U).all() and (W > U).any()
    u_ref, t_ref = bk.ref_unique3(k)
    print(f"k {k}: U_ref {u_ref.tolist()} Tot_ref {t_ref.tolist()}")
    assert ((0 < u_ref) & (u_ref < t_ref)).any()
    assert ((0 < u_ref) & (u_ref < t_ref)).all(), "every group shares a window with another (the planted contigs)"
    # the prefixes the GPU test scans alone
    for n in (0, 1, bk.RUN + 1):
        T, amb, U, _ = bk.oracle_scan3(k, False, False, n)
        assert T == int(np.maximum(lens[:n] - k + 1, 0).sum()) - _bad(rd, k, n)
        assert int(U.sum()) <= T and (n == 0 or T > 0)


def _bad(rd, k, n):
    """Windows of the first n reads that fail the filter."""
    q = np.clip(rd.qual.astype(np.int32) - 33, 0, 41)
    bad = np.concatenate([[0], np.cumsum((q <= bk.CUTOFF) | ~np.isin(rd.seq, np.frombuffer(b"ACGT", np.uint8)))])
    out = 0
    for i in range(n):
        a, b = int(rd.offsets[i]), int(rd.offsets[i + 1])
        if b - a >= k:
            out += int((bad[a + k:b + 1] != bad[a:b - k + 1]).sum())
    return out


@pytest.mark.parametrize("k", bk.K_EM)
def test_em_histograms_hold_multi_group_rows(k):
    """The planted contigs and the record with N put k-mers into two groups; reads cover them at every k."""
    for paired in (False, True):
        h = bk.histogram(k, paired)
        T, _, U, _ = bk.oracle_scan3(k, paired, False)
        assert (h.total, h.unique) == (T, U.tolist())
        assert h.n_intervals >= 2 and h.n_windows >= h.n_intervals
        print(f"k {k}: {h.n_intervals} intervals, {h.n_windows} windows")


def test_relabelled_oracle_equals_the_moved_counts():
    """The labels of a 2049-group replica are names: an oracle built under them gives the three-group answers at the
    labels' places."""
    k, G = 129, 2049
    r, rd = bk.reference(k), bk.reads(k)
    orc = Oracle(r.records, bk.groups_of(k, G), G, k)
    for paired, local in product((False, True), (False, True)):
        T, amb, U, W = orc.scan(rd.seq, rd.qual, rd.offsets, phred_cutoff=bk.CUTOFF, paired=paired, local=local)
        eT, eamb, eU, eW = bk.oracle_scan(k, G, paired, local)
        assert (T, amb) == (eT, eamb) and np.array_equal(U, eU)
        assert W is None and eW is None or np.array_equal(W, eW)
    u, t = orc.ref_unique()
    eu, et = bk.ref_unique(k, G)
    assert np.array_equal(u, eu) and np.array_equal(t, et)


@pytest.mark.parametrize("k,cutoff,q_inf,q_fin", bk.OVERFLOW)
def test_overflow_pairs_by_the_oracle(k, cutoff, q_inf, q_fin):
    """The reference's w = w / (1 - 1/10^(q/10)) overflows to +inf at q_inf and stays finite at q_fin."""
    orc = bk.oracle(k)
    rd = bk.overflow_reads(k, q_inf)
    T, _, U, W = orc.scan(rd.seq, rd.qual, rd.offsets, phred_cutoff=cutoff, local=True)
    assert T == 9 and U.tolist() == [3, 3, 3]
    assert np.isposinf(W).all()
    rd = bk.overflow_reads(k, q_fin)
    T, _, U, W = orc.scan(rd.seq, rd.qual, rd.offsets, phred_cutoff=cutoff, local=True)
    assert T == 9 and U.tolist() == [3, 3, 3]
    assert np.isfinite(W).all() and (W > 1e200).all()
    # one base at the cutoff itself fails every window
    rd = bk.overflow_reads(k, cutoff)
    assert orc.scan(rd.seq, rd.qual, rd.offsets, phred_cutoff=cutoff, local=True)[0] == 0


# ---------------------------------------------------------------- the LDS budget and the plan past k = 128
LDS_LIMIT = 160 * 1024
TUNINGS = list(product((1, 2), (1, 2), (0, 1, 2, 4)))   # ilp, ilp_local, ilp_kt


def test_every_k_scan_plan_past_128_fits_160_kib(plan_check):  # noqa: F811
    """Every k of KS, every mode, G at both sides of the LDS tally's limit, every allowed tuning, with and without an
    EM histogram: plan_scan takes k_scan with LF steps, the instantiation tests/variant_table.py predicts, and its LDS
    stays within 160 KiB. The largest is worked out by hand: k = 4096, local, G = 2048, "ilp_kt" 4: a staging buffer
    of 2 (256 + 4096) = 8704 B; per wave 2 x 8704 + 32 (8704 / 64 + 1) = 21792 B; the histogram 2 x 2048 + 2 words =
    32784 B; the quality table 1008 B: 32784 + 1008 + 4 x 21792 = 120960 B."""
    cases, facts = [], []
    for k, mode, G, (ilp, ilp_local, ilp_kt), em, paired in product(bk.KS, (GLOBAL, LOCAL, REF), (2048, 2049), TUNINGS,
                                                                    (False, True), (False, True)):
        if mode == REF and (em or paired):
            continue
        cases.append((k, mode, G, ilp, ilp_local, ilp_kt, em, paired))
        facts.append(dict(BASE, mode=mode, paired=paired, em=em, k=k, G=G, units=5000 if mode == REF else 300, ilp=ilp,
                          ilp_local=ilp_local, ilp_kt=ilp_kt, ax_usable=0, table=NONE))
    _, plans = plan_check(facts)
    largest = 0
    for (k, mode, G, ilp, ilp_local, ilp_kt, em, paired), plan in zip(cases, plans):
        packed, last_kernel, _grid, buf, lds, lds_launch, table_read = plan
        r = vt.Recipe(f"big{G}", k, paired, mode == LOCAL, vt.REF if mode == REF else vt.EM if em else vt.SCAN,
                      (("ilp", ilp), ("ilp_local", ilp_local), ("ilp_kt", ilp_kt)))
        got = vt.unpack(packed)
        assert got.family == vt.K_SCAN and not got.kt and last_kernel == 0 and not table_read, r.id
        assert got == vt.predict(r), f"{r.id}: planned {got}, the table predicts {vt.predict(r)}"
        assert got.lds_hist == (G <= 2048)
        assert lds <= lds_launch <= LDS_LIMIT, (r.id, lds, lds_launch)
        assert buf >= 2 * (64 * got.width + k), "the staging buffer holds a pass of the chosen width"
        largest = max(largest, lds)
        if (k, mode, G, ilp_kt) == (4096, LOCAL, 2048, 4):
            assert (buf, lds) == (8704, 120960)
    assert largest == 120960
