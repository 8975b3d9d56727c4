"""CPU: the pure-Python exact reference of the EM histogram (tests/em_reference.py) against the C oracle, on every
input set of tests/test_gpu_em_rows.py (tests/em_cases.py).

The two share no code: the oracle is a C hash map with occurrence lists, the reference a Python dict of k-mer
strings. Checked here: the single-group tallies, the class of every passing window, the non-vacuity of the inputs that
aim at one recording site of the kernels, and the oracle's literal fp64 EM pass against the exact rational step.

The bound on the literal pass: with non-negative finite percentages and positive group counts every term is
non-negative (no cancellation); a window's terms a_g / norm carry a constant number of roundings, and next[g] takes
one more per addition. The bound counts the additions of multi-group windows, (n_windows + 2 G + 8) * 2^-53 relative;
the additions of single-group windows add exactly 1.0 and also round once next[g] is no integer, so the bound is not
a strict worst case, but roundings do not all point one way: the largest deviation seen over all the input sets is
0.25 of the bound, at 1,000-base error-free reads and k = 128, where single-group windows dominate (printed by test_oracle_em_pass_within_bound_of_exact_step)."""
import numpy as np
import pytest

import em_cases as ec
import em_reference as er

U = 2.0 ** -53
_worst = {"ratio": 0.0, "at": None}


@pytest.mark.parametrize("inp,k", ec.INPUT_SETS, ids=[f"{i.id}-k{k}" for i, k in ec.INPUT_SETS])
def test_reference_classifies_windows_as_the_oracle_does(inp, k):
    rs, rd, h = ec.ref(inp.ref), ec.reads(inp), ec.histogram(inp, k)
    T, _, Uo, _ = ec.oracle_scan(inp, k, False)
    assert h.total == T
    assert h.unique == Uo.tolist()
    assert h.total == h.absent + sum(h.unique) + h.n_windows
    # every passing window: absent, its group, or -2
    idx, orc = ec.index(inp.ref, k), ec.oracle(inp.ref, k)
    s5 = er.dna5(rd.seq.tobytes())
    s_arr = np.frombuffer(s5, dtype=np.uint8)
    seen = set()
    for r in range(rd.n):
        a, b = int(rd.offsets[r]), int(rd.offsets[r + 1])
        for j in er.passing_windows(s_arr[a:b], rd.qual[a:b], k, ec.CUTOFF).tolist():
            w = s5[a + j:a + j + k]
            if w in seen:
                continue
            seen.add(w)
            c = idx.get(w)
            assert orc.lookup(w) == (-1 if c is None else c[0][0] if len(c) == 1 else -2), w
    # the derived values hang together
    assert h.n_intervals == len(h.multi) == sum(h.unmerged.values())
    assert sum(h.merged.values()) == h.n_windows and len(h.merged) <= h.n_intervals
    assert all(len(c) >= 2 and list(c) == sorted(c) and all(n >= 1 for _, n in c) for c, _ in h.multi.values())
    if rs.G == 1:
        assert h.n_windows == 0
    elif inp.kind != "repeat":
        assert h.n_windows > 100 and h.n_intervals > 50, "the input set records too little"


@pytest.mark.parametrize("inp,k,local", ec.EM_SETS,
                         ids=[f"{i.id}-k{k}-{'local' if l else 'global'}" for i, k, l in ec.EM_SETS])
def test_oracle_em_pass_within_bound_of_exact_step(inp, k, local):
    rs, h = ec.ref(inp.ref), ec.histogram(inp, k)
    bound = (h.n_windows + 2 * rs.G + 8) * U
    for which in ec.percents(rs.G):
        exact = ec.exact_step(inp, k, which)
        dev = er.max_relative_deviation(ec.oracle_em_pass(inp, k, local, which), exact)
        if dev / bound > _worst["ratio"]:
            _worst.update(ratio=dev / bound, at=(inp.id, k, local, which))
        assert dev <= bound, (which, dev, bound)
    print(f"largest oracle deviation / bound so far: {_worst['ratio']:.4f} at {_worst['at']}")


def test_exact_step_on_a_hand_computed_histogram():
    # two groups, p = (1, 3), n = (1, 2): weights 1 and 3/2. One window with counts (1, 1) three times, one with (2, 1)
    # once; 5 and 7 single-group windows.
    merged = {((0, 1), (1, 1)): 3, ((0, 2), (1, 1)): 1}
    got = er.exact_step([1.0, 3.0], [1, 2], [5, 7], merged)
    from fractions import Fraction as F
    assert got == [5 + 3 * F(2, 5) + F(4, 7), 7 + 3 * F(3, 5) + F(3, 7)]
    # a zero percentage takes its group out of every window, and its single-group windows out of the sum
    assert er.exact_step([0.0, 3.0], [1, 2], [5, 7], merged) == [0, 7 + 4]
    assert er.exact_step([0.0, 0.0], [1, 2], [5, 7], merged) == [0, 0]


def test_index_counts_every_occurrence():
    # AACGTT is its own reverse complement: twice per record; N and record ends cut windows
    idx = er.build_index([b"AACGTT", b"aacguuNAACGTT", b"CCCCCCC"], [0, 1, 1], 2, 6)
    assert idx[b"AACGTT"] == ((0, 2), (1, 4))
    assert idx[b"CCCCCC"] == ((1, 2),) and idx[b"GGGGGG"] == ((1, 2),)
    assert len(idx) == 3


def test_deferred_inputs_reach_the_deferred_site():
    """At least a tenth of the multi-group windows lie in reads that hold an error (k_scan_ax records those in its
    deferred-window pass when the anchor's run ended at the error)."""
    for k in (21, 31, 70):
        inp = ec.Inputs("std", "deferred")
        rd, h = ec.reads(inp), ec.histogram(inp, k)
        in_err = sum(len(at) for at, e in zip(h.multi_at, rd.has_error) if e)
        print(f"deferred k={k}: {in_err} of {h.n_windows} multi-group windows in reads with an error")
        assert h.n_windows > 500 and in_err * 10 >= h.n_windows


def test_stop_inputs_have_windows_on_both_sides():
    """At least 50 reads with multi-group windows both wholly before and wholly after their stop."""
    for k in (21, 31, 70):
        inp = ec.Inputs("std", "stops", 200)
        rd, h = ec.reads(inp), ec.histogram(inp, k)
        both = sum(1 for at, lo, hi in zip(h.multi_at, rd.stop_lo, rd.stop_hi)
                   if any(j + k <= lo for j in at) and any(j >= hi for j in at))
        print(f"stops k={k}: {both} of {rd.n} reads with multi-group windows on both sides of the stop")
        assert both >= 50


def test_low_complexity_reference_holds_what_it_should():
    rs, k = ec.ref("lowcx"), ec.LOWCX_K
    idx, h = ec.index("lowcx", k), ec.histogram(ec.Inputs("lowcx", "lowcx"), k)
    assert idx[rs.marks["pal"]] == ((0, 4), (1, 4))          # 2 records per group, both strands each
    assert idx[b"A" * k] == ((0, 2 * (80 - k + 1)), (1, 2 * (95 - k + 1)))
    assert rs.marks["pal"] in h.multi and b"A" * k in h.multi and b"T" * k in h.multi
    assert max(n for c, _ in h.multi.values() for _, n in c) >= 2 * (95 - k + 1)
    # the segment that group 2 alone repeats: counted in U[2], never a row
    tw = rs.marks["twice"]
    inside = [tw[i:i + k] for i in range(len(tw) - k + 1)]
    assert all(idx[w] == ((2, 4),) for w in inside)
    assert not any(w in h.multi for w in inside)
    rd = ec.reads(ec.Inputs("lowcx", "lowcx"))
    seq = rd.seq.tobytes()
    hits = sum(seq.count(w) for w in inside)
    assert hits > 100 and h.unique[2] >= hits
