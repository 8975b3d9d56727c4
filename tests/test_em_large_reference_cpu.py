"""No GPU: the numpy EM reference for large indexes (tests/em_large_reference.py) and the inputs of
tests/test_gpu_em_large.py.

The numpy reference reads intervals off the index's suffix array; the exact pure-Python reference
(tests/em_reference.py) keeps a dictionary of k-mers and knows nothing of a suffix array. On the `std` / `mixed` inputs
of tests/em_cases.py the two must give the same multiset of (entries, multiplicity), the same T and the same U. The
large inputs must meet the conditions the GPU test is built for: more than 1,024 tiles, intervals on both sides of
k_em_scan's second trip, a tile with no interval, and an interval in the last, partial tile."""
from collections import Counter

import numpy as np

import em_cases as ec
import em_large_reference as elr
from speq_amd import FmIndex


def test_numpy_reference_equals_the_exact_reference():
    for inp, k in ((ec.Inputs("std", "mixed"), 21), (ec.Inputs("lowcx", "lowcx"), ec.LOWCX_K),
                   (ec.Inputs("std", "stops", 200), 31)):
        rs, rd, h = ec.ref(inp.ref), ec.reads(inp), ec.histogram(inp, k)
        idx = FmIndex.build(rs.records, rs.groups, rs.G, prefix_q=8)
        e = elr.expected(idx.array("text", np.uint8), idx.array("sa", np.uint32), idx.array("text_start", np.uint64),
                         idx.array("text_group", np.int32), rs.G, k, rd.seq, rd.qual, rd.offsets, ec.CUTOFF)
        assert e.info == (h.n_intervals, h.n_entries, h.n_windows) and h.n_intervals > 0, inp
        assert (e.total, e.unique.tolist()) == (h.total, list(h.unique)), inp
        assert (np.diff(e.lo) > 0).all()
        got = Counter((tuple(zip(e.grp[a:b].tolist(), e.cnt[a:b].tolist())), m)
                      for a, b, m in zip(e.ptr[:-1].tolist(), e.ptr[1:].tolist(), e.mult.tolist()))
        assert got == h.unmerged, inp


def test_large_inputs_meet_the_conditions():
    _, idx, reads, e = elr.large_inputs()
    n = int(idx.info().n)
    assert 4_194_304 < n <= 4_400_000 and e.n == n
    c = e.conditions()
    print(c, e.info)
    assert c["tiles"] >= elr.SCAN_TILES + 1
    assert c["beyond_first_trip"] > 0 and c["within_first_trip"] > 0
    assert c["empty_tiles"] > 0
    assert n % elr.EM_TILE != 0 and c["in_last_partial_tile"] > 0
    # the figures tests/test_gpu_em_large.py quotes: a change of the generator or of a seed shows here first
    assert n == 4_240_009 and c["tiles"] == 1_036 and n % elr.EM_TILE == 649
    assert (c["beyond_first_trip"], c["within_first_trip"], c["empty_tiles"], c["in_last_partial_tile"]) == \
        (3_163, 289_201, 9, 51)
    assert e.info == (292_364, 584_728, 367_962)
    assert reads.n == 4_000 and e.total > 0 and (e.unique > 0).all()
