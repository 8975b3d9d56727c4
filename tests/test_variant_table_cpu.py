"""No GPU: the hand-written dispatch table (tests/variant_table.py) is consistent with itself, and the ledger's inputs
(tests/variant_inputs.py) are ones on which a wrong instantiation would show.

The plan reaches every instantiation the rules can produce and nothing else; the enumeration has the counts the
dispatcher's templates give; and on every read set the references alone find ambiguous units, many counted groups
(the far end of the 2049-group tally among them) and multi-group histogram rows."""
from collections import Counter

import numpy as np
import pytest

import variant_inputs as vi
import variant_table as vt
from speq_amd import FmIndex


def test_enumeration_counts():
    assert len(vt.ALL_VARIANTS) == sum(vt.COUNTS.values()) == 208
    assert Counter(v.family for v in vt.ALL_VARIANTS) == vt.COUNTS
    ks = [v for v in vt.ALL_VARIANTS if v.family == vt.K_SCAN]
    assert sum(v.mode == "ref" for v in ks) == 8
    assert sum(v.mode != "ref" and not v.kt for v in ks) == 24 and sum(v.mode != "ref" and v.kt for v in ks) == 28
    assert sum(v.stats for v in vt.ALL_VARIANTS) == 20
    assert sum(not v.lds_hist for v in vt.ALL_VARIANTS) == 94   # the global-atomic plane
    for v in vt.ALL_VARIANTS:
        assert vt.unpack(v.pack()) == v
    assert len({v.pack() for v in vt.ALL_VARIANTS}) == 208


def test_plan_reaches_exactly_every_variant():
    reached = Counter(vt.predict(r) for r in vt.PLAN)
    assert set(reached) - vt.ALL_VARIANTS == set(), "the plan lands outside the enumeration"
    assert [str(v) for v in sorted(vt.ALL_VARIANTS - set(reached))] == [], "unreached"
    assert len({r for r in vt.PLAN}) == len(vt.PLAN), "a recipe twice"


def test_plan_recipes_are_runnable():
    for r in vt.PLAN:
        assert r.ref in vt.REFS and r.entry in (vt.SCAN, vt.EM, vt.STATS, vt.REF)
        assert set(dict(r.tune)) <= set(vt.DEFAULTS) and "kt_compact" not in dict(r.tune), r.id
        assert vt.read_len(r.k) >= r.k and vt.read_len(r.k) <= vt.REFS[r.ref].length
        if r.entry == vt.STATS:
            assert vt.predict(r).stats and vt.REFS[r.ref].G <= vt.LDS_HIST_MAX_G
    # a recipe outside what the instrumented twin takes is an error of the table, not another variant
    with pytest.raises(ValueError):
        vt.predict(vt.Recipe("g2049", 21, False, False, vt.STATS))
    with pytest.raises(ValueError):
        vt.predict(vt.Recipe("g5", 140, False, False, vt.STATS))


@pytest.mark.parametrize("name", list(vt.REFS))
def test_reference_shapes(name):
    """The shapes the table assumes are the ones the inputs build (the m-mer filter's m depends on the text length)."""
    shape, r = vt.REFS[name], vi.ref(name)
    assert (len(r.records), len(set(r.groups)), len(r.records[0])) == \
        (shape.n_variants * shape.n_isolates, shape.G, shape.length)
    idx = FmIndex.build(r.records, r.groups, shape.G, prefix_q=8)
    assert idx.info().n == shape.text_len < 4 << 20   # ("ilp" opens at 2 below 4 M symbols)
    assert (name == "g2049") == (shape.G > vt.LDS_HIST_MAX_G) and (name != "g2049" or shape.G == 2049)
    # ax_sproof 2 (the default) is on at k = 21 and off at k = 25 on both references
    assert vt.mfilter_m(shape.text_len, vt.K_COMPACT) == 0 and vt.mfilter_m(shape.text_len, vt.K_WIDE) > 0


@pytest.mark.parametrize("name,k,paired", vt.INPUT_SETS, ids=[f"{n}-k{k}-{'pe' if p else 'se'}"
                                                              for n, k, p in vt.INPUT_SETS])
def test_input_conditions_hold_by_the_references_alone(name, k, paired):
    G = vt.REFS[name].G
    rd = vi.reads_of(name, k, paired)
    units = vi.N_PLAIN + vi.N_CHIMERIC + vi.N_CLEAN
    assert rd.n == units * (2 if paired else 1) and units > 4 * 64   # more than one wave of the anchor kernel
    assert set(np.diff(rd.offsets).tolist()) == {vt.read_len(k)}
    T, amb, U, W = vi.oracle_scan(name, k, paired, True)
    h = vi.histogram(name, k, paired)
    print(f"{name} k={k} paired={paired}: T={T} ambiguous={amb} groups counted={int((U > 0).sum())} "
          f"rows={h.info[0]} merged={len(h.merged)}")
    assert amb >= 2
    assert int((U > 0).sum()) >= min(64, G)
    if G > vt.LDS_HIST_MAX_G:
        assert (U[G - 64:] > 0).any(), "no counted group among the last 64"
    assert h.info[0] >= 100
    assert (W > 0).tolist() == (U > 0).tolist()
    # the two references agree with each other on the integers (they share no code)
    assert (h.exact.total, h.exact.unique) == (T, U.tolist())
    assert vi.oracle_scan(name, k, paired, False)[:2] == (T, amb)
