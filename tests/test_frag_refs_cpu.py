"""CPU: the references of tests/frag_refs.py (short, empty and tiny contigs) are sound inputs, and they bite.

Four independent statements of the per-window semantics must agree on them: the hash-map oracle, the SeqAn-like
stand-in, the pure-Python brute force of tests/golden/make_golden.py (on a reduced instance) and the build's own
label-run algorithm on host cores over the host-built index (k <= 32). The oracle is then what the GPU tests
(tests/test_gpu_frag_refs.py) compare with. The remaining tests are conditions on the inputs, so that the GPU tests
cannot go vacuous: enough records shorter than k, empty, and shorter than a granule; text starts at most residues
mod 32; splice reads over many texts; a group without a reference window; and counts that differ from those of the
same reads against the uncut genomes."""
import os
import sys

import numpy as np
import pytest

import frag_refs as fr
from oracle.oracle import FmCpu, Oracle, SeqanLike
from speq_amd import FmIndex

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden as bf  # noqa: E402

KS = [21, 33, 70]


def same(a, b, local=False):
    assert (a[0], a[1], a[2].tolist()) == (b[0], b[1], b[2].tolist())
    if local:
        np.testing.assert_allclose(a[3], b[3], rtol=1e-12, atol=0)


@pytest.mark.parametrize("paired", [False, True])
def test_oracle_equals_bruteforce_on_a_reduced_instance(paired):
    k, length, L = 9, 400, 45
    f = fr.fragmented(k, length=length)
    rd = fr.reads(k, paired=paired, read_len=L, length=length, n_genome=60, n_splice=60)
    assert min(len(r) for r in f.records) == 0 and any(len(r) == k - 1 for r in f.records[:f.n_cut])
    recs = [r.decode() for r in f.records]
    texts = bf.texts_of(recs)
    dgs = [g for g in f.groups for _ in (0, 1)]
    rs, qs = bf.reads_lists(rd)
    orc = Oracle(f.records, f.groups, f.G, k)
    u, t = orc.ref_unique()
    bu, bt = bf.ref_unique(recs, texts, dgs, list(f.groups), f.G, k)
    assert u.tolist() == bu and t.tolist() == bt
    assert t[fr.GENOMES] == 0 and t[:fr.GENOMES].all()
    for local in (False, True):
        got = orc.scan(rd.seq, rd.qual, rd.offsets, paired=paired, local=local)
        bT, bamb, bU, bW = bf.scan(texts, dgs, f.G, rs, qs, k, 30, local, paired)
        assert (got[0], got[1], got[2].tolist()) == (bT, bamb, bU)
        assert got[0] > 0 and sum(bU) > 0
        if local:
            np.testing.assert_allclose(got[3], bW, rtol=1e-12)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("paired", [False, True])
def test_oracle_equals_seqan_like_and_label_runs(k, paired):
    f, rd = fr.fragmented(k), fr.reads(k, paired)
    orc = Oracle(f.records, f.groups, f.G, k)
    sl = SeqanLike(f.records, f.groups, f.G)
    for local in (False, True):
        a = orc.scan(rd.seq, rd.qual, rd.offsets, paired=paired, local=local)
        same(sl.scan(rd.seq, rd.qual, rd.offsets, k=k, paired=paired, local=local), a, local)
    if k <= 32:
        a = orc.scan(rd.seq, rd.qual, rd.offsets, paired=paired)
        for q, pairs, tri in ((8, True, True), (0, False, False)):
            idx = FmIndex.build(f.records, f.groups, f.G, prefix_q=q, pair_steps=pairs, triple_steps=tri)
            got = FmCpu(idx).scan(rd.seq, rd.qual, rd.offsets, k=k, paired=paired)
            assert (got[0], got[1], got[2].tolist()) == (a[0], a[1], a[2].tolist()), q


@pytest.mark.parametrize("case", fr.TINY, ids=fr.TINY_IDS)
def test_tiny_collections_agree(case):
    records, groups, G, k, rd = case
    assert fr.fm_length(records) < 256
    orc = Oracle(records, groups, G, k)
    a = orc.scan(rd.seq, rd.qual, rd.offsets)
    sl = SeqanLike(records, groups, G)
    for local in (False, True):
        same(sl.scan(rd.seq, rd.qual, rd.offsets, k=k, local=local), orc.scan(rd.seq, rd.qual, rd.offsets, local=local),
             local)
    idx = FmIndex.build(records, groups, G, prefix_q=3, pair_steps=True, triple_steps=True)
    assert idx.info().n == fr.fm_length(records)
    got = FmCpu(idx).scan(rd.seq, rd.qual, rd.offsets, k=k)
    assert (got[0], got[1], got[2].tolist()) == (a[0], a[1], a[2].tolist())
    recs = [r.decode() for r in records]
    u, t = orc.ref_unique()
    bu, bt = bf.ref_unique(recs, bf.texts_of(recs), [g for g in groups for _ in (0, 1)], list(groups), G, k)
    assert u.tolist() == bu and t.tolist() == bt
    lens = np.diff(rd.offsets).astype(np.int64)
    assert lens.max() > fr.fm_length(records) and (lens == 0).any() and (lens == k - 1).any()
    assert 0 < a[0] <= int(np.maximum(lens - k + 1, 0).sum())


def test_tiny_collections_cover_the_sizes():
    ns = sorted(fr.fm_length(c[0]) for c in fr.TINY)
    for lo, hi in ((1, 32), (32, 96), (96, 160), (160, 256)):  # a granule, an occ block, AX_CMP bases, an S block
        assert any(lo <= n < hi for n in ns), (lo, hi, ns)
    no_window = [c for c in fr.TINY if all(len(r) < c[3] for r in c[0])]
    assert no_window and all(Oracle(c[0], c[1], c[2], c[3]).ref_unique()[1].sum() == 0 for c in no_window)
    assert any(b"" in c[0] for c in fr.TINY) and any(b"N" in r for c in fr.TINY for r in c[0])


@pytest.mark.parametrize("k", KS + [128])
def test_inputs_are_not_vacuous(k):
    f = fr.fragmented(k)
    L = 250 if k == 128 else 150
    rd = fr.reads(k, read_len=L)
    lens = [len(r) for r in f.records[:f.n_cut]]  # (the fifth group would satisfy all of these by itself)
    assert sum(n < k for n in lens) >= 10
    assert lens.count(0) >= 3
    assert sum(n < 32 for n in lens) >= 10
    assert {k - 1, k, k + 1} <= set(lens)
    assert all(len(r) < k for r in f.records[f.n_cut:]) and len(f.records) > f.n_cut
    # text starts, as the index has them
    idx = FmIndex.build(f.records, f.groups, f.G)
    ts = idx.array("text_start", np.uint64)
    assert np.array_equal(ts[:-1], fr.text_starts(f.records).astype(np.uint64))
    res = set((ts[:2 * f.n_cut] % np.uint64(32)).tolist())
    assert len(res) >= 24, len(res)
    _, spans = fr.splice_reads(f.records, fr.N_SPLICE, L)
    assert max(spans) >= 6 and sum(s >= 6 for s in spans) >= 10 and len(spans) >= 400
    assert len(fr.contig_reads(f.records, k, L)) >= 10
    # against the uncut genomes the same reads count differently
    orc = Oracle(f.records, f.groups, f.G, k)
    u_ref, tot_ref = orc.ref_unique()
    assert tot_ref[fr.GENOMES] == 0 and u_ref[fr.GENOMES] == 0 and tot_ref[:fr.GENOMES].all()
    T, amb, U, _ = orc.scan(rd.seq, rd.qual, rd.offsets)
    whole = Oracle(f.uncut.records, f.uncut.groups, fr.GENOMES, k)
    T0, amb0, U0, _ = whole.scan(rd.seq, rd.qual, rd.offsets)
    print(f"k={k}: {len(f.records)} records ({f.n_cut} cut from the genomes), {len(res)} text-start residues, "
          f"longest splice {max(spans)} texts; fragmented T={T} ambiguous={amb} U={U.tolist()}, "
          f"uncut ambiguous={amb0} U={U0.tolist()}")
    assert T == T0 and U[fr.GENOMES] == 0
    assert all(U[g] != U0[g] for g in range(fr.GENOMES))
    assert amb >= amb0 + 50, (amb, amb0)


@pytest.mark.parametrize("k", [21, 70])
@pytest.mark.parametrize("paired", [False, True])
def test_em_reference_takes_these_inputs(k, paired):
    """tests/em_reference.py (what the EM rows are compared with) classifies the windows as the oracle does, and the
    oracle's literal EM pass lies within tests/test_em_reference_cpu.py's bound of its exact step."""
    import em_cases as ec
    import em_reference as er
    f, rd = fr.fragmented(k), fr.reads(k, paired)
    h = er.scan(er.build_index(f.records, f.groups, f.G, k), f.G, k, rd.seq, rd.qual, rd.offsets, cutoff=ec.CUTOFF,
                paired=paired)
    orc = Oracle(f.records, f.groups, f.G, k)
    T, _, U, _ = orc.scan(rd.seq, rd.qual, rd.offsets, phred_cutoff=ec.CUTOFF, paired=paired)
    assert h.total == T and h.unique == U.tolist() and h.total == h.absent + sum(h.unique) + h.n_windows
    assert h.n_windows > 100 and h.n_intervals > 50 and len(h.merged) <= h.n_intervals
    counts = tuple(g % 3 + 1 for g in range(f.G))
    bound = (h.n_windows + 2 * f.G + 8) * 2.0 ** -53
    for which, percent in ec.percents(f.G).items():
        lit = orc.em_pass(rd.seq, rd.qual, rd.offsets, percent, counts, phred_cutoff=ec.CUTOFF, paired=paired,
                          local=paired)
        dev = er.max_relative_deviation(lit, er.exact_step(percent, counts, h.unique, h.merged))
        assert dev <= bound, (which, dev, bound)
