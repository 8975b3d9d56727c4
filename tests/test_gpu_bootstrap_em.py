"""GPU: one EM histogram per bootstrap replicate (speq_bootstrap_attach_em / _finalize_em, `speq scan --bootstrap-em`)
against the pure-Python model (tests/bootstrap_em_model.py; validated by tests/test_bootstrap_em_cpu.py).

The multiplicities are integers, so every comparison of `mult` is exact equality with the model; the counts of a handle
with a histogram attached are compared exactly, and its local weights within tests/test_gpu_bootstrap.py's bound, with
the model of a handle without. Inputs: the bootstrap tests' base input (3 groups: 15,591 intervals in 4 merged rows at
k = 21), the 70-group input of tests/bootstrap_em_inputs.py (603 rows, more than a block's LDS takes), and the golden
FASTQ cases through the CLI."""
import os
import shutil
import subprocess
from collections import Counter
from functools import lru_cache

import numpy as np
import pytest

import bootstrap_em_inputs as bi
import bootstrap_em_model as bem
import bootstrap_model as bm
import em_reference as er
import read_report_inputs as ri
from golden_io import Case
from oracle.oracle import Oracle
from speq_amd import (Bootstrap, DeviceIndex, EmHistogram, FmIndex, SpeqError, bootstrap_summary_percent, em_refine,
                      em_rows_refine, file_to_map, unique_to_percent)
from speq_amd._lib import SPEQ_E_ARG

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEQ = os.path.join(ROOT, "bin", "speq")
FULL = dict(pair_steps=True, triple_steps=True, label_table=True)
BS = [1, 63, 64, 65, 129]
SEED = 7
LDS_BUDGET = 64 << 10


def lds_rows(n_rows: int, B: int, G: int, local: bool, k: int) -> int:
    """H as include/speq_scan.h states it: what is left of 64 KiB after the tile search's four wave regions and, when
    they take the LDS path, the counters, in rows of 8 (B + 1) bytes."""
    waves = 4 * ((3 * (64 + k) + 15) & ~15)
    acc = 8 * (B + 1) * (G + 2 + (G if local else 0))
    taken = waves + (acc if acc + waves <= LDS_BUDGET else 0)
    return min(n_rows, max(LDS_BUDGET - taken, 0) // (8 * (B + 1)))


# ---- inputs ----
@pytest.fixture(scope="module")
def dev():
    ref = ri.base_ref()
    d = DeviceIndex(FmIndex.build(ref.records, ref.groups, 3, prefix_q=8, **FULL))
    yield d
    d.close()


@pytest.fixture(scope="module")
def dev70():
    ref = bi.ref70()
    d = DeviceIndex(FmIndex.build(ref.records, ref.groups, bi.G70, prefix_q=8, **FULL))
    yield d
    d.close()


def histogram(d, reads, k, paired=False, local=False) -> EmHistogram:
    em = EmHistogram(d)
    em.scan(*reads, k=k, phred_cutoff=ri.CUTOFF, paired=paired, local=local)
    em.finalize()
    return em


@lru_cache(maxsize=None)
def base_units(k: int, paired: bool) -> bm.Units:
    return bm.units(bi.base_index(k), 3, k, *ri.base_reads(k), ri.CUTOFF, paired, True)


def run(d, em, k, reads, B, paired, local, seed=SEED, first_unit=0):
    """((counts, weights), (mult, missed), em_info, info) of one handle with em attached."""
    b = Bootstrap(d, k, B, seed, ri.CUTOFF, paired, local)
    b.attach_em(em)
    b.add(*reads, first_unit)
    out = b.finalize(), b.finalize_em(), b.em_info(), b.info()
    b.close()
    return out


def assert_counts(got, un: bm.Units, B, local, k, **kw):
    (gc, gw), (ec, ew) = got, bm.replicates(un, SEED, B, **kw)
    np.testing.assert_array_equal(gc, ec)
    assert (gw is None) == (not local)
    if local:
        assert (np.abs(gw - ew) <= bm.weights_bound(k, ec) * ew).all()


def _to_device(reads):
    import torch
    seq, qual, off = reads
    return (torch.from_numpy(np.frombuffer(seq, np.uint8).copy()).cuda(),
            torch.from_numpy(np.frombuffer(qual, np.uint8).copy()).cuda(),
            torch.from_numpy(np.asarray(off).astype(np.int64)).cuda())


def _split(reads, n0: int, n1: int):
    seq, qual, off = reads
    a, b = int(off[n0]), int(off[n1])
    return seq[a:b], qual[a:b], off[n0:n1 + 1] - off[n0]


# ---- the base input ----
@pytest.mark.parametrize("local", [False, True], ids=["global", "local"])
@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
@pytest.mark.parametrize("k", [8, 21, 70, 151])
def test_base_reads_equal_the_model_and_row_0_the_histogram(dev, k, paired, local):
    reads = ri.base_reads(k)
    mu = bi.base_multi(k, paired)
    em = histogram(dev, reads, k, paired, local)
    rows = em.rows()
    contents = [c for _, c in rows]
    assert {c: m for m, c in rows} == mu.hist.merged
    lo, row = em.intervals()
    assert len(lo) == em.info()[0] == mu.hist.n_intervals and (np.diff(lo.astype(np.int64)) > 0).all()
    assert row.max() == len(rows) - 1 and set(row.tolist()) == set(range(len(rows)))
    for B in BS:
        plain = Bootstrap(dev, k, B, SEED, ri.CUTOFF, paired, local)
        plain.add(*reads)
        pc, pw = plain.finalize()
        plain.close()
        (counts, w), (mult, missed), em_info, info = run(dev, em, k, reads, B, paired, local)
        exp, _ = bem.mult(mu, contents, SEED, B)
        assert mult.dtype == np.uint64 and mult.shape == exp.shape
        np.testing.assert_array_equal(mult, exp)
        assert mult[0].tolist() == [m for m, _ in rows] and missed == 0
        np.testing.assert_array_equal(counts, pc)
        assert_counts((counts, w), base_units(k, paired), B, local, k)
        assert em_info == {"n_rows": len(rows), "lds_rows": lds_rows(len(rows), B, 3, local, k)}
        assert info["units_added"] == mu.n
    assert (mult[1:] != mult[0]).any()
    em.close()


def test_one_row_per_interval(dev, monkeypatch):
    """SPEQ_EM_MERGE_ROWS=0: the identity map, 15,591 rows, of which a block's LDS takes 121 at B = 63: nearly every add
    is a device atomic, and a tile of 64 distinct k-mers is 64 rounds."""
    k, B = 21, 63
    reads = ri.base_reads(k)
    mu = bi.base_multi(k, False)
    monkeypatch.setenv("SPEQ_EM_MERGE_ROWS", "0")
    em = histogram(dev, reads, k)
    monkeypatch.delenv("SPEQ_EM_MERGE_ROWS")
    rows = em.rows()
    lo, row = em.intervals()
    assert len(rows) == 15_591 and row.tolist() == list(range(15_591))
    _, (mult, missed), em_info, _ = run(dev, em, k, reads, B, False, False)
    assert missed == 0 and mult[0].tolist() == [m for m, _ in rows]
    assert em_info == {"n_rows": 15_591, "lds_rows": lds_rows(15_591, B, 3, False, k)} and em_info["lds_rows"] == 121
    assert Counter((c, tuple(mult[:, r].tolist())) for r, (_, c) in enumerate(rows)) == bem.mult_by_kmer(mu, SEED, B)
    em.close()
    # the collision fallback of the merge gives the same map as the hashes
    monkeypatch.setenv("SPEQ_EM_MERGE_ROWS", "2")
    em2 = histogram(dev, reads, k)
    monkeypatch.delenv("SPEQ_EM_MERGE_ROWS")
    em1 = histogram(dev, reads, k)
    assert em2.rows() == em1.rows() and len(em1.rows()) == 4
    np.testing.assert_array_equal(em2.intervals()[1], em1.intervals()[1])
    np.testing.assert_array_equal(em1.intervals()[0], lo)
    assert [rows[i][1] for i in range(len(lo))] == [em1.rows()[r][1] for r in em1.intervals()[1]]
    em1.close()
    em2.close()


# ---- 70 groups: LDS rows and device rows in one launch ----
@pytest.mark.parametrize("B,local", [(63, False), (63, True), (1024, False)], ids=["B63", "B63-local", "B1024"])
def test_70_groups(dev70, B, local):
    k = bi.K
    reads = bi.reads70()
    mu = bi.multi70()
    em = histogram(dev70, reads, k, local=local)
    rows = em.rows()
    assert len(rows) == 603 and {c: m for m, c in rows} == mu.hist.merged
    got, (mult, missed), em_info, info = run(dev70, em, k, reads, B, False, local)
    H = lds_rows(603, B, bi.G70, local, k)
    assert em_info == {"n_rows": 603, "lds_rows": H} and H == {(63, False): 54, (63, True): 126, (1024, False): 7}[B, local]
    exp, _ = bem.mult(mu, [c for _, c in rows], SEED, B)
    np.testing.assert_array_equal(mult, exp)
    assert missed == 0 and mult[0].tolist() == [m for m, _ in rows] and max(mult[0]) == 7_270
    # rows on both sides of H were hit
    order = np.argsort(-mult[0].astype(np.int64), kind="stable")
    assert mult[1:, order[:H]].any() and mult[1:, order[H:]].any()
    un = bm.units(bi.index70(), bi.G70, k, *reads, bi.CUTOFF, False, True)
    assert_counts(got, un, B, local, k)
    assert info["lds_path"] == (B == 63 and not local)
    em.close()


def test_reads_absent_from_the_histogram_are_missed(dev70):
    k, B, n = bi.K, 2, 150
    seq, qual, off = bi.reads70()
    head = (seq[:int(off[n])], qual[:int(off[n])], off[:n + 1])
    sub = bem.multi_units(bi.index70(), bi.G70, k, *head, bi.CUTOFF)
    em = histogram(dev70, head, k)
    rows = em.rows()
    _, (mult, missed), _, _ = run(dev70, em, k, bi.reads70(), B, False, False)
    exp, exp_missed = bem.mult_in_table(bi.multi70(), sub, [c for _, c in rows], SEED, B)
    np.testing.assert_array_equal(mult, exp)
    assert missed == exp_missed > 0
    em.close()


# ---- unit indices, entry points, repeats ----
def test_first_unit_splits_and_a_large_index(dev):
    import torch
    k, B = 21, 65
    reads = ri.base_reads(k)
    n = len(reads[2]) - 1
    for paired in (False, True):
        mu = bi.base_multi(k, paired)
        em = histogram(dev, reads, k, paired)
        contents = [c for _, c in em.rows()]
        exp, _ = bem.mult(mu, contents, SEED, B)
        per = 2 if paired else 1
        cut_unit = 777
        parts = [_to_device(_split(reads, 0, cut_unit * per)), _to_device(_split(reads, cut_unit * per, n))]
        torch.cuda.synchronize()
        two = Bootstrap(dev, k, B, SEED, ri.CUTOFF, paired, False)
        two.attach_em(em)
        for (s, q, o), first in zip(parts, (0, cut_unit)):
            two.add_device(s.data_ptr(), q.data_ptr(), o.data_ptr(), len(o) - 1, first_unit=first)
        mult, missed = two.finalize_em()
        np.testing.assert_array_equal(mult, exp)
        assert missed == 0
        two.close()
        wrong = Bootstrap(dev, k, B, SEED, ri.CUTOFF, paired, False)
        wrong.attach_em(em)
        for s, q, o in parts:
            wrong.add_device(s.data_ptr(), q.data_ptr(), o.data_ptr(), len(o) - 1)
        wm, _ = wrong.finalize_em()
        assert wm[0].tolist() == exp[0].tolist() and (wm[1:] != exp[1:]).any()
        wrong.close()
        big = (1 << 40) + 5
        _, (mult, missed), _, _ = run(dev, em, k, reads, B, paired, False, first_unit=big)
        np.testing.assert_array_equal(mult, bem.mult(mu, contents, SEED, B, first_unit=big)[0])
        assert (mult != bem.mult(mu, contents, SEED, B, first_unit=5)[0]).any()
        em.close()


def test_host_add_equals_device_add_and_finalize_twice(dev):
    import torch
    k, B = 21, 64
    reads = ri.base_reads(k)
    n = len(reads[2]) - 1
    mu = bi.base_multi(k, True)
    em = histogram(dev, reads, k, True, True)
    contents = [c for _, c in em.rows()]
    exp, _ = bem.mult(mu, contents, SEED, B)
    _, (host, _), _, _ = run(dev, em, k, reads, B, True, True)
    d_reads = _to_device(reads)
    torch.cuda.synchronize()
    b = Bootstrap(dev, k, B, SEED, ri.CUTOFF, True, True)
    b.attach_em(em)
    b.add_device(d_reads[0].data_ptr(), d_reads[1].data_ptr(), d_reads[2].data_ptr(), n)
    device, _ = b.finalize_em()
    b.close()
    np.testing.assert_array_equal(host, exp)
    np.testing.assert_array_equal(device, exp)
    # finalize twice with an add in between; the histogram itself may be gone by then
    half = n // 4 * 2  # (whole pairs)
    b = Bootstrap(dev, k, B, SEED, ri.CUTOFF, True, False)
    b.attach_em(em)
    em.close()
    mult, missed = b.finalize_em()
    assert not mult.any() and missed == 0
    b.add(*_split(reads, 0, half))
    first, _ = b.finalize_em()
    again, _ = b.finalize_em()
    np.testing.assert_array_equal(first, again)
    head = bem.MultiUnits(half // 2, mu.by_content[:half // 2], mu.by_kmer[:half // 2], mu.content_of, mu.hist)
    np.testing.assert_array_equal(first, bem.mult(head, contents, SEED, B)[0])
    b.add(*_split(reads, half, n), first_unit=half // 2)
    np.testing.assert_array_equal(b.finalize_em()[0], exp)
    assert_counts(b.finalize(), base_units(k, True), B, False, k)
    b.close()


def test_attach_errors(dev, dev70):
    k = 21
    reads = ri.base_reads(k)
    em = histogram(dev, reads, k)
    raw = EmHistogram(dev)
    b = Bootstrap(dev, k, 8, SEED, ri.CUTOFF)
    for call in (b.em_info, b.finalize_em):
        with pytest.raises(SpeqError) as e:
            call()
        assert e.value.code == SPEQ_E_ARG and "no histogram attached" in str(e.value)
    with pytest.raises(SpeqError) as e:
        b.attach_em(raw)
    assert e.value.code == SPEQ_E_ARG and "not finalized" in str(e.value)
    other = Bootstrap(dev70, k, 8, SEED, ri.CUTOFF)
    with pytest.raises(SpeqError) as e:
        other.attach_em(em)
    assert e.value.code == SPEQ_E_ARG and "another replica" in str(e.value)
    other.close()
    b.attach_em(em)
    with pytest.raises(SpeqError) as e:
        b.attach_em(em)
    assert e.value.code == SPEQ_E_ARG and "attached already" in str(e.value)
    b.close()
    late = Bootstrap(dev, k, 8, SEED, ri.CUTOFF)
    late.add(*reads)
    with pytest.raises(SpeqError) as e:
        late.attach_em(em)
    assert e.value.code == SPEQ_E_ARG and "added already" in str(e.value)
    np.testing.assert_array_equal(late.finalize()[0], bm.replicates(base_units(k, False), SEED, 8)[0])
    late.close()
    raw.close()
    em.close()


# ---- files ----
def _write_fastq(path, seq, qual, off, start: int, step: int):
    with open(path, "wb") as f:
        f.write(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, seq[int(off[i]):int(off[i + 1])], qual[int(off[i]):int(off[i + 1])])
                         for i in range(start, len(off) - 1, step)))


def test_fastq_equals_the_model_for_any_thread_count(dev, tmp_path):
    """70,000 records: more than two of the reader's 32,768-record blocks."""
    k, B, n = 21, 65, 70_000
    base = ri.base_reads(k)
    seq, qual, off = ri.tiled(*base, n)
    single = str(tmp_path / "reads.fq")
    _write_fastq(single, seq, qual, off, 0, 1)
    em = histogram(dev, base, k)  # (every interval of the file is one of the read set's)
    contents = [c for _, c in em.rows()]
    exp, _ = bem.mult(bi.base_multi(k, False), contents, SEED, B, n_total=n)
    for threads in (1, 4):
        counts, w, mult, missed = dev.bootstrap_em_fastq(em, single, None, k=k, replicates=B, seed=SEED,
                                                         phred_cutoff=ri.CUTOFF, local=True, threads=threads)
        np.testing.assert_array_equal(mult, exp)
        assert missed == 0
        assert_counts((counts, w), base_units(k, False), B, True, k, n_total=n)
    p1, p2 = str(tmp_path / "reads_1.fq"), str(tmp_path / "reads_2.fq")
    _write_fastq(p1, seq, qual, off, 0, 2)
    _write_fastq(p2, seq, qual, off, 1, 2)
    exp, _ = bem.mult(bi.base_multi(k, True), contents, SEED, B, n_total=n // 2)
    for threads in (1, 4):
        counts, w, mult, missed = dev.bootstrap_em_fastq(em, p1, p2, k=k, replicates=B, seed=SEED,
                                                         phred_cutoff=ri.CUTOFF, threads=threads)
        np.testing.assert_array_equal(mult, exp)
        assert missed == 0 and w is None
        assert_counts((counts, w), base_units(k, True), B, False, k, n_total=n // 2)
    em.close()


def test_row_0_refined_is_the_runs_own_loop_bit_for_bit(dev):
    """Global mode: em_rows_refine of the bootstrap's row 0 against em_refine over EmHistogram.step, the loop of the
    CLI and of the tests of `speq scan`'s refinement."""
    k, B = 21, 8
    reads = ri.base_reads(k)
    em = histogram(dev, reads, k)
    (counts, _), (mult, _), _, _ = run(dev, em, k, reads, B, False, False)
    u_ref, tot_ref = dev.count_unique_kmers_per_group(k)
    group_counts = [1, 2, 1]
    scale = 1.0 / 0.99 ** k
    row_mult, ptr, grp, cnt = em.rows_csr()
    assert row_mult.tolist() == mult[0].tolist()
    got_p, got_it = em_rows_refine(3, ptr, grp, cnt, mult, counts, None, u_ref, tot_ref, group_counts, scale, 1e-6, 1000)
    ut = (counts[0, 2:].astype(np.float64) * np.float64(scale)).tolist()
    p0 = unique_to_percent(ut, int(counts[0, 0]), u_ref.astype(np.float64), tot_ref.astype(np.float64))
    its = em_refine(lambda p: em.step(p, group_counts, counts[0, 2:]), ut, int(counts[0, 0]), p0, 1e-6, 1000)
    assert len(its) == got_it[0] >= 2 and its[-1][0] == got_p[0].tolist()
    assert (got_p[1:] != got_p[0]).any() and (got_it > 0).all()
    em.close()


@pytest.mark.parametrize("name,accuracy", [("tiny_single", None), ("tiny_paired", "0.99")])
def test_cli_bootstrap_em_file(name, accuracy, tmp_path):
    """`speq all --bootstrap-em FILE`: stdout, stderr, -o and a --bootstrap file are byte-identical to a run without
    the option; FILE is the model's table (every replicate refined by the model's exact step), each number within 1e-6,
    the print precision, of the model's; the percent column is -o's vector."""
    c = Case(name)
    k = c.ks[0]
    local = accuracy is None
    outs = {}
    for tag in ("plain", "em"):
        d = tmp_path / tag
        d.mkdir()
        for f in os.listdir(c.dir):
            shutil.copy(os.path.join(c.dir, f), d / f)
        args = ["all", "-r", "refs.fa", "-g", "groups.txt", "-1", "reads_1.fq"]
        if c.paired:
            args += ["-2", "reads_2.fq"]
        args += ["-x", "ref", "-k", str(k), "--phred-cutoff", str(c.cutoff), "--prefix-q", "4", "-o", "p.txt",
                 "--bootstrap", "ci.tsv", "--bootstrap-replicates", "64", "--bootstrap-seed", "7"]
        if accuracy:
            args += ["--fixed-accuracy", accuracy]
        if tag == "em":
            args += ["--bootstrap-em", "ci_em.tsv"]
        r = subprocess.run([SPEQ] + args, cwd=d, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        outs[tag] = (r.stderr, r.stdout, (d / "p.txt").read_bytes(), (d / "ci.tsv").read_bytes())
    assert outs["plain"] == outs["em"]
    assert not (tmp_path / "plain" / "ci_em.tsv").exists()
    # the model
    index = er.build_index(c.records, c.groups, c.G, k)
    un = bm.units(index, c.G, k, c.seq, c.qual, c.offsets, c.cutoff, c.paired, local)
    counts, w = bm.replicates(un, 7, 64)
    mu = bem.multi_units(index, c.G, k, c.seq, c.qual, c.offsets, c.cutoff, c.paired)
    contents = sorted(mu.hist.merged)
    M, _ = bem.mult(mu, contents, 7, 64)
    u_ref, tot_ref = Oracle(c.records, c.groups, c.G, k).ref_unique()
    gm = file_to_map(os.path.join(c.dir, "groups.txt"))
    scale = 1.0 if local else 1.0 / float(accuracy) ** k
    percent = np.array([bem.refine_row(contents, M[b], counts[b], None if w is None else w[b], u_ref, tot_ref,
                                       gm.counts, scale, 1e-6, 1000)[0] for b in range(65)])
    written = [ln.split("\t") for ln in (tmp_path / "em" / "p.txt").read_text().splitlines()]
    assert [f[0] for f in written] == gm.names
    cis = bootstrap_summary_percent(percent, counts[:, 0] != 0)
    got = (tmp_path / "em" / "ci_em.tsv").read_text().splitlines(keepends=True)
    assert got[0] == bm.HEADER and len(got) == c.G + 1
    assert any(ci["se"] > 0 for ci in cis)
    for line, nm, ci, out in zip(got[1:], gm.names, cis, written):
        f = line.rstrip("\n").split("\t")
        assert len(f) == 7 and f[0] == nm and int(f[6]) == ci["used"] == 64
        assert "%g" % float(f[1]) == out[1]  # -o prints 6 significant digits
        for text, key in zip(f[1:6], ("estimate", "mean", "se", "lo", "hi")):
            assert len(text.split(".")[1]) == 6 and abs(float(text) - ci[key]) <= 1e-6, (nm, key, text, ci[key])
