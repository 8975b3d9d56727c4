"""GPU: marker coverage (speq_markers_*, `speq --marker-coverage`) against the exact pure-Python model
(tests/marker_model.py; validated against the C oracle by tests/test_marker_model_cpu.py).

Everything is integers, so every comparison is exact. Each case compares finalize() with the model's per-group
records, and list() with the model's markers one by one: every listed SA position is mapped to its k-mer through the
host suffix array and text, the set of listed k-mers must be the model's marker set, and every group and depth must be
equal. Inputs: tests/read_report_inputs.py (search paths, tile edges, the read filter), tests/frag_refs.py (texts
shorter than k, empty, with N; collections below one occ block), hand-made references (duplicate records, a k-mer equal
to its reverse complement, one group, 70 groups, more groups than the fold's LDS tally takes), and the golden FASTQ
cases, plain and gzip, through the library and the CLI."""
import gzip
import os
import shutil
import subprocess
from functools import lru_cache

import numpy as np
import pytest

import em_reference as er
import frag_refs as fr
import marker_model as mm
import read_report_inputs as ri
from golden_io import CASES, Case
from speq_amd import DeviceIndex, FmIndex, Markers, file_to_map

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEQ = os.path.join(ROOT, "bin", "speq")

FULL = dict(pair_steps=True, triple_steps=True, label_table=True)
VARIANTS = {
    "no_qmer_table": dict(prefix_q=0, pair_steps=False, triple_steps=False, label_table=False),
    "single_steps": dict(prefix_q=8, pair_steps=False, triple_steps=False, label_table=False),
    "pairs": dict(prefix_q=8, pair_steps=True, triple_steps=False, label_table=False),
    "pairs_label": dict(prefix_q=8, pair_steps=True, triple_steps=False, label_table=True),
    "triples_no_label": dict(prefix_q=8, pair_steps=True, triple_steps=True, label_table=False),
}
_ACGT = np.zeros(256, dtype=np.uint8)
_ACGT[2:6] = np.frombuffer(b"ACGT", dtype=np.uint8)  # SA-alphabet codes A..T = 2..5; anything else decodes to 0


# ---- comparison ----
def listed_kmers(idx: FmIndex, lo: np.ndarray, k: int) -> list:
    """The k-mer at each SA position: text[sa[lo] : sa[lo] + k] decoded (a window that left the text or met a
    separator would hold a zero byte and match no marker of the model)."""
    sa = idx.array("sa", np.int32).astype(np.int64)
    text = idx.array("text", np.uint8)
    at = sa[lo.astype(np.int64)][:, None] + np.arange(k, dtype=np.int64)[None, :]
    codes = np.where(at < len(text), text[np.minimum(at, len(text) - 1)], 0)
    rows = _ACGT[codes]
    return [r.tobytes() for r in rows]


def _records_of(cov) -> np.ndarray:
    """A MarkerCoverage as [G, 12], the model's layout."""
    return np.concatenate([np.stack([cov.markers, cov.observed, cov.hits, cov.max_depth], axis=1), cov.depth_hist], axis=1)


def assert_equal(m: Markers, idx: FmIndex, k: int, exp: mm.Coverage):
    cov = m.finalize()
    got = _records_of(cov)
    np.testing.assert_array_equal(got, exp.records())
    assert got.dtype == np.uint64 and cov.depth_hist.shape == (exp.G, mm.BINS)
    lo, grp, dep = m.list()
    assert len(lo) == len(exp.group_of)
    assert (np.diff(lo.astype(np.int64)) > 0).all(), "ascending SA positions, each once"
    kmers = listed_kmers(idx, lo, k)
    assert dict(zip(kmers, zip(grp.tolist(), dep.tolist()))) == exp.marker_depths()
    return cov


def run(idx: FmIndex, k: int, reads, exp: mm.Coverage, cutoff: int = ri.CUTOFF, dev: DeviceIndex = None):
    own = dev is None
    dev = dev or DeviceIndex(idx)
    m = Markers(dev, k, cutoff)
    m.add(*reads)
    cov = assert_equal(m, idx, k, exp)
    m.close()
    if own:
        dev.close()
    return cov


# ---- the base input: every search path and the read filter ----
@lru_cache(maxsize=None)
def base_index(variant: str = "full") -> FmIndex:
    ref = ri.base_ref()
    opts = dict(prefix_q=8, **FULL) if variant == "full" else VARIANTS[variant]
    return FmIndex.build(ref.records, ref.groups, 3, **opts)


@lru_cache(maxsize=None)
def base_model(k: int) -> mm.Coverage:
    ref = ri.base_ref()
    return mm.coverage(er.build_index(ref.records, ref.groups, 3, k), 3, k, *ri.base_reads(k), ri.CUTOFF)


# k below, at and above the q-mer table (q = 8), every (k - q) mod 3 leftover (9, 10, 11), one and many tiles
@pytest.mark.parametrize("k", [1, 9, 10, 11] + ri.KS)
def test_search_paths_and_agreement_with_scan_and_report(k):
    reads = ri.base_reads(k)
    dev = DeviceIndex(base_index())
    cov = run(base_index(), k, reads, base_model(k), dev=dev)
    if k == 21:
        assert (cov.max_depth >= 7).all() and (cov.depth_hist[:, 7] > 0).all()
    if k == 3:
        assert not cov.markers.any() and not cov.depth_hist.any()
    sc = dev.scan(*reads, k=k, phred_cutoff=ri.CUTOFF)
    assert cov.hits.tolist() == sc.unique.tolist()
    assert int(cov.hits.sum()) == int(dev.report(*reads, k=k, phred_cutoff=ri.CUTOFF).unique.sum())
    assert cov.hits.tolist() == dev.marker_coverage(*reads, k=k, phred_cutoff=ri.CUTOFF).hits.tolist()
    dev.close()


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_index_variants(variant):
    for k in (8, 21, 70):
        run(base_index(variant), k, ri.base_reads(k), base_model(k))


# ---- the marker pass: text ends, N, groups without a window ----
@pytest.mark.parametrize("k", [21, 70])
def test_fragmented_reference(k):
    f = fr.fragmented(k)
    lens = {len(r) for r in f.records}
    assert {0, 1, k - 1, k, 2 * k - 2} <= lens and any(b"N" in r for r in f.records)
    rd = fr.reads(k)
    exp = mm.coverage(er.build_index(f.records, f.groups, f.G, k), f.G, k, rd.seq, rd.qual, rd.offsets, ri.CUTOFF)
    assert exp.markers[4] == 0 and min(exp.markers[:4]) > 0
    idx = FmIndex.build(f.records, f.groups, f.G, prefix_q=8, **FULL)
    cov = run(idx, k, (rd.seq.tobytes(), rd.qual.tobytes(), rd.offsets), exp)
    assert cov.markers[4] == cov.hits[4] == cov.max_depth[4] == 0 and not cov.depth_hist[4].any()


@pytest.mark.parametrize("case", fr.TINY, ids=fr.TINY_IDS)
def test_tiny_collections(case):
    records, groups, G, k, rd = case
    exp = mm.coverage(er.build_index(records, groups, G, k), G, k, rd.seq, rd.qual, rd.offsets, ri.CUTOFF)
    for opts in (dict(prefix_q=0), dict(prefix_q=3, **FULL)):
        idx = FmIndex.build(records, groups, G, **opts)
        run(idx, k, (rd.seq.tobytes(), rd.qual.tobytes(), rd.offsets), exp)


def _dna(rng, n: int) -> bytes:
    return bytes(b"ACGT"[c] for c in rng.integers(0, 4, n))


def _reads_of(seqs):
    return ri.pack(seqs, [bytes([ri.GOOD]) * len(s) for s in seqs])


def test_identical_records_in_one_group_count_each_marker_once():
    rng = np.random.default_rng(41)
    a, b, k = _dna(rng, 300), _dna(rng, 300), 21
    records, groups = [a, a, b], [0, 0, 1]
    reads = _reads_of([a[:100], a[50:200], er.revcomp(a[100:180]), b[:90]])
    exp = mm.coverage(er.build_index(records, groups, 2, k), 2, k, *reads, ri.CUTOFF)
    idx = FmIndex.build(records, groups, 2, prefix_q=4, **FULL)
    dev = DeviceIndex(idx)
    cov = run(idx, k, reads, exp, dev=dev)
    u_ref, _ = dev.count_unique_kmers_per_group(k)
    assert cov.markers.tolist() == [2 * (300 - k + 1)] * 2
    assert u_ref[0] == 2 * cov.markers[0] and u_ref[0] > cov.markers[0] and u_ref[1] >= cov.markers[1]
    dev.close()


def test_a_kmer_equal_to_its_reverse_complement():
    rng = np.random.default_rng(43)
    k, pal = 6, b"GAATTC"
    assert er.revcomp(pal) == pal
    other = _dna(rng, 80)
    while pal in other or pal in er.revcomp(other):
        other = _dna(rng, 80)
    records, groups = [_dna(rng, 40) + pal + _dna(rng, 40), other], [0, 1]
    reads = _reads_of([records[0][30:60], records[0][38:50], pal, other[:30]])
    exp = mm.coverage(er.build_index(records, groups, 2, k), 2, k, *reads, ri.CUTOFF)
    assert exp.marker_depths()[pal][0] == 0 and exp.marker_depths()[pal][1] >= 3  # one marker: both strands are one k-mer
    idx = FmIndex.build(records, groups, 2, prefix_q=3, **FULL)
    run(idx, k, reads, exp)


# ---- groups ----
def test_one_group():
    rng = np.random.default_rng(47)
    rec, k = _dna(rng, 500), 15
    reads = _reads_of([rec[:120], rec[60:200], er.revcomp(rec[300:420]), _dna(rng, 100)])
    exp = mm.coverage(er.build_index([rec], [0], 1, k), 1, k, *reads, ri.CUTOFF)
    assert exp.markers[0] == len(er.build_index([rec], [0], 1, k))  # every k-mer of the texts is a marker
    run(FmIndex.build([rec], [0], 1, prefix_q=4, **FULL), k, reads, exp)


def test_70_groups():
    records, groups = ri.many_ref()
    reads = ri.many_reads()
    exp = mm.coverage(er.build_index(records, groups, 70, ri.MANY_K), 70, ri.MANY_K, *reads, ri.CUTOFF)
    idx = FmIndex.build(records, groups, 70, prefix_q=6, **FULL)
    cov = run(idx, ri.MANY_K, reads, exp)
    assert cov.markers.tolist() == [560] * 70
    assert np.flatnonzero(cov.hits).tolist() == [0, 1, 33, 63, 64, 65, 69]


@pytest.mark.parametrize("label", [False, True], ids=["runs", "label_table"])
def test_more_groups_than_the_lds_tally_takes(label):
    """600 groups of one 40-base record: the fold's device-atomic path (the LDS tally takes 512 groups); 512 groups of
    the same records run the LDS path at its limit."""
    rng = np.random.default_rng(53)
    k = 11
    all_records = [_dna(rng, 40) for _ in range(600)]
    for G in (600, 512):
        records, groups = all_records[:G], list(range(G))
        reads = _reads_of([records[g] for g in (0, 1, 255, 256, 511, G - 1)] + [er.revcomp(records[7])] * 9 +
                          [records[3][:20] + records[G - 2][20:]])
        exp = mm.coverage(er.build_index(records, groups, G, k), G, k, *reads, ri.CUTOFF)
        assert exp.max_depth[7] == 9 and exp.hits[G - 1] > 0 and min(exp.markers) > 0
        idx = FmIndex.build(records, groups, G, prefix_q=4, pair_steps=True, triple_steps=label, label_table=label)
        run(idx, k, reads, exp)


# ---- the feature's point ----
def test_copies_of_one_kmer_against_spread_reads():
    """4,096 copies of one read with a single private window, against 4,096 distinct private windows: the scan cannot
    tell them apart, the breadth can. (The copies also put the 64 lanes' adds of many waves on one address.)"""
    ref, k, n = ri.base_ref(), 21, 4096
    index = er.build_index(ref.records, ref.groups, 3, k)
    copies, spread = mm.two_samples([ref.records[1]], index, 1, k, n)
    dev = DeviceIndex(base_index())
    covs = []
    for reads in (copies, spread):
        exp = mm.coverage(index, 3, k, *reads, ri.CUTOFF)
        covs.append(run(base_index(), k, reads, exp, dev=dev))
    a, b = covs
    ua = dev.scan(*copies, k=k, phred_cutoff=ri.CUTOFF).unique.tolist()
    ub = dev.scan(*spread, k=k, phred_cutoff=ri.CUTOFF).unique.tolist()
    assert ua == ub == [0, n, 0] == a.hits.tolist() == b.hits.tolist()
    assert (a.observed[1], a.max_depth[1]) == (1, n) and (b.observed[1], b.max_depth[1]) == (n, 1)
    assert a.breadth[1] < 0.001 < 0.5 < b.expected_breadth[1] < b.breadth[1]
    assert a.expected_breadth[1] == b.expected_breadth[1]
    dev.close()


# ---- accumulation ----
def _split(reads, n0: int, n1: int):
    seq, qual, off = reads
    a, b = int(off[n0]), int(off[n1])
    return seq[a:b], qual[a:b], off[n0:n1 + 1] - off[n0]


def _to_device(reads):
    import torch
    seq, qual, off = reads
    return (torch.from_numpy(np.frombuffer(seq, np.uint8).copy()).cuda(),
            torch.from_numpy(np.frombuffer(qual, np.uint8).copy()).cuda(),
            torch.from_numpy(np.asarray(off).astype(np.int64)).cuda())


def test_host_add_across_a_batch_edge():
    """speq_markers_add_reads stages at most 2^20 records per batch: 2^20 + 3 reads of the base read set repeated end
    to end. The expected depths are the model's over the whole set times the whole repeats, plus the model's over the
    reads of the cut last repeat; the markers themselves do not change."""
    from collections import Counter
    k = 21
    n = (1 << 20) + 3
    reads = ri.base_reads(k)
    reps, rem = divmod(n, len(reads[2]) - 1)
    assert rem
    whole = base_model(k)
    ref = ri.base_ref()
    part = mm.coverage(er.build_index(ref.records, ref.groups, 3, k), 3, k, *_split(reads, 0, rem), ri.CUTOFF)
    exp = mm.Coverage(3, whole.group_of, Counter({w: reps * d for w, d in whole.depth.items()}) + part.depth)
    assert sum(exp.hits) == reps * sum(whole.hits) + sum(part.hits) and 0 < sum(part.hits) < sum(whole.hits)
    idx = base_index()
    dev = DeviceIndex(idx)
    m = Markers(dev, k, ri.CUTOFF)
    m.add(*ri.tiled(*reads, n))
    cov = assert_equal(m, idx, k, exp)
    assert cov.markers.tolist() == whole.markers
    m.close()
    dev.close()


def test_accumulation():
    import torch
    k = 21
    reads = ri.base_reads(k)
    n = len(reads[2]) - 1
    half = n // 2 + 1
    exp = base_model(k)
    idx = base_index()
    dev = DeviceIndex(idx)
    # two halves are the whole; no reads change nothing
    m = Markers(dev, k, ri.CUTOFF)
    m.add(*_split(reads, 0, half))
    m.add(b"", b"", np.zeros(1, dtype=np.uint64))
    m.add_device(0, 0, 0, 0)
    first = m.finalize()
    assert 0 < int(first.hits.sum()) < sum(exp.hits)
    m.add(*_split(reads, half, n))
    assert_equal(m, idx, k, exp)  # finalize, more adds, finalize
    # the same reads again: every depth doubles, no marker is newly seen
    m.add(*reads)
    twice = assert_equal(m, idx, k, exp.added(exp))
    assert twice.observed.tolist() == exp.observed and twice.hits.tolist() == [2 * h for h in exp.hits]
    assert twice.max_depth.tolist() == [2 * d for d in exp.max_depth]
    m.close()
    # device buffers: one stream, then the halves on two streams at once
    whole = _to_device(reads)
    parts = [_to_device(_split(reads, 0, half)), _to_device(_split(reads, half, n))]
    torch.cuda.synchronize()
    m1 = Markers(dev, k, ri.CUTOFF)
    m1.add_device(whole[0].data_ptr(), whole[1].data_ptr(), whole[2].data_ptr(), n)
    assert_equal(m1, idx, k, exp)
    m1.close()
    m2 = Markers(dev, k, ri.CUTOFF)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for (s, q, o), st in zip(parts, streams):
        m2.add_device(s.data_ptr(), q.data_ptr(), o.data_ptr(), len(o) - 1, stream=st.cuda_stream)
    assert_equal(m2, idx, k, exp)  # (finalize waits for every stream of the device)
    m2.close()
    dev.close()


# ---- files and the CLI ----
@lru_cache(maxsize=None)
def golden_model(name: str, k: int) -> mm.Coverage:
    c = Case(name)
    return mm.coverage(er.build_index(c.records, c.groups, c.G, k), c.G, k, c.seq, c.qual, c.offsets, c.cutoff)


@pytest.mark.parametrize("name", CASES)
def test_marker_coverage_fastq_equals_the_host_arrays(name, tmp_path):
    c = Case(name)
    idx = FmIndex.build(c.records, c.groups, c.G, prefix_q=4, **FULL)
    dev = DeviceIndex(idx)
    p1 = os.path.join(c.dir, "reads_1.fq")
    p2 = os.path.join(c.dir, "reads_2.fq") if c.paired else None
    k = c.ks[0]
    exp = golden_model(name, k)
    host = run(idx, k, (c.seq, c.qual, c.offsets), exp, cutoff=c.cutoff, dev=dev)
    got = dev.marker_coverage_fastq(p1, p2, k=k, phred_cutoff=c.cutoff, threads=3)
    np.testing.assert_array_equal(_records_of(got), exp.records())
    np.testing.assert_array_equal(_records_of(got), _records_of(host))
    sc, _ = dev.scan_fastq(p1, p2, k=k, phred_cutoff=c.cutoff)
    assert got.hits.tolist() == sc.unique.tolist()
    gz = []
    for p in (p1, p2):
        if p:
            gz.append(str(tmp_path / (os.path.basename(p) + ".gz")))
            with open(p, "rb") as f, gzip.open(gz[-1], "wb") as g:
                g.write(f.read())
    got_gz = dev.marker_coverage_fastq(gz[0], gz[1] if c.paired else None, k=k, phred_cutoff=c.cutoff, threads=2)
    np.testing.assert_array_equal(_records_of(got_gz), exp.records())
    dev.close()


@pytest.mark.parametrize("name", CASES)
def test_cli_marker_coverage_file(name, tmp_path):
    """`speq all --marker-coverage FILE`: stderr, stdout and -o are byte-identical to a run without the option; FILE's
    name and integer columns equal the model's lines byte for byte, and its three ratio columns parse to within 1.5e-6
    of the model's (one unit of the last printed digit, which a 1-ulp difference between two exp() can flip)."""
    c = Case(name)
    k = c.ks[0]
    outs = {}
    for tag in ("plain", "markers"):
        d = tmp_path / tag
        d.mkdir()
        for f in os.listdir(c.dir):
            shutil.copy(os.path.join(c.dir, f), d / f)
        args = ["all", "-r", "refs.fa", "-g", "groups.txt", "-1", "reads_1.fq"]
        if c.paired:
            args += ["-2", "reads_2.fq"]
        args += ["-x", "ref", "-k", str(k), "--phred-cutoff", str(c.cutoff), "--prefix-q", "4", "-o", "p.txt"]
        if tag == "markers":
            args += ["--marker-coverage", "cov.tsv"]
        r = subprocess.run([SPEQ] + args, cwd=d, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        outs[tag] = (r.stderr, r.stdout, (d / "p.txt").read_bytes())
    assert outs["plain"] == outs["markers"]
    assert not (tmp_path / "plain" / "cov.tsv").exists()
    names = file_to_map(os.path.join(c.dir, "groups.txt")).names
    want = [mm.HEADER] + golden_model(name, k).tsv_lines(names)
    got = (tmp_path / "markers" / "cov.tsv").read_text().splitlines(keepends=True)
    assert got[0] == want[0] and len(got) == len(want) == c.G + 1
    ratio_cols = (3, 5, 6)
    for gl, wl in zip(got[1:], want[1:]):
        gf, wf = gl.rstrip("\n").split("\t"), wl.rstrip("\n").split("\t")
        assert len(gf) == len(wf) == 16
        assert [x for i, x in enumerate(gf) if i not in ratio_cols] == [x for i, x in enumerate(wf) if i not in ratio_cols]
        for i in ratio_cols:
            if wf[i] == "-":
                assert gf[i] == "-"
            else:
                assert len(gf[i].split(".")[1]) == 6 and abs(float(gf[i]) - float(wf[i])) <= 1.5e-6
