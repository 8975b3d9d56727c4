"""GPU: the marker track (speq_markers_track*, `speq --marker-track`) against the exact pure-Python model
(tests/marker_track_model.py; its own hand-worked cases are in tests/test_marker_track_cpu.py).

Everything is integers, so every comparison is exact: every case compares first_bin and every field of every bin of
every record with the model. The kernel has two fold paths, named in the test ids: `narrow` (bin < 64, one set of
atomics per marker lane) and `wide` (bin >= 64, a wave reduction per touched bin)."""
import os
import shutil
import subprocess
from functools import lru_cache

import numpy as np
import pytest

import em_reference as er
import marker_model as mm
import marker_track_model as tm
import read_report_inputs as ri
from golden_io import CASES, Case
from speq_amd import DeviceIndex, FmIndex, Markers, MarkerTrack, file_to_map

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEQ = os.path.join(ROOT, "bin", "speq")

FULL = dict(pair_steps=True, triple_steps=True, label_table=True)
VARIANTS = {  # those of tests/test_gpu_markers.py: every search step form, label table and run bitvector
    "no_qmer_table": dict(prefix_q=0, pair_steps=False, triple_steps=False, label_table=False),
    "single_steps": dict(prefix_q=8, pair_steps=False, triple_steps=False, label_table=False),
    "pairs": dict(prefix_q=8, pair_steps=True, triple_steps=False, label_table=False),
    "pairs_label": dict(prefix_q=8, pair_steps=True, triple_steps=False, label_table=True),
    "triples_no_label": dict(prefix_q=8, pair_steps=True, triple_steps=True, label_table=False),
}
BINS = [1, 7, 64, 100, 4096]


def path_of(bin: int) -> str:
    return "wide" if bin >= 64 else "narrow"


BIN_IDS = [f"{path_of(b)}-{b}" for b in BINS]


# ---- comparison ----
def assert_track(got: MarkerTrack, exp: tm.Track):
    assert got.bin == exp.bin and got.k == exp.k
    np.testing.assert_array_equal(got.first_bin, exp.first_bin)
    assert got.first_bin.dtype == np.uint64 and got.bins.dtype == tm.DTYPE
    assert got.loci.tolist() == exp.loci
    for f in tm.DTYPE.names:
        np.testing.assert_array_equal(got.bins[f], exp.bins[f], err_msg=f)


def check(records, groups, G, k, reads, bins=(7, 100), cutoff=ri.CUTOFF, opts=None, dev=None):
    """Adds the reads to a fresh handle and compares the track at every bin width with the model; returns
    (model coverage, {bin: model track})."""
    own = dev is None
    if own:
        idx = FmIndex.build(records, groups, G, **(opts or dict(prefix_q=4, **FULL)))
        dev = DeviceIndex(idx)
    cov = mm.coverage(er.build_index(records, groups, G, k), G, k, *reads, cutoff)
    m = Markers(dev, k, cutoff)
    m.add(*reads)
    exp = {}
    for bin in bins:
        exp[bin] = tm.track(records, groups, k, cov, bin)
        assert_track(m.track(bin), exp[bin])
    m.close()
    if own:
        dev.close()
    return cov, exp


def _dna(rng, n: int) -> bytes:
    return bytes(b"ACGT"[c] for c in rng.integers(0, 4, n))


def _reads_of(seqs):
    return ri.pack(seqs, [bytes([ri.GOOD]) * len(s) for s in seqs])


def _sample(rng, records, k: int, n: int, strands=(0, 1)):
    """n substrings of the records, k .. k + 150 bases, from the given strands."""
    out = []
    pool = [r for r in records if len(r) >= k]
    for _ in range(n):
        rec = pool[int(rng.integers(len(pool)))]
        L = min(len(rec), k + int(rng.integers(0, 151)))
        a = int(rng.integers(0, len(rec) - L + 1))
        s = rec[a:a + L]
        out.append(er.revcomp(s) if strands[int(rng.integers(len(strands)))] else s)
    return out


# ---- tile and bin edges ----
EDGE_K = 21
EDGE_NWIN = [1, 63, 64, 65, 128, 129]


@lru_cache(maxsize=None)
def edge_case():
    """Records of 1, 63, 64, 65, 128 and 129 loci and one shorter than k, in three groups; the record of 129 loci holds
    40 bases of the one of 128 (another group), so some of its loci are no markers. Reads from both strands cover
    parts of every record, and one read runs over a record's last window."""
    rng = np.random.default_rng(101)
    records = [_dna(rng, n + EDGE_K - 1) for n in EDGE_NWIN] + [_dna(rng, EDGE_K - 1)]
    last = bytearray(records[5])
    last[50:90] = records[4][30:70]
    records[5] = bytes(last)
    groups = [0, 1, 2, 0, 1, 2, 0]
    seqs = []
    for rec in records[:6]:
        seqs += [rec[:EDGE_K + 40], er.revcomp(rec[len(rec) // 2:]), rec[-EDGE_K:], rec]
    seqs += _sample(rng, records, EDGE_K, 30)
    reads = _reads_of(seqs)
    cov = mm.coverage(er.build_index(records, groups, 3, EDGE_K), 3, EDGE_K, *reads, ri.CUTOFF)
    return records, groups, reads, cov


@pytest.fixture(scope="module")
def edge_dev():
    records, groups, _, _ = edge_case()
    dev = DeviceIndex(FmIndex.build(records, groups, 3, prefix_q=4, **FULL))
    yield dev
    dev.close()


@pytest.mark.parametrize("bin", BINS, ids=BIN_IDS)
def test_tile_and_bin_edges(bin, edge_dev):
    records, groups, reads, cov = edge_case()
    assert tm.loci_of(records, EDGE_K) == EDGE_NWIN + [0]
    exp = tm.track(records, groups, EDGE_K, cov, bin)
    m = Markers(edge_dev, EDGE_K, ri.CUTOFF)
    m.add(*reads)
    got = m.track(bin)
    assert_track(got, exp)
    m.close()
    n_bins = [len(got.record(r)) for r in range(7)]
    assert n_bins == [-(-n // bin) for n in EDGE_NWIN] + [0]
    assert [got.end(r, n_bins[r] - 1) for r in range(6)] == EDGE_NWIN and got.start(5, n_bins[5] - 1) == (n_bins[5] - 1) * bin
    if bin == 7:  # a bin boundary inside a tile; the last bin of 129 loci holds 3
        assert got.end(5, 18) - got.start(5, 18) == 3
    if bin == 4096:
        assert n_bins[:6] == [1] * 6
    # the shared stretch of the last record carries no markers, the rest of it does
    one = tm.track(records, groups, EDGE_K, cov, 1).record(5)["markers"]
    assert one[50:70].tolist() == [0] * 20 and one[:29].all() and int(exp.bins["hits"].sum()) > 0
    with np.errstate(all="ignore"):
        b = got.breadth()
    assert np.isnan(b[got.bins["markers"] == 0]).all() and (b[got.bins["markers"] > 0] <= 1.0).all()


# ---- k: every search path, self-reverse-complement k-mers ----
KS = sorted(set([1, 4, 21, 31, 70, 200] + ri.KS))


@lru_cache(maxsize=None)
def k_case():
    """Three groups of one 2,400-base record each, variants of one sequence with a substitution every 97 (131, 173)
    bases, and a one-group collection of one 700-base record, where every k-mer is a marker for any k."""
    rng = np.random.default_rng(103)
    base = _dna(rng, 2400)
    records = []
    for step in (97, 131, 173):
        s = bytearray(base)
        for p in range(step // 2, len(s), step):
            s[p] = b"ACGT"[(b"ACGT".index(s[p]) + 1) % 4]
        records.append(bytes(s))
    return records, [0, 1, 2], [_dna(rng, 700)], [0]


@pytest.fixture(scope="module")
def k_devs():
    r3, g3, r1, g1 = k_case()
    devs = (DeviceIndex(FmIndex.build(r3, g3, 3, prefix_q=8, **FULL)), DeviceIndex(FmIndex.build(r1, g1, 1, prefix_q=8, **FULL)))
    yield devs
    for d in devs:
        d.close()


@pytest.mark.parametrize("k", KS)
def test_every_k(k, k_devs):
    r3, g3, r1, g1 = k_case()
    rng = np.random.default_rng(1000 + k)
    n_self = 0
    for records, groups, G, dev in ((r3, g3, 3, k_devs[0]), (r1, g1, 1, k_devs[1])):
        if max(len(r) for r in records) < k:
            seqs = [records[0]]
        else:
            seqs = _sample(rng, records, k, 24)
        seq, qual, off = _reads_of(seqs)
        q = bytearray(qual)
        s = bytearray(seq)
        for p in rng.integers(0, len(s), 6).tolist():  # a few bad positions: the scan's filter
            q[p] = 33 + ri.CUTOFF
        s[int(rng.integers(0, len(s)))] = ord("N")
        cov, exp = check(records, groups, G, k, (bytes(s), bytes(q), off), bins=(7, 100), dev=dev)
        n_self += sum(1 for w in cov.group_of if er.revcomp(w) == w and cov.depth.get(w, 0))
        if G == 1 and k <= 200:
            assert int(exp[100].bins["markers"].sum()) == 700 - k + 1 and int(exp[100].bins["hits"].sum()) > 0
    if k == 4:
        assert n_self > 0, "covered self-reverse-complement markers"


# ---- strands ----
def test_strands_and_a_planted_self_reverse_complement_marker():
    rng = np.random.default_rng(107)
    k, pal = 6, b"GAATTC"
    assert er.revcomp(pal) == pal
    a, other = _dna(rng, 40) + pal + _dna(rng, 40), _dna(rng, 300)
    while a.count(pal) != 1 or pal in other or pal in er.revcomp(other):
        a, other = _dna(rng, 40) + pal + _dna(rng, 40), _dna(rng, 300)
    records, groups = [a, other], [0, 1]
    fwd = [a[30:60], a[38:50], pal, a[:20], other[10:80], other[200:290]]
    rc = [er.revcomp(s) for s in fwd]
    dev = DeviceIndex(FmIndex.build(records, groups, 2, prefix_q=3, **FULL))
    tracks = {}
    for name, seqs in (("fwd", fwd), ("rc", rc), ("both", fwd + rc)):
        cov, exp = check(records, groups, 2, k, _reads_of(seqs), bins=(1, 64), dev=dev)
        tracks[name] = exp
        # the planted k-mer is one marker whose depth is counted once at its locus
        n = 3 * (2 if name == "both" else 1)
        assert cov.marker_depths()[pal] == (0, n)
        assert tuple(exp[1].record(0)[40]) == (1, 1, n, n)
    for bin in (1, 64):
        for f in tm.DTYPE.names:
            np.testing.assert_array_equal(tracks["fwd"][bin].bins[f], tracks["rc"][bin].bins[f])
        np.testing.assert_array_equal(tracks["both"][bin].bins["hits"], 2 * tracks["fwd"][bin].bins["hits"])
    dev.close()


# ---- bad positions ----
def test_n_near_bin_edges_and_record_ends():
    """k = 21, bin = 100 (and 7): N at a bin's last and first locus, k - 1 before a bin edge (the last window over it
    is the bin's last locus), inside the first and the last window of a record, and a record ending in N."""
    rng = np.random.default_rng(109)
    k = 21
    a, b, c = bytearray(_dna(rng, 420)), bytearray(_dna(rng, 330)), bytearray(_dna(rng, 150))
    for p in (99, 100, 200 - k + 1, 200 + k - 1, 3, 420 - 5):
        a[p] = ord("N")
    for p in (0, 329, 180):
        b[p] = ord("N")
    records, groups = [bytes(a), bytes(b), bytes(c)], [0, 1, 1]
    clean = [bytes(x).replace(b"N", b"A") for x in (a, b)]
    seqs = [records[0], er.revcomp(records[1]), records[2], clean[0][50:260], er.revcomp(clean[0][150:300]), clean[1]]
    cov, exp = check(records, groups, 2, k, _reads_of(seqs), bins=(1, 7, 100))
    one = exp[1].record(0)["markers"].tolist()
    assert one[99 - k + 1:101] == [0] * (k + 1) and one[98 - k + 1] == 1 and one[101] == 1
    assert one[:4] == [0] * 4 and one[-1] == 0 and sum(one) > 200
    assert exp[100].record(1)["markers"].tolist()[0] == 99 and int(exp[100].bins["hits"].sum()) > 0


# ---- index variants and group counts ----
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_index_variants(variant):
    r3, g3, _, _ = k_case()
    rng = np.random.default_rng(113)
    for k in (8, 21, 70):
        check(r3, g3, 3, k, _reads_of(_sample(rng, r3, k, 16)), bins=(7, 100), opts=VARIANTS[variant])


def test_one_group():
    rng = np.random.default_rng(127)
    rec, k = _dna(rng, 500), 15
    reads = _reads_of([rec[:120], rec[60:200], er.revcomp(rec[300:420]), _dna(rng, 100)])
    cov, exp = check([rec], [0], 1, k, reads, bins=(1, 100))
    assert int(exp[100].bins["markers"].sum()) == 500 - k + 1 and exp[100].group_hits([0], 1) == cov.hits


def test_70_groups():
    records, groups = ri.many_ref()
    cov, exp = check(records, groups, 70, ri.MANY_K, ri.many_reads(), bins=(7, 100), opts=dict(prefix_q=6, **FULL))
    assert exp[100].bins["markers"].tolist() == [100, 100, 80] * 70
    assert exp[100].group_hits(groups, 70) == cov.hits


@pytest.mark.parametrize("label", [False, True], ids=["runs", "label_table"])
def test_600_groups(label):
    rng = np.random.default_rng(53)
    k, G = 11, 600
    records, groups = [_dna(rng, 40) for _ in range(G)], list(range(G))
    reads = _reads_of([records[g] for g in (0, 1, 255, 256, 511, G - 1)] + [er.revcomp(records[7])] * 9 +
                      [records[3][:20] + records[G - 2][20:]])
    cov, exp = check(records, groups, G, k, reads, bins=(7, 64),
                     opts=dict(prefix_q=4, pair_steps=True, triple_steps=label, label_table=label))
    assert int(exp[64].record(7)["max_depth"][0]) == 9 and len(exp[64].bins) == G and len(exp[7].bins) == 5 * G


# ---- repeats ----
def test_repeats_give_every_locus_the_full_depth():
    rng = np.random.default_rng(131)
    a, b, k = _dna(rng, 300), _dna(rng, 300), 21
    rep = a + a[100:160]  # 40 k-mers of the record lie at two loci each
    records, groups = [a, a, b, rep], [0, 0, 1, 0]
    reads = _reads_of([a[:100], a[50:200], er.revcomp(a[100:180]), b[:90], rep[280:], er.revcomp(rep[290:350])])
    cov, exp = check(records, groups, 2, k, reads, bins=(1, 100))
    t = exp[1]
    for f in tm.DTYPE.names:
        np.testing.assert_array_equal(t.record(0)[f], t.record(1)[f])
        np.testing.assert_array_equal(t.record(0)[f][:280], t.record(3)[f][:280])
    np.testing.assert_array_equal(t.record(3)["hits"][100:140], t.record(3)["hits"][300:340])
    assert t.record(3)["hits"][300:340].min() >= 3
    sums = exp[100].group_hits(groups, 2)
    assert sums[0] > cov.hits[0] and sums[1] == cov.hits[1] > 0


# ---- the handle ----
def _records_of(cov) -> np.ndarray:
    return np.concatenate([np.stack([cov.markers, cov.observed, cov.hits, cov.max_depth], axis=1), cov.depth_hist], axis=1)


def test_handle_adds_finalize_and_repeated_tracks(edge_dev):
    records, groups, reads, cov_all = edge_case()
    seq, qual, off = reads
    n = len(off) - 1
    half = n // 2
    cut = int(off[half])
    first = (seq[:cut], qual[:cut], off[:half + 1])
    second = (seq[cut:], qual[cut:], off[half:] - off[half])
    cov_first = mm.coverage(er.build_index(records, groups, 3, EDGE_K), 3, EDGE_K, *first, ri.CUTOFF)
    m = Markers(edge_dev, EDGE_K, ri.CUTOFF)
    m.add(*first)
    before = _records_of(m.finalize())
    t1 = m.track(100)
    t2 = m.track(100)
    t7 = m.track(7)
    after = _records_of(m.finalize())
    np.testing.assert_array_equal(before, after)
    np.testing.assert_array_equal(before, cov_first.records())
    assert_track(t1, tm.track(records, groups, EDGE_K, cov_first, 100))
    assert_track(t7, tm.track(records, groups, EDGE_K, cov_first, 7))
    assert t1.bins.tobytes() == t2.bins.tobytes()
    m.add(*second)
    assert_track(m.track(100), tm.track(records, groups, EDGE_K, cov_all, 100))
    assert_track(m.track(1), tm.track(records, groups, EDGE_K, cov_all, 1))
    np.testing.assert_array_equal(_records_of(m.finalize()), cov_all.records())
    lo, grp, dep = m.list()
    assert int(dep.astype(np.int64).sum()) == sum(cov_all.hits)  # the depths themselves are as the adds left them
    m.close()


# ---- files and the CLI ----
@lru_cache(maxsize=None)
def golden_model(name: str, k: int, bin: int):
    c = Case(name)
    return tm.model(c.records, c.groups, c.G, k, (c.seq, c.qual, c.offsets), bin, c.cutoff)


@pytest.mark.parametrize("name", CASES)
def test_marker_track_fastq_equals_the_host_arrays(name):
    c = Case(name)
    idx = FmIndex.build(c.records, c.groups, c.G, prefix_q=4, **FULL)
    dev = DeviceIndex(idx)
    p1 = os.path.join(c.dir, "reads_1.fq")
    p2 = os.path.join(c.dir, "reads_2.fq") if c.paired else None
    k = c.ks[0]
    for bin in (7, 100):
        cov_exp, exp = golden_model(name, k, bin)
        m = Markers(dev, k, c.cutoff)
        m.add(c.seq, c.qual, c.offsets)
        host = m.track(bin)
        m.close()
        cov, got = dev.marker_track_fastq(p1, p2, k=k, phred_cutoff=c.cutoff, bin=bin, threads=3)
        assert_track(host, exp)
        assert_track(got, exp)
        np.testing.assert_array_equal(_records_of(cov), cov_exp.records())
        np.testing.assert_array_equal(_records_of(cov),
                                      _records_of(dev.marker_coverage_fastq(p1, p2, k=k, phred_cutoff=c.cutoff)))
    dev.close()


@pytest.mark.parametrize("name", CASES)
def test_cli_marker_track_file(name, tmp_path):
    """`speq all --marker-track FILE --track-bin 50`: stderr, stdout, -o and the --marker-coverage file are
    byte-identical to a run without the option; FILE's integer columns and names equal the model's lines byte for byte,
    and its two ratio columns parse to within 1.5e-6 of the model's (one unit of the last printed digit)."""
    c = Case(name)
    k, bin = c.ks[0], 50
    outs = {}
    for tag in ("plain", "track", "track_only"):
        d = tmp_path / tag
        d.mkdir()
        for f in os.listdir(c.dir):
            shutil.copy(os.path.join(c.dir, f), d / f)
        args = ["all", "-r", "refs.fa", "-g", "groups.txt", "-1", "reads_1.fq"]
        if c.paired:
            args += ["-2", "reads_2.fq"]
        args += ["-x", "ref", "-k", str(k), "--phred-cutoff", str(c.cutoff), "--prefix-q", "4", "-o", "p.txt"]
        if tag != "track_only":
            args += ["--marker-coverage", "cov.tsv"]
        if tag != "plain":
            args += ["--marker-track", "track.tsv", "--track-bin", str(bin)]
        r = subprocess.run([SPEQ] + args, cwd=d, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        outs[tag] = (r.stderr, r.stdout, (d / "p.txt").read_bytes())
    assert outs["plain"] == outs["track"] == outs["track_only"]
    assert (tmp_path / "plain" / "cov.tsv").read_bytes() == (tmp_path / "track" / "cov.tsv").read_bytes()
    assert not (tmp_path / "plain" / "track.tsv").exists() and not (tmp_path / "track_only" / "cov.tsv").exists()
    names = file_to_map(os.path.join(c.dir, "groups.txt")).names
    _, exp = golden_model(name, k, bin)
    want = [tm.HEADER] + exp.tsv_lines(c.groups, names)
    got = (tmp_path / "track" / "track.tsv").read_text().splitlines(keepends=True)
    assert got == (tmp_path / "track_only" / "track.tsv").read_text().splitlines(keepends=True)
    assert got[0] == want[0] and len(got) == len(want) == len(exp.bins) + 1 > 1
    ratio_cols = (6, 8)
    for gl, wl in zip(got[1:], want[1:]):
        gf, wf = gl.rstrip("\n").split("\t"), wl.rstrip("\n").split("\t")
        assert len(gf) == len(wf) == 10
        assert [x for i, x in enumerate(gf) if i not in ratio_cols] == [x for i, x in enumerate(wf) if i not in ratio_cols]
        for i in ratio_cols:
            if wf[i] == "-":
                assert gf[i] == "-"
            else:
                assert len(gf[i].split(".")[1]) == 6 and abs(float(gf[i]) - float(wf[i])) <= 1.5e-6


# ---- the use case ----
def test_a_recombinant_shows_in_the_track():
    """Two groups A and B of one 600-base record; B is A with a substitution about every 50 bases, so at k = 21 a
    k-mer over a substitution is a marker and one between two substitutions is shared. Reads: every 100-base substring
    of A[0:300] and of the reverse complement of B[300:600]. A marker of A cannot occur in a read of B, so A's bins 0
    and 1 (loci 0..199, every window inside A[0:300]) are fully covered and its bins 4 and 5 not at all; B mirrors."""
    rng = np.random.default_rng(137)
    k, bin = 21, 100
    a = _dna(rng, 600)
    s = bytearray(a)
    for p in range(25, 600, 50):
        s[p] = b"ACGT"[(b"ACGT".index(s[p]) + 1 + int(rng.integers(3))) % 4]
    b = bytes(s)
    records, groups = [a, b], [0, 1]
    rcb = er.revcomp(b[300:600])
    seqs = [a[i:i + 100] for i in range(201)] + [rcb[i:i + 100] for i in range(201)]
    cov, exp = check(records, groups, 2, k, _reads_of(seqs), bins=(bin, 7))
    ta, tb = exp[bin].record(0), exp[bin].record(1)
    assert len(ta) == len(tb) == 6 and (ta["markers"] > 0).all() and ta["markers"].tolist() == tb["markers"].tolist()
    assert ta["observed"][:2].tolist() == ta["markers"][:2].tolist() and ta["observed"][4:].tolist() == [0, 0]
    assert tb["observed"][4:].tolist() == tb["markers"][4:].tolist() and tb["observed"][:2].tolist() == [0, 0]
    # the same on the device's own answer, through the public helpers
    dev = DeviceIndex(FmIndex.build(records, groups, 2, prefix_q=4, **FULL))
    m = Markers(dev, k)
    m.add(*_reads_of(seqs))
    got = m.track(bin)
    br = got.breadth()
    assert br[:2].tolist() == [1.0, 1.0] and br[4:6].tolist() == [0.0, 0.0]
    assert br[6:8].tolist() == [0.0, 0.0] and br[10:12].tolist() == [1.0, 1.0]
    assert (got.mean_depth()[:2] > 1.0).all() and got.start(1, 5) == 500 and got.end(1, 5) == 580
    # coverage per group cannot tell this from half coverage of both
    assert 0 < m.finalize().breadth[0] < 1
    m.close()
    dev.close()
