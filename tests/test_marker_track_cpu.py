"""No GPU: the marker-track model (tests/marker_track_model.py) against hand-worked cases, the identity between the
track's sums and the coverage's hits, the host-only bin layout of the library, the header's new symbols and the CLI's
argument errors. tests/test_gpu_marker_track.py holds the library's track against this model."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import em_reference as er
import marker_model as mm
import marker_track_model as tm
import read_report_inputs as ri
from golden_io import Case
from speq_amd import FmIndex, SpeqError
from speq_amd._lib import ABI_VERSION, SIGNATURES, TRACK_MAX_BIN, MarkerBin, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEQ = os.path.join(ROOT, "bin", "speq")
HEADER = os.path.join(ROOT, "include", "speq_scan.h")


def _reads(seqs):
    return ri.pack(seqs, [bytes([ri.GOOD]) * len(s) for s in seqs])


def _rows(t: tm.Track, r: int) -> list:
    return [tuple(x) for x in t.record(r).tolist()]


# ---- hand-worked cases ----
def test_a_self_reverse_complement_kmer_is_counted_once():
    """ACGTA at k = 4: locus 0 is ACGT, its own reverse complement; locus 1 is CGTA, whose reverse complement is TACG.
    Three reads ACGT and two reads TACG: locus 0 has depth 3 (not 6), locus 1 has 0 + 2."""
    records, groups, k = [b"ACGTA"], [0], 4
    assert er.revcomp(b"ACGT") == b"ACGT" and er.revcomp(b"CGTA") == b"TACG"
    reads = _reads([b"ACGT"] * 3 + [b"TACG"] * 2)
    cov, t1 = tm.model(records, groups, 1, k, reads, 1)
    assert t1.first_bin.tolist() == [0, 2]
    assert _rows(t1, 0) == [(1, 1, 3, 3), (1, 1, 2, 2)]
    _, t2 = tm.model(records, groups, 1, k, reads, 2)
    assert _rows(t2, 0) == [(2, 2, 5, 3)]
    # three markers (ACGT, CGTA, TACG), every one at one locus: the sums agree
    assert cov.markers == [3] and cov.hits == [5] == t2.group_hits(groups, 1)


def test_a_tandem_repeat_gives_every_locus_the_full_depth():
    """ACACACA at k = 3: ACA at loci 0, 2, 4 and CAC at 1, 3. One read ACA and two reads GTG (= rc(CAC))."""
    records, groups, k = [b"ACACACA"], [0], 3
    reads = _reads([b"ACA", b"GTG", b"GTG"])
    cov, t = tm.model(records, groups, 1, k, reads, 2)
    assert tm.locus_depths(records, groups, k, cov) == [[1, 2, 1, 2, 1]]
    assert t.first_bin.tolist() == [0, 3]
    assert _rows(t, 0) == [(2, 2, 3, 2), (2, 2, 3, 2), (1, 1, 1, 1)]
    assert cov.hits == [3] and t.group_hits(groups, 1) == [7]


def test_identical_records_of_one_group_each_carry_the_depth():
    """ACGGT twice in group 0, TTTTT in group 1, k = 3. Read ACGG covers ACG and CGG; two reads ACC cover rc(GGT)."""
    records, groups, k = [b"ACGGT", b"ACGGT", b"TTTTT"], [0, 0, 1], 3
    reads = _reads([b"ACGG", b"ACC", b"ACC"])
    cov, t = tm.model(records, groups, 2, k, reads, 100)
    assert tm.locus_depths(records, groups, k, cov) == [[1, 1, 2], [1, 1, 2], [0, 0, 0]]
    assert t.first_bin.tolist() == [0, 1, 2, 3]
    assert [_rows(t, r) for r in range(3)] == [[(3, 3, 4, 2)], [(3, 3, 4, 2)], [(3, 0, 0, 0)]]
    assert cov.hits == [4, 0] and t.group_hits(groups, 2) == [8, 0]


def test_n_and_shared_kmers_are_no_marker_loci():
    """k = 3. ACGNACG: the windows over N are no loci of a marker. GGGAC in a second group shares no k-mer with it;
    ACGTT in a third group shares ACG (and CGT = rc(ACG)), which is then nobody's marker."""
    records, groups, k = [b"ACGNACG", b"GGGAC", b"ACGTT"], [0, 1, 2], 3
    reads = _reads([b"ACG", b"GGGAC", b"AAC"])
    cov, t = tm.model(records, groups, 3, k, reads, 1)
    d = tm.locus_depths(records, groups, k, cov)
    assert d[0] == [None] * 5                     # ACG shared, CGN GNA NAC hold N
    assert d[1] == [1, 1, 1]                      # GGG, GGA, GAC
    assert d[2] == [None, None, 1]                # ACG, CGT shared; GTT = rc(AAC)
    assert t.first_bin.tolist() == [0, 5, 8, 11]
    assert _rows(t, 0) == [(0, 0, 0, 0)] * 5


# ---- the identity ----
def _dna(rng, n: int) -> bytes:
    return bytes(b"ACGT"[c] for c in rng.integers(0, 4, n))


def test_sums_equal_the_coverage_hits_iff_every_marker_has_one_locus():
    rng = np.random.default_rng(5)
    a, b, k = _dna(rng, 300), _dna(rng, 300), 21  # (k odd: no k-mer is its own reverse complement)
    reads = _reads([a[:100], a[50:200], er.revcomp(a[100:180]), b[:90], er.revcomp(b[200:300])])
    for records, groups, equal in (([a, b], [0, 1], True), ([a, a, b], [0, 0, 1], False),
                                   ([a + a[:60], b], [0, 1], False)):
        cov, t = tm.model(records, groups, 2, k, reads, 64)
        loci = [sum(x is not None for x in row) for row in tm.locus_depths(records, groups, k, cov)]
        per_group = [sum(n for n, g in zip(loci, groups) if g == gg) for gg in range(2)]
        # a k-mer and its reverse complement are two markers of one locus
        assert ([2 * n for n in per_group] == cov.markers) == equal
        sums = t.group_hits(groups, 2)
        assert sums[1] == cov.hits[1] > 0
        assert (sums[0] == cov.hits[0]) if equal else (sums[0] > cov.hits[0])
        assert int(t.bins["markers"].sum()) == sum(loci)
        # every bin width folds the same loci
        for bin in (1, 7, 1000):
            tb = tm.track(records, groups, k, cov, bin)
            assert tb.group_hits(groups, 2) == sums and int(tb.bins["max_depth"].max()) == int(t.bins["max_depth"].max())


# ---- the library's host-only layout ----
def test_track_layout_of_the_library():
    rng = np.random.default_rng(9)
    k = 21
    lens = [k - 1, k, k + 5, 0, 3 * k, 1, 2 * k + 43]
    records = [_dna(rng, n) for n in lens]
    idx = FmIndex.build(records, [0] * len(records), 1, prefix_q=4)
    nwin = [0, 1, 6, 0, 2 * k + 1, 0, k + 44]
    assert tm.loci_of(records, k) == nwin == idx.track_loci(k).tolist()
    for bin in (1, 5, 6, 7, 64, 100, TRACK_MAX_BIN):
        first = idx.track_layout(k, bin)
        np.testing.assert_array_equal(first, tm.layout(records, k, bin))
        assert first.dtype == np.uint64 and first[0] == 0
    assert np.diff(idx.track_layout(k, 1)).tolist() == nwin                       # bin = 1: one bin per locus
    assert np.diff(idx.track_layout(k, 100)).tolist() == [0, 1, 1, 0, 1, 0, 1]    # bin > nwin: one bin per record
    assert np.diff(idx.track_layout(k, 6)).tolist() == [0, 1, 1, 0, 8, 0, 11]
    # another k, records shorter than it
    assert idx.track_loci(64).tolist() == [0, 0, 0, 0, 0, 0, 2 * k + 43 - 63]
    n = C.c_uint64(99)
    assert lib().speq_index_track_layout(idx.handle, k, 6, C.byref(n), None) == 0 and n.value == 21
    for bad_bin in (0, TRACK_MAX_BIN + 1):
        with pytest.raises(SpeqError) as e:
            idx.track_layout(k, bad_bin)
        assert e.value.code == -1
    with pytest.raises(SpeqError):
        idx.track_layout(0, 10)


def test_null_arguments_are_argument_errors():
    L = lib()
    n = C.c_uint64()
    rows = (MarkerBin * 4)()
    assert L.speq_markers_track_layout(None, 100, C.byref(n), None) == -1
    assert b"null handle" in L.speq_last_error()
    assert L.speq_markers_track(None, 100, rows) == -1
    assert L.speq_index_track_layout(None, 21, 100, C.byref(n), None) == -1
    assert L.speq_markers_track_fastq(None, b"x.fq", None, None, 2, 100, None, None, None, None, None) == -1


# ---- the header ----
def test_header_symbols_and_abi_version():
    text = open(HEADER).read()
    assert re.search(r"#define\s+SPEQ_ABI_VERSION\s+8\b", text) and ABI_VERSION == 8 == lib().speq_abi_version()
    assert re.search(r"#define\s+SPEQ_TRACK_MAX_BIN\s+\(1u << 20\)", text) and TRACK_MAX_BIN == 1 << 20
    assert re.search(r"typedef struct \{\s*uint64_t markers, observed, hits, max_depth;\s*\} speq_marker_bin;", text)
    assert C.sizeof(MarkerBin) == 32 == tm.DTYPE.itemsize
    for name in ("speq_markers_track_layout", "speq_markers_track", "speq_markers_track_fastq",
                 "speq_index_track_layout"):
        assert re.search(r"\bint " + name + r"\(", text) and name in SIGNATURES
        assert getattr(lib(), name)


# ---- the CLI ----
@pytest.fixture
def work(tmp_path):
    c = Case("tiny_single")
    for f in ("refs.fa", "groups.txt", "reads_1.fq"):
        shutil.copy(os.path.join(c.dir, f), tmp_path / f)
    return tmp_path


def _run(args, cwd):
    return subprocess.run([SPEQ] + args, cwd=cwd, capture_output=True, text=True, timeout=300)


def test_cli_argument_errors(work):
    base = ["all", "-r", "refs.fa", "-g", "groups.txt", "-1", "reads_1.fq", "-x", "ref", "-o", "p.txt"]
    r = _run(base + ["--track-bin", "50"], work)
    assert r.returncode == 1 and "argument parsing error" in r.stderr and "--marker-track" in r.stderr
    for bad in ("0", str(TRACK_MAX_BIN + 1), "-3", "ten"):
        r = _run(base + ["--marker-track", "t.tsv", "--track-bin", bad], work)
        assert r.returncode == 1 and "argument parsing error" in r.stderr and "--track-bin" in r.stderr, bad
    (work / "t.tsv").write_text("x")
    r = _run(base + ["--marker-track", "t.tsv"], work)
    assert r.returncode == 1 and "Cowardly refusing" in r.stderr
    r = _run(base + ["--marker-track"], work)
    assert r.returncode == 1 and "Missing value" in r.stderr
    r = _run(["index", "-r", "refs.fa", "-g", "groups.txt", "--marker-track", "u.tsv"], work)  # a scan option
    assert r.returncode == 1 and "Unknown option" in r.stderr
    assert not (work / "p.txt").exists() and not (work / "ref.idx").exists()
    h = _run(["--help"], work).stdout
    assert "--marker-track FILE" in h and "--track-bin N" in h
