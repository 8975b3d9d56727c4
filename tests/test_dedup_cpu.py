"""CPU: the duplicate-read pass (speq_dedup_*, `speq scan --dedup`) as far as it needs no GPU.

* speq_dedup_fingerprint, the host accessor of the kernel's term function, equals the model (tests/dedup_model.py).
* On every input set of the suite the classes by fingerprint equal the classes by exact comparison of the converted
  sequences: a condition on the inputs, checked here so that no GPU test can hide a collision.
* The premise of the masking, against the independent C oracle: a scan of the reads with '!' over the records of every
  unit that is not kept equals a scan of the reads with those units removed.
* The ABI and CLI parts that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dedup_inputs as di
import dedup_model as dm
import read_report_inputs as ri
from oracle.oracle import Oracle
from speq_amd import dedup_fingerprint, lib
from speq_amd._lib import LIB_PATH, SPEQ_E_ARG, SPEQ_MODE_LOCAL, DedupStatsRecord, ScanParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEQ = os.path.join(ROOT, "bin", "speq")
KS = [8, 21, 70, 151]


# ---- the fingerprint ----
def host_fingerprints(rd, paired: bool) -> np.ndarray:
    seq, _, off = rd
    off = [int(x) for x in off]
    per = 2 if paired else 1
    out = np.zeros(((len(off) - 1) // per, 2), dtype=np.uint64)
    for u in range(len(out)):
        r = per * u
        out[u] = dedup_fingerprint(seq[off[r]:off[r + 1]], seq[off[r + 1]:off[r + 2]] if paired else None)
    return out


def test_base_codes_are_the_scans():
    """One base at position 0: the 256 byte values fall into the five codes of the scan's dna5 conversion."""
    by_code = {0: b"Aa", 1: b"Cc", 2: b"Gg", 3: b"TtUu"}
    fp = {c: dedup_fingerprint(bytes([s[0]])) for c, s in by_code.items()}
    fp[4] = dedup_fingerprint(b"N")
    assert len(set(fp.values())) == 5
    for b in range(256):
        code = next((c for c, s in by_code.items() if b in s), 4)
        assert dedup_fingerprint(bytes([b])) == fp[code] == dm.fingerprint(bytes([b])), b


def test_small_cases_of_the_definition():
    assert dedup_fingerprint(b"") == (0, 0) == dedup_fingerprint(b"", b"") == dm.fingerprint(b"")
    assert dedup_fingerprint(b"ACGT") == dedup_fingerprint(b"acgu") == dedup_fingerprint(b"ACGU", b"")
    assert dedup_fingerprint(b"ANT") == dedup_fingerprint(b"aRu") == dedup_fingerprint(b"A.T")
    x = b"GATTACAGCTTGCA"
    distinct = [(x, None), (x[:-1], None), (x[1:], None), (b"", x), (x, x), (x[:7], x[7:]), (x[:6], x[6:]),
                (x[7:], x[:7]), (b"AC", b"G"), (b"A", b"CG"), (b"G", b"AC")]
    fps = [dedup_fingerprint(a, b) for a, b in distinct]
    assert len(set(fps)) == len(fps)
    assert fps == [dm.fingerprint(a, b) for a, b in distinct]
    # the sum is commutative: two halves' terms add up to the whole's (what lets a wave split a read any way it likes)
    lo, hi = dm.fingerprints(x, [0, len(x)], False)[0].tolist()
    assert (lo, hi) == dedup_fingerprint(x)


@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
def test_host_fingerprint_equals_the_model_on_the_inputs(paired):
    rd = di.reads(21, paired)
    np.testing.assert_array_equal(host_fingerprints(rd, paired), dm.fingerprints(rd[0], rd[2], paired))


def test_host_fingerprint_equals_the_model_on_random_reads():
    """10^5 reads of random length 0 .. 300 over every byte value (most of them code 4) and over the bases' spellings,
    as single-end units and as pairs."""
    rng = np.random.default_rng(100_000)
    alphabet = np.frombuffer(b"ACGTUacgtuNnR.", dtype=np.uint8)
    for chunk in range(10):
        lens = rng.integers(0, 301, 10_000)
        off = np.zeros(len(lens) + 1, dtype=np.uint64)
        off[1:] = np.cumsum(lens)
        n = int(off[-1])
        raw = rng.integers(0, 256, n).astype(np.uint8)
        seq = np.where(rng.random(n) < 0.9, alphabet[rng.integers(0, len(alphabet), n)], raw).tobytes()
        paired = bool(chunk % 2)
        np.testing.assert_array_equal(host_fingerprints((seq, None, off), paired), dm.fingerprints(seq, off, paired))


# ---- the inputs hold no collision ----
def input_sets():
    for k in KS:
        for paired in (False, True):
            yield f"reads-{k}-{paired}", di.reads(k, paired), paired
    yield "chunk", di.chunk_reads(), False
    for name in ("tiny_single", "tiny_paired"):
        seqs, quals, paired = di.fastq_records(name)
        yield f"fastq-{name}", ri.pack(seqs, quals), paired
        uniq, dup, paired = di.cli_records(name)
        yield f"cli-uniq-{name}", di.flatten(uniq), paired
        yield f"cli-dup-{name}", di.flatten(dup), paired


def test_classes_by_fingerprint_equal_classes_by_exact_comparison():
    for name, rd, paired in input_sets():
        exact = dm.rep_exact(rd[0], rd[2], paired)
        np.testing.assert_array_equal(dm.rep_fingerprint(rd[0], rd[2], paired), exact, err_msg=name)
        if name.startswith("cli-uniq"):
            assert (exact == np.arange(len(exact))).all(), name


def test_the_inputs_hold_what_they_promise():
    units, edge = di.unit_list(21)
    rd = di.reads(21, False)
    off = rd[2]
    for L, i in edge.items():
        assert int(off[i + 1] - off[i]) == L and int(off[i]) % 2 == 1, (L, i)
    rep = dm.rep_exact(rd[0], rd[2], False)
    st = dm.stats(rep)
    assert st["units"] == di.n_units(21, False) == len(units) and st["max_multiplicity"] == 4096
    assert (st["mult_hist"] > 0).all() and int(st["mult_hist"].sum()) == st["distinct"] < st["units"]
    sizes = np.bincount(rep)
    assert {1, 2, 3, 6, 7, 8, 9, 4096} <= set(sizes.tolist())
    # the paired flavour: what only pairs have
    rdp = di.reads(21, True)
    repp = dm.rep_exact(rdp[0], rdp[2], True)
    base = len(units)
    assert repp[base:].tolist() == [base, base + 1, base + 2, base + 3, base + 4, base + 5, base + 6, base, base,
                                    int(repp[base + 9]), int(repp[base + 9])]
    assert repp[base + 9] < base  # the empty pair is the edge block's empty unit with its empty mate
    assert dm.stats(repp)["max_multiplicity"] == 4096
    # the chunk input lies on both sides of 65,536 units and holds duplicates across it
    crep = dm.rep_exact(di.chunk_reads()[0], di.chunk_reads()[2], False)
    assert len(crep) > 65_536 and (crep[65_536:] < 65_536).any() and (crep[65_536:] >= 65_536).any()
    for name in ("tiny_single", "tiny_paired"):
        uniq, dup, paired = di.cli_records(name)
        d = di.flatten(dup)
        st = dm.stats(dm.rep_exact(d[0], d[2], paired))
        assert st["distinct"] == len(uniq) < st["units"] == len(dup) and st["max_multiplicity"] >= 8


# ---- the premise, against the C oracle ----
@pytest.mark.parametrize("k", [8, 21, 70])
def test_masked_scan_equals_scan_of_removed_units(k):
    ref = ri.base_ref()
    oracle = Oracle(ref.records, ref.groups, 3, k)
    for paired in (False, True):
        seq, qual, off = di.reads(k, paired)
        rep = dm.rep_fingerprint(seq, off, paired)
        masked = dm.mask(qual, off, rep, paired)
        removed = dm.remove(seq, qual, off, rep, paired)
        assert len(masked) == len(qual) and len(removed[2]) - 1 == (2 if paired else 1) * int((rep == np.arange(len(rep))).sum())
        for local in (False, True):
            for cutoff in (0, 30):
                a = oracle.scan(seq, masked, off, cutoff, paired, local, threads=1)
                b = oracle.scan(*removed, cutoff, paired, local, threads=1)
                plain = oracle.scan(seq, qual, off, cutoff, paired, local, threads=1)
                assert (a[0], a[1], a[2].tolist()) == (b[0], b[1], b[2].tolist()), (paired, local, cutoff)
                if local:
                    np.testing.assert_array_equal(a[3], b[3])
                if k <= 21:
                    assert a[0] < plain[0] and a[0] > 0  # the duplicates carried windows, and so do the kept units


# ---- the library, without a device ----
NEW_SYMBOLS = ("speq_dedup_create", "speq_dedup_add_reads_device", "speq_dedup_add_reads", "speq_dedup_finalize",
               "speq_dedup_representatives", "speq_dedup_mask_device", "speq_dedup_scan_reads", "speq_dedup_free",
               "speq_dedup_fingerprint", "speq_dedup_fastq")


def last_error() -> str:
    return lib().speq_last_error().decode()


def test_abi_version_and_symbols():
    assert lib().speq_abi_version() == 8
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (speq_[a-z0-9_]+)$", out, flags=re.M))
    assert not [s for s in NEW_SYMBOLS if s not in exported]
    hdr = open(os.path.join(ROOT, "include", "speq_scan.h")).read()
    assert "#define SPEQ_ABI_VERSION 8" in hdr and "#define SPEQ_DEDUP_BINS 8" in hdr
    assert C.sizeof(DedupStatsRecord) == 96


def test_argument_checks_precede_device_use():
    """No replica exists here, so the replica or the handle is null in every call; the message tells which check refused
    it. A paired scan's odd record count is told from the parameters, before the handle is looked at; a paired handle's
    own check needs a handle (tests/test_gpu_dedup.py)."""
    L = lib()
    h = C.c_void_p()
    assert L.speq_dedup_create(None, 1, C.byref(h)) == SPEQ_E_ARG and "null device index" in last_error()
    assert not h.value
    off = np.array([0, 4, 2, 6], dtype=np.uint64)
    offp = off.ctypes.data_as(C.POINTER(C.c_uint64))
    assert L.speq_dedup_add_reads(None, b"ACGTAC", None, 3, 0) == SPEQ_E_ARG and "null offsets" in last_error()
    assert L.speq_dedup_add_reads(None, b"ACGTAC", offp, 3, 0) == SPEQ_E_ARG
    assert "offsets must be non-decreasing" in last_error()
    off[:] = [0, 2, 4, 6]
    assert L.speq_dedup_add_reads(None, None, offp, 3, 0) == SPEQ_E_ARG and "null read buffer" in last_error()
    assert L.speq_dedup_add_reads(None, b"ACGTAC", offp, 3, 0) == SPEQ_E_ARG and "null handle" in last_error()
    assert L.speq_dedup_add_reads(None, None, None, 0, 0) == SPEQ_E_ARG and "null handle" in last_error()
    assert L.speq_dedup_add_reads_device(None, None, None, 3, 0, None) == SPEQ_E_ARG and "null buffer" in last_error()
    assert L.speq_dedup_add_reads_device(None, 16, 16, 3, 0, None) == SPEQ_E_ARG and "null handle" in last_error()
    st = DedupStatsRecord()
    assert L.speq_dedup_finalize(None, C.byref(st)) == SPEQ_E_ARG and "null handle" in last_error()
    rep = np.zeros(4, dtype=np.uint32)
    assert L.speq_dedup_representatives(None, 0, 4, rep.ctypes.data_as(C.POINTER(C.c_uint32))) == SPEQ_E_ARG
    assert "null handle" in last_error()
    assert L.speq_dedup_mask_device(None, None, None, 3, 0, None) == SPEQ_E_ARG and "null buffer" in last_error()
    assert L.speq_dedup_mask_device(None, 16, 16, 3, 0, None) == SPEQ_E_ARG and "null handle" in last_error()
    counts = np.zeros(8, dtype=np.uint64)
    cp = counts.ctypes.data_as(C.POINTER(C.c_uint64))
    assert L.speq_dedup_scan_reads(None, None, b"ACGTAC", b"IIIIII", offp, 3, 0, None, cp, None) == SPEQ_E_ARG
    assert "null params" in last_error()
    pp = ScanParams(21, 30, 1, 0)
    assert L.speq_dedup_scan_reads(None, None, b"ACGTAC", b"IIIIII", offp, 3, 0, C.byref(pp), cp, None) == SPEQ_E_ARG
    assert "even record count" in last_error()
    loc = ScanParams(21, 30, 0, SPEQ_MODE_LOCAL)
    assert L.speq_dedup_scan_reads(None, None, b"ACGTAC", b"IIIIII", offp, 3, 0, C.byref(loc), cp, None) == SPEQ_E_ARG
    assert "local mode needs weights" in last_error()
    g = ScanParams(21, 30, 0, 0)
    assert L.speq_dedup_scan_reads(None, None, b"ACGTAC", b"IIIIII", offp, 3, 0, C.byref(g), None, None) == SPEQ_E_ARG
    assert "null output" in last_error()
    assert L.speq_dedup_scan_reads(None, None, b"ACGTAC", b"IIIIII", offp, 3, 0, C.byref(g), cp, None) == SPEQ_E_ARG
    assert "null handle" in last_error()
    assert L.speq_dedup_fastq(None, None, b"x.fq", None, None, 2, C.byref(st), cp, None, None) == SPEQ_E_ARG
    assert "null params" in last_error()
    assert L.speq_dedup_fastq(None, None, b"x.fq", None, C.byref(g), 2, C.byref(st), cp, None, None) == SPEQ_E_ARG
    assert "null argument" in last_error()
    L.speq_dedup_free(None)
    assert not counts.any()


def test_cli_dedup_option(tmp_path):
    r = subprocess.run([SPEQ, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--dedup FILE" in r.stdout
    (tmp_path / "r.fq").write_text("@r\nACGT\n+\nIIII\n")
    r = subprocess.run([SPEQ, "scan", "-1", "r.fq", "--dedup"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "argument parsing error" in r.stderr and "Missing value for option --dedup" in r.stderr
    # an existing FILE needs --force, like every output file (the index only has to exist for the parser)
    (tmp_path / "ref.idx").write_bytes(b"")
    (tmp_path / "f.tsv").write_text("kept\n")
    base = [SPEQ, "scan", "-1", "r.fq", "-x", "ref", "-o", "p.txt", "--dedup", "f.tsv"]
    r = subprocess.run(base, cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Cowardly refusing to use an existing output file" in r.stderr
    assert (tmp_path / "f.tsv").read_text() == "kept\n"
    r = subprocess.run(base + ["--force"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert "Cowardly" not in r.stderr and "argument parsing error" not in r.stderr  # (it fails later: no such index)
    r = subprocess.run([SPEQ, "index", "--dedup", "x"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Unknown option --dedup" in r.stderr
