"""CPU: the marker-coverage model against the C oracle, and the parts of the feature's interface that need no GPU.

tests/marker_model.py states what speq_markers_finalize / speq_markers_list must return. Here its hits per group are
checked against oracle.Oracle.scan's U[g] on the inputs of tests/test_gpu_markers.py (tests/read_report_inputs.py, the
golden cases), its bins against its marker counts, and the two-sample case (equal hits, different breadth) is built.
The library side: ABI version 8, the new symbols, the argument checks that precede any device use, and the CLI's
--marker-coverage option."""
import ctypes as C
import os
import re
import subprocess
from collections import Counter

import numpy as np
import pytest

import em_reference as er
import marker_model as mm
import read_report_inputs as ri
from golden_io import CASES, Case
from oracle.oracle import Oracle
from speq_amd import lib
from speq_amd._lib import LIB_PATH, SPEQ_E_ARG, MarkerCov, ScanParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEQ = os.path.join(ROOT, "bin", "speq")


def check_against_oracle(records, groups, G, k, seq, qual, offsets, cutoff):
    cov = mm.coverage(er.build_index(records, groups, G, k), G, k, seq, qual, offsets, cutoff)
    _, _, U, _ = Oracle(records, groups, G, k).scan(np.frombuffer(seq, np.uint8), np.frombuffer(qual, np.uint8),
                                                    offsets, phred_cutoff=cutoff)
    assert cov.hits == U.tolist()
    rec = cov.records()
    assert rec.shape == (G, 12)
    assert rec[:, 4:].sum(axis=1).tolist() == cov.markers                       # the bins hold every marker once
    assert rec[:, 4].tolist() == [m - o for m, o in zip(cov.markers, cov.observed)]
    assert all(o <= m and o <= h and mx <= h and (mx > 0) == (o > 0)
               for m, o, h, mx in zip(cov.markers, cov.observed, cov.hits, cov.max_depth))
    return cov


@pytest.mark.parametrize("k", [3, 8, 21, 33, 70, 151, 1024])
def test_model_hits_are_the_oracles_unique_counts_on_the_base_input(k):
    ref = ri.base_ref()
    cov = check_against_oracle(ref.records, ref.groups, 3, k, *ri.base_reads(k), ri.CUTOFF)
    triples = list(zip(cov.markers, cov.observed, cov.hits))
    if k == 21:
        assert triples == [(4682, 3721, 7711), (4420, 4288, 15675), (4648, 4619, 24605)]
        assert cov.max_depth == [9, 16, 14]
        assert all(row[7] > 0 for row in cov.depth_hist), "the last bin (depth >= 7) is in use"
    if k == 3:
        assert triples == [(0, 0, 0)] * 3                                       # the all-zero edge
    if k == 1024:
        assert cov.markers == [17_954] * 3 and cov.observed == [208, 1_420, 668]


def test_model_on_70_groups():
    records, groups = ri.many_ref()
    cov = check_against_oracle(records, groups, 70, ri.MANY_K, *ri.many_reads(), ri.CUTOFF)
    assert cov.markers == [560] * 70
    assert [g for g, h in enumerate(cov.hits) if h] == [0, 1, 33, 63, 64, 65, 69]


@pytest.mark.parametrize("name", CASES)
def test_model_hits_are_the_oracles_unique_counts_on_the_golden_cases(name):
    c = Case(name)
    for k in c.ks:
        check_against_oracle(c.records, c.groups, c.G, k, c.seq, c.qual, c.offsets, c.cutoff)


def test_two_samples_have_equal_hits_and_different_breadth():
    ref, k, n = ri.base_ref(), 21, 4096
    index = er.build_index(ref.records, ref.groups, 3, k)
    copies, spread = mm.two_samples([ref.records[1]], index, 1, k, n)
    a = check_against_oracle(ref.records, ref.groups, 3, k, *copies, ri.CUTOFF)
    b = check_against_oracle(ref.records, ref.groups, 3, k, *spread, ri.CUTOFF)
    assert a.hits == b.hits == [0, n, 0]
    assert (a.observed[1], a.max_depth[1]) == (1, n) and (b.observed[1], b.max_depth[1]) == (n, 1)
    assert a.depth_hist[1][7] == 1 and b.depth_hist[1][1] == n
    la, lb = a.tsv_lines(["V0", "V1", "V2"])[1].split("\t"), b.tsv_lines(["V0", "V1", "V2"])[1].split("\t")
    assert la[4] == lb[4] and la[6] == lb[6]                                    # same hits, same expected breadth
    assert float(la[3]) < 0.001 < 0.5 < float(lb[6]) < float(lb[3])             # breadth tells them apart


def test_tsv_lines():
    cov = mm.Coverage(3, {b"AA": 0, b"AC": 0, b"CC": 2}, Counter({b"AA": 9, b"CC": 1}))
    assert mm.HEADER.rstrip("\n").split("\t") == ["name", "markers", "observed", "breadth", "hits", "mean_depth",
                                                  "expected_breadth", "max_depth"] + [f"d{j}" for j in range(8)]
    assert cov.tsv_lines(["a", "b", "c"]) == [
        "a\t2\t1\t0.500000\t9\t4.500000\t0.988891\t9\t1\t0\t0\t0\t0\t0\t0\t1\n",
        "b\t0\t0\t-\t0\t-\t-\t0\t0\t0\t0\t0\t0\t0\t0\t0\n",
        "c\t1\t1\t1.000000\t1\t1.000000\t0.632121\t1\t0\t1\t0\t0\t0\t0\t0\t0\n"]


# ---- the library, without a device ----
NEW_SYMBOLS = ("speq_markers_create", "speq_markers_add_reads_device", "speq_markers_add_reads",
               "speq_markers_finalize", "speq_markers_list", "speq_markers_fastq", "speq_markers_free")


def test_abi_version_and_symbols():
    assert lib().speq_abi_version() == 8
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (speq_[a-z0-9_]+)$", out, flags=re.M))
    assert not [s for s in NEW_SYMBOLS if s not in exported]
    hdr = open(os.path.join(ROOT, "include", "speq_scan.h")).read()
    assert "#define SPEQ_MARKER_BINS 8" in hdr and "#define SPEQ_ABI_VERSION 8" in hdr
    assert C.sizeof(MarkerCov) == 96


def last_error() -> str:
    return lib().speq_last_error().decode()


def test_argument_checks_precede_device_use():
    """No replica exists here, so the handle is null in every call; the message tells which check refused it."""
    L = lib()
    h = C.c_void_p()
    # create: params, k, then the replica
    assert L.speq_markers_create(None, None, C.byref(h)) == SPEQ_E_ARG and "null params" in last_error()
    for k in (0, 1025):
        p = ScanParams(k, 30, 0, 0)
        assert L.speq_markers_create(None, C.byref(p), C.byref(h)) == SPEQ_E_ARG
        assert "k must be in [1, 1024]" in last_error()
    for k in (1, 21, 1024):
        p = ScanParams(k, 30, 0, 0)
        assert L.speq_markers_create(None, C.byref(p), C.byref(h)) == SPEQ_E_ARG
        assert "null device index" in last_error()
    assert not h.value
    # add: the arrays, then the handle; no reads is still a call on a handle
    off = np.array([0, 4, 2, 6], dtype=np.uint64)
    offp = off.ctypes.data_as(C.POINTER(C.c_uint64))
    assert L.speq_markers_add_reads(None, b"ACGTAC", b"IIIIII", None, 3) == SPEQ_E_ARG and "null offsets" in last_error()
    assert L.speq_markers_add_reads(None, b"ACGTAC", b"IIIIII", offp, 3) == SPEQ_E_ARG
    assert "offsets must be non-decreasing" in last_error()
    off[:] = [0, 2, 4, 6]
    assert L.speq_markers_add_reads(None, None, b"IIIIII", offp, 3) == SPEQ_E_ARG and "null read buffer" in last_error()
    assert L.speq_markers_add_reads(None, b"ACGTAC", b"IIIIII", offp, 3) == SPEQ_E_ARG and "null handle" in last_error()
    assert L.speq_markers_add_reads(None, None, None, None, 0) == SPEQ_E_ARG and "null handle" in last_error()
    assert L.speq_markers_add_reads_device(None, None, None, None, 3, None) == SPEQ_E_ARG
    assert "null buffer" in last_error()
    assert L.speq_markers_add_reads_device(None, 16, 16, 16, 3, None) == SPEQ_E_ARG and "null handle" in last_error()
    assert L.speq_markers_add_reads_device(None, None, None, None, 0, None) == SPEQ_E_ARG
    assert "null handle" in last_error()
    cov = (MarkerCov * 3)()
    assert L.speq_markers_finalize(None, cov) == SPEQ_E_ARG and "null handle" in last_error()
    n = C.c_uint64()
    assert L.speq_markers_list(None, C.byref(n), None, None, None) == SPEQ_E_ARG and "null handle" in last_error()
    p = ScanParams(21, 30, 0, 0)
    assert L.speq_markers_fastq(None, b"x.fq", None, None, 2, cov, None) == SPEQ_E_ARG and "null params" in last_error()
    bad = ScanParams(1025, 30, 0, 0)
    assert L.speq_markers_fastq(None, b"x.fq", None, C.byref(bad), 2, cov, None) == SPEQ_E_ARG
    assert "k must be in [1, 1024]" in last_error()
    assert L.speq_markers_fastq(None, b"x.fq", None, C.byref(p), 2, cov, None) == SPEQ_E_ARG and "null" in last_error()
    L.speq_markers_free(None)


def test_cli_marker_coverage_option(tmp_path):
    r = subprocess.run([SPEQ, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--marker-coverage FILE" in r.stdout
    (tmp_path / "r.fq").write_text("@r\nACGT\n+\nIIII\n")
    r = subprocess.run([SPEQ, "scan", "-1", "r.fq", "--marker-coverage"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1 and "argument parsing error" in r.stderr
    assert "Missing value for option --marker-coverage" in r.stderr
    # an index-only run does not take it (like the other scan options)
    r = subprocess.run([SPEQ, "index", "--marker-coverage", "x.tsv"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1 and "Unknown option --marker-coverage" in r.stderr
