"""CPU: the per-unit report's model against the C oracle, and the parts of the report's interface that need no GPU.

tests/read_report_model.py states what speq_report_reads must return; here its sums are checked against
oracle.Oracle.scan on the inputs of tests/test_gpu_read_report.py (tests/read_report_inputs.py) and on the golden
cases: the passing windows give T, the units with two or more groups give the ambiguous count, and the unique windows
per group give U[g]. The library side: ABI version 8, the new symbols, the argument checks that precede any device use,
and the CLI's --group-sets option."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import em_reference as er
import read_report_inputs as ri
import read_report_model as rm
from golden_io import CASES, Case
from oracle.oracle import Oracle
from speq_amd import lib
from speq_amd._lib import LIB_PATH, SPEQ_E_ARG, ScanParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEQ = os.path.join(ROOT, "bin", "speq")


def check_against_oracle(records, groups, G, k, seq, qual, offsets, cutoff, paired):
    rep = rm.report(er.build_index(records, groups, G, k), G, k, seq, qual, offsets, cutoff, paired)
    T, amb, U, _ = Oracle(records, groups, G, k).scan(np.frombuffer(seq, np.uint8), np.frombuffer(qual, np.uint8),
                                                      offsets, phred_cutoff=cutoff, paired=paired)
    assert sum(rep.passing) == T
    assert rep.ambiguous == amb
    assert rep.per_group == U.tolist()
    assert sum(rep.unique) == int(U.sum())
    assert all(p >= u + s for p, u, s in zip(rep.passing, rep.unique, rep.shared))
    assert all((f >= 0) == (u > 0) and (f < 0 or f in s) for f, u, s in zip(rep.first_group, rep.unique, rep.sets))
    return rep


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("k", [3, 8, 21, 33, 70, 151])
def test_model_matches_the_oracle_on_the_base_input(k, paired):
    ref = ri.base_ref()
    seq, qual, off = ri.base_reads(k, paired)
    rep = check_against_oracle(ref.records, ref.groups, 3, k, seq, qual, off, ri.CUTOFF, paired)
    if not paired and k in (21, 33):
        seqs, _ = ri.base_read_list(k)
        i = seqs.index(ri.chimera(k))
        assert rep.sets[i] == frozenset({0, 2}) and rep.first_group[i] == 0
        assert rep.sets[i + 1] == frozenset({0, 2}) and rep.first_group[i + 1] == 2
    if paired and k == 21:
        u = ri.split_pair_unit(k)
        assert rep.sets[u] == frozenset({0, 1}) and rep.first_group[u] == 0 and rep.ambiguous >= 1


def test_model_matches_the_oracle_on_70_groups():
    records, groups = ri.many_ref()
    seq, qual, off = ri.many_reads()
    rep = check_against_oracle(records, groups, 70, ri.MANY_K, seq, qual, off, ri.CUTOFF, False)
    assert rep.W == 2
    assert frozenset({63, 64}) in rep.sets and frozenset({69}) in rep.sets and frozenset({0}) in rep.sets
    w = rep.words()
    i = rep.sets.index(frozenset({63, 64}))
    assert w[i].tolist() == [1 << 63, 1]


@pytest.mark.parametrize("name", CASES)
def test_model_matches_the_oracle_on_the_golden_cases(name):
    c = Case(name)
    for k in c.ks:
        check_against_oracle(c.records, c.groups, c.G, k, c.seq, c.qual, c.offsets, c.cutoff, c.paired)


def test_sorted_sets_order():
    h = {frozenset(): 5, frozenset({64}): 1, frozenset({0, 1}): 2, frozenset({63}): 3, frozenset({2}): 4}
    assert [sorted(s) for s, _ in rm.sorted_sets(h)] == [[], [0, 1], [2], [63], [64]]


# ---- the library, without a device ----
NEW_SYMBOLS = ("speq_report_reads_device", "speq_report_reads", "speq_report_fastq", "speq_group_sets_count",
               "speq_group_sets_get", "speq_group_sets_totals", "speq_group_sets_free")


def test_abi_version_and_symbols():
    assert lib().speq_abi_version() == 8
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (speq_[a-z0-9_]+)$", out, flags=re.M))
    assert not [s for s in NEW_SYMBOLS if s not in exported]
    hdr = open(os.path.join(ROOT, "include", "speq_scan.h")).read()
    assert "#define SPEQ_REPORT_MAX_K 1024" in hdr and "#define SPEQ_ABI_VERSION 8" in hdr


def last_error() -> str:
    return lib().speq_last_error().decode()


def test_argument_checks_precede_device_use():
    """No replica exists here, so the handle is null in every call; the message tells which check refused it."""
    L = lib()
    off = np.zeros(4, dtype=np.uint64)
    offp = off.ctypes.data_as(C.POINTER(C.c_uint64))
    rec = np.zeros((3, 4), dtype=np.uint32)
    sets = np.zeros(3, dtype=np.uint64)
    setp = sets.ctypes.data_as(C.POINTER(C.c_uint64))

    def host(p, n):
        return L.speq_report_reads(None, b"", b"", offp, n, C.byref(p) if p else None, rec.ctypes.data, setp)

    def device(p, n):
        return L.speq_report_reads_device(None, None, None, None, n, C.byref(p) if p else None, None, None, None)

    for call in (host, device):
        assert call(None, 3) == SPEQ_E_ARG and "null" in last_error()
        for k in (0, 1025):
            assert call(ScanParams(k, 30, 0, 0), 3) == SPEQ_E_ARG and "k must be in [1, 1024]" in last_error()
        assert call(ScanParams(21, 30, 1, 0), 3) == SPEQ_E_ARG and "even record count" in last_error()
        for k in (1, 21, 1024):  # a valid shape gets as far as the handle
            assert call(ScanParams(k, 30, 1, 0), 2) == SPEQ_E_ARG and "null device index" in last_error()
    h = C.c_void_p()
    p = ScanParams(21, 30, 0, 0)
    assert L.speq_report_fastq(None, b"x.fq", None, C.byref(p), 2, C.byref(h), None) == SPEQ_E_ARG
    assert L.speq_group_sets_count(None) == 0
    w, u = C.c_uint64(), C.c_uint64()
    assert L.speq_group_sets_get(None, 0, C.byref(w), C.byref(u)) == SPEQ_E_ARG
    assert L.speq_group_sets_totals(None, None, None, None, None) == SPEQ_E_ARG
    L.speq_group_sets_free(None)


def test_cli_group_sets_option(tmp_path):
    r = subprocess.run([SPEQ, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--group-sets FILE" in r.stdout
    (tmp_path / "r.fq").write_text("@r\nACGT\n+\nIIII\n")
    r = subprocess.run([SPEQ, "scan", "-1", "r.fq", "--group-sets"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1 and "argument parsing error" in r.stderr
    assert "Missing value for option --group-sets" in r.stderr
    # an index-only run does not take it (like the other scan options)
    r = subprocess.run([SPEQ, "index", "--group-sets", "x.tsv"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1 and "Unknown option --group-sets" in r.stderr
