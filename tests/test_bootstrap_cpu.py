"""CPU: the read bootstrap's model against the C oracle, and the parts of the feature that need no GPU.

tests/bootstrap_model.py states what speq_bootstrap_* must return. Here its weight function (thresholds recomputed from
decimals) is compared with the library's speq_bootstrap_weight, the draws' mean and variance with Poisson(1)'s, its row
0 with oracle.Oracle.scan on the inputs of tests/test_gpu_bootstrap.py, and its bootstrap variance with the exact
variance of a Poisson-weighted sum. The library side: speq_bootstrap_summary against the model's summary, ABI version
8, the new symbols, the argument checks that precede any device use, and the CLI's --bootstrap options."""
import ctypes as C
import math
import os
import re
import subprocess
from functools import lru_cache

import numpy as np
import pytest

import bootstrap_model as bm
import em_reference as er
import read_report_inputs as ri
from oracle.oracle import Oracle
from speq_amd import bootstrap_summary, lib
from speq_amd._lib import LIB_PATH, SPEQ_E_ARG, SPEQ_MODE_LOCAL, BootstrapCI, ScanParams, SpeqError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEQ = os.path.join(ROOT, "bin", "speq")


# ---- the weight function ----
def test_thresholds_as_stated():
    c = bm.thresholds()
    assert len(c) == 21 and c[0] == 0x5E2D58D8B3BCDF1A and c[19] == 2 ** 64 - 3 and c[20] == 2 ** 64 - 1


@lru_cache(maxsize=None)
def million_triples():
    """(seeds, units, replicates) of 10^6 draws: 1,000 replicates of 1,000 units, a quarter of them at 2^40 and above,
    some at the top of the u64 range, over four seeds."""
    rng = np.random.default_rng(5)
    units = np.concatenate([np.arange(500, dtype=np.uint64), np.uint64(1 << 40) + np.arange(250, dtype=np.uint64),
                            rng.integers(0, 1 << 63, 240, dtype=np.uint64),
                            np.uint64(2 ** 64 - 10) + np.arange(10, dtype=np.uint64)])
    seeds = [0, 1, 7, 2 ** 64 - 1]
    return seeds, units, 1000


def test_library_weights_equal_the_model_on_a_million_triples_and_are_poisson_1():
    L = lib()
    seeds, units, B = million_triples()
    per_seed = len(units) // len(seeds)
    draws = []
    for i, seed in enumerate(seeds):
        u = units[i * per_seed:(i + 1) * per_seed]
        w = bm.weights(seed, u, B)
        assert (w[0] == 1).all()
        got = np.array([[L.speq_bootstrap_weight(seed, int(x), b) for x in u] for b in range(B + 1)], dtype=np.int64)
        np.testing.assert_array_equal(got, w)
        # the vectorised model against its own integer restatement, on a few
        for b in (1, 2, B):
            for j in (0, per_seed - 1):
                assert bm.weight_int(seed, int(u[j]), b) == w[b, j]
        draws.append(w[1:].ravel())
    d = np.concatenate(draws)
    assert d.size == 10 ** 6 and d.max() <= 21
    # Poisson(1): mean 1, variance 1, fourth central moment 4, so var(s^2) = (4 - 1) / n
    assert abs(d.mean() - 1.0) <= 5e-3
    assert abs(d.var(ddof=1) - 1.0) <= 5 * math.sqrt(3 / 10 ** 6)


def test_a_known_triple_for_each_weight_0_to_4_at_the_thresholds():
    """For each weight 0 .. 4 the model finds, among the first draws of seed 3, the draw h closest below the next
    threshold and the one closest at or above the last: the library must put both on the model's side."""
    L = lib()
    c = bm.thresholds()
    seed = 3
    best = {}
    for unit in range(4000):
        for b in (1, 2, 3):
            h = bm.draw_int(seed, unit, b)
            w = sum(h >= t for t in c)
            if w > 4:
                continue
            lo_gap = h - (c[w - 1] if w else 0)
            hi_gap = c[w] - h
            for key, gap in (((w, "lo"), lo_gap), ((w, "hi"), hi_gap)):
                if key not in best or gap < best[key][0]:
                    best[key] = (gap, unit, b)
    assert sorted({w for w, _ in best}) == [0, 1, 2, 3, 4]
    for (w, _), (gap, unit, b) in best.items():
        assert L.speq_bootstrap_weight(seed, unit, b) == w == bm.weight_int(seed, unit, b), (w, unit, b, gap)
    assert L.speq_bootstrap_weight(seed, 17, 0) == 1


# ---- the model against the oracle ----
@lru_cache(maxsize=None)
def base_units(k: int, paired: bool, local: bool) -> bm.Units:
    ref = ri.base_ref()
    return bm.units(er.build_index(ref.records, ref.groups, 3, k), 3, k, *ri.base_reads(k), ri.CUTOFF, paired, local)


def check_row0(un: bm.Units, records, groups, G, k, reads, paired):
    counts, w = bm.replicates(un, 1, 1)
    seq, qual, off = reads
    T, amb, U, W = Oracle(records, groups, G, k).scan(np.frombuffer(seq, np.uint8), np.frombuffer(qual, np.uint8), off,
                                                      phred_cutoff=ri.CUTOFF, paired=paired, local=True)
    assert counts[0].tolist() == [T, amb] + U.tolist()
    assert counts[0, 0] == un.P.sum() and counts[0, 1] == un.amb.sum()
    tol = bm.weights_bound(k, counts)[0]
    assert (np.abs(np.asarray(W) - w[0]) <= tol * w[0]).all(), (W, w[0])
    return counts


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("k", [8, 21, 70, 151])
def test_model_row_0_is_the_oracles_scan_on_the_base_input(k, paired):
    ref = ri.base_ref()
    counts = check_row0(base_units(k, paired, True), ref.records, ref.groups, 3, k, ri.base_reads(k), paired)
    if k == 21:
        assert counts[0, 1] > 0 and (counts[0, 2:] > 0).all()


def test_model_row_0_is_the_oracles_scan_on_70_groups():
    records, groups = ri.many_ref()
    reads = ri.many_reads()
    un = bm.units(er.build_index(records, groups, 70, ri.MANY_K), 70, ri.MANY_K, *reads, ri.CUTOFF, False, True)
    counts = check_row0(un, records, groups, 70, ri.MANY_K, reads, False)
    assert np.flatnonzero(counts[0, 2:]).tolist() == [0, 1, 33, 63, 64, 65, 69]


def test_bootstrap_variance_is_the_poisson_weighted_sums():
    """Var(sum_u w_u c_u) = sum_u c_u^2 for independent Poisson(1) weights; the sample variance over B replicates of a
    near-normal sum has relative standard error sqrt(2 / (B - 1))."""
    un = base_units(21, False, False)
    B = 1024
    counts, _ = bm.replicates(un, 11, B)
    for g in range(3):
        exact = float((un.c[:, g].astype(np.float64) ** 2).sum())
        var = counts[1:, 2 + g].astype(np.float64).var(ddof=1)
        assert exact > 0 and abs(var / exact - 1.0) <= 5 * math.sqrt(2 / (B - 1)), (g, var, exact)


def test_replicates_of_a_tiled_input_equal_the_units_written_out():
    un = base_units(21, False, False)
    n = 2 * un.n + 37
    rep = bm.Units(3, *(np.concatenate([a, a, a[:37]]) for a in (un.P, un.amb, un.c)), None)
    a, _ = bm.replicates(un, 5, 9, first_unit=(1 << 40) + 5, n_total=n)
    b, _ = bm.replicates(rep, 5, 9, first_unit=(1 << 40) + 5)
    np.testing.assert_array_equal(a, b)


# ---- speq_bootstrap_summary ----
def assert_summary(counts, wts, u_ref, tot_ref, scale, level):
    got = bootstrap_summary(counts, wts, u_ref, tot_ref, scale, level)
    exp = bm.summary(counts, wts, u_ref, tot_ref, scale, level)
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        assert g["used"] == e["used"]
        for f in ("estimate", "lo", "hi"):  # one expression per value, order statistics: exact
            assert g[f] == e[f] or (math.isnan(g[f]) and math.isnan(e[f])), (f, g, e)
        for f in ("mean", "se"):
            assert abs(g[f] - e[f]) <= 1e-12 * abs(e[f]), (f, g, e)
    return got


@pytest.mark.parametrize("level", [0.5, 0.95])
def test_summary_against_the_model(level):
    un = base_units(21, False, True)
    counts, wts = bm.replicates(un, 7, 129)
    u_ref, tot_ref = np.array([4682, 4420, 4648], dtype=np.uint64), np.array([19960] * 3, dtype=np.uint64)
    glob = assert_summary(counts, None, u_ref, tot_ref, 1.0 / 0.99 ** 21, level)
    loc = assert_summary(counts, wts, u_ref, tot_ref, 1.0, level)
    for ci in glob + loc:
        assert ci["used"] == 129 and ci["lo"] <= ci["mean"] <= ci["hi"] and ci["se"] > 0
        assert level < 0.9 or ci["lo"] < ci["estimate"] < ci["hi"]
    # a group without reference windows: 0 everywhere
    tot0 = tot_ref.copy()
    tot0[1] = 0
    z = assert_summary(counts, None, u_ref, tot0, 1.0, level)[1]
    assert (z["estimate"], z["mean"], z["se"], z["lo"], z["hi"], z["used"]) == (0.0, 0.0, 0.0, 0.0, 0.0, 129)
    # replicates without a passing window are left out
    c2 = counts.copy()
    c2[[3, 64, 129]] = 0
    assert all(ci["used"] == 126 for ci in assert_summary(c2, None, u_ref, tot_ref, 1.0, level))
    c1 = counts.copy()
    c1[2:] = 0
    one = assert_summary(c1, None, u_ref, tot_ref, 1.0, level)
    assert all(ci["used"] == 1 and ci["se"] == 0.0 and ci["lo"] == ci["hi"] == ci["mean"] for ci in one)
    c0 = counts.copy()
    c0[1:] = 0
    none = assert_summary(c0, None, u_ref, tot_ref, 1.0, level)
    assert all((ci["used"], ci["mean"], ci["se"], ci["lo"], ci["hi"]) == (0, 0.0, 0.0, 0.0, 0.0) for ci in none)
    assert all(ci["estimate"] > 0 for ci in none)


def test_summary_rejects_bad_levels_and_shapes():
    counts = np.ones((3, 5), dtype=np.uint64)
    ref = np.ones(3, dtype=np.uint64)
    for level in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(SpeqError, match="level must be in"):
            bootstrap_summary(counts, None, ref, ref, 1.0, level)
    out = (BootstrapCI * 3)()
    p = counts.ctypes.data_as(C.POINTER(C.c_uint64))
    r = ref.ctypes.data_as(C.POINTER(C.c_uint64))
    assert lib().speq_bootstrap_summary(None, None, 2, 3, r, r, 1.0, 0.9, out) == SPEQ_E_ARG
    assert lib().speq_bootstrap_summary(p, None, 0, 3, r, r, 1.0, 0.9, out) == SPEQ_E_ARG and "replicates" in last_error()
    assert lib().speq_bootstrap_summary(p, None, 1025, 3, r, r, 1.0, 0.9, out) == SPEQ_E_ARG


# ---- the library, without a device ----
NEW_SYMBOLS = ("speq_bootstrap_create", "speq_bootstrap_add_reads_device", "speq_bootstrap_add_reads",
               "speq_bootstrap_finalize", "speq_bootstrap_info", "speq_bootstrap_free", "speq_bootstrap_fastq",
               "speq_bootstrap_weight", "speq_bootstrap_summary")


def test_abi_version_and_symbols():
    assert lib().speq_abi_version() == 8
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (speq_[a-z0-9_]+)$", out, flags=re.M))
    assert not [s for s in NEW_SYMBOLS if s not in exported]
    hdr = open(os.path.join(ROOT, "include", "speq_scan.h")).read()
    assert "#define SPEQ_BOOTSTRAP_MAX_REPLICATES 1024" in hdr and "#define SPEQ_ABI_VERSION 8" in hdr
    assert C.sizeof(BootstrapCI) == 48


def last_error() -> str:
    return lib().speq_last_error().decode()


def test_argument_checks_precede_device_use():
    """No replica exists here, so the replica or the handle is null in every call; the message tells which check refused
    it. Order: params, k, replicates, (the arrays,) the replica or handle; a paired handle's odd record count can only
    be told once there is a handle."""
    L = lib()
    h = C.c_void_p()
    assert L.speq_bootstrap_create(None, None, 10, 1, C.byref(h)) == SPEQ_E_ARG and "null params" in last_error()
    for k in (0, 1025):
        p = ScanParams(k, 30, 0, 0)
        assert L.speq_bootstrap_create(None, C.byref(p), 0, 1, C.byref(h)) == SPEQ_E_ARG
        assert "k must be in [1, 1024]" in last_error()
    p = ScanParams(21, 30, 1, SPEQ_MODE_LOCAL)
    for reps in (0, 1025):
        assert L.speq_bootstrap_create(None, C.byref(p), reps, 1, C.byref(h)) == SPEQ_E_ARG
        assert "replicates must be in [1, 1024]" in last_error()
    for reps in (1, 1024):
        assert L.speq_bootstrap_create(None, C.byref(p), reps, 1, C.byref(h)) == SPEQ_E_ARG
        assert "null device index" in last_error()
    assert not h.value
    off = np.array([0, 4, 2, 6], dtype=np.uint64)
    offp = off.ctypes.data_as(C.POINTER(C.c_uint64))
    assert L.speq_bootstrap_add_reads(None, b"ACGTAC", b"IIIIII", None, 3, 0) == SPEQ_E_ARG
    assert "null offsets" in last_error()
    assert L.speq_bootstrap_add_reads(None, b"ACGTAC", b"IIIIII", offp, 3, 0) == SPEQ_E_ARG
    assert "offsets must be non-decreasing" in last_error()
    off[:] = [0, 2, 4, 6]
    assert L.speq_bootstrap_add_reads(None, None, b"IIIIII", offp, 3, 0) == SPEQ_E_ARG
    assert "null read buffer" in last_error()
    assert L.speq_bootstrap_add_reads(None, b"ACGTAC", b"IIIIII", offp, 3, 5) == SPEQ_E_ARG
    assert "null handle" in last_error()
    assert L.speq_bootstrap_add_reads(None, None, None, None, 0, 0) == SPEQ_E_ARG and "null handle" in last_error()
    assert L.speq_bootstrap_add_reads_device(None, None, None, None, 3, 0, None) == SPEQ_E_ARG
    assert "null buffer" in last_error()
    assert L.speq_bootstrap_add_reads_device(None, 16, 16, 16, 3, 0, None) == SPEQ_E_ARG and "null handle" in last_error()
    assert L.speq_bootstrap_add_reads_device(None, None, None, None, 0, 0, None) == SPEQ_E_ARG
    assert "null handle" in last_error()
    counts = np.zeros(64, dtype=np.uint64)
    cp = counts.ctypes.data_as(C.POINTER(C.c_uint64))
    assert L.speq_bootstrap_finalize(None, cp, None) == SPEQ_E_ARG and "null handle" in last_error()
    assert L.speq_bootstrap_info(None, None, None, None) == SPEQ_E_ARG and "null handle" in last_error()
    assert L.speq_bootstrap_fastq(None, b"x.fq", None, None, 10, 1, 2, cp, None, None) == SPEQ_E_ARG
    assert "null params" in last_error()
    bad = ScanParams(1025, 30, 0, 0)
    assert L.speq_bootstrap_fastq(None, b"x.fq", None, C.byref(bad), 10, 1, 2, cp, None, None) == SPEQ_E_ARG
    assert "k must be in [1, 1024]" in last_error()
    g = ScanParams(21, 30, 0, 0)
    assert L.speq_bootstrap_fastq(None, b"x.fq", None, C.byref(g), 1025, 1, 2, cp, None, None) == SPEQ_E_ARG
    assert "replicates must be in [1, 1024]" in last_error()
    assert L.speq_bootstrap_fastq(None, b"x.fq", None, C.byref(g), 10, 1, 2, cp, None, None) == SPEQ_E_ARG
    assert "null argument" in last_error()
    L.speq_bootstrap_free(None)


def test_cli_bootstrap_options(tmp_path):
    r = subprocess.run([SPEQ, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for opt in ("--bootstrap FILE", "--bootstrap-replicates N", "--bootstrap-seed S", "--bootstrap-level L"):
        assert opt in r.stdout
    assert "EM-refined percentages are not covered" in r.stdout
    (tmp_path / "r.fq").write_text("@r\nACGT\n+\nIIII\n")
    for opt in ("--bootstrap", "--bootstrap-replicates", "--bootstrap-seed", "--bootstrap-level"):
        r = subprocess.run([SPEQ, "scan", "-1", "r.fq", opt], cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "argument parsing error" in r.stderr
        assert "Missing value for option " + opt in r.stderr
    for args in (["--bootstrap-replicates", "0"], ["--bootstrap-replicates", "1025"], ["--bootstrap-level", "1"],
                 ["--bootstrap-level", "0"]):
        r = subprocess.run([SPEQ, "scan", "-1", "r.fq"] + args, cwd=tmp_path, capture_output=True, text=True,
                           timeout=60)
        assert r.returncode == 1 and "Validation failed for option " + args[0] in r.stderr
    # an index-only run does not take it (like the other scan options)
    r = subprocess.run([SPEQ, "index", "--bootstrap", "x"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Unknown option --bootstrap" in r.stderr
