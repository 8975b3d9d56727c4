"""CPU: the model of the bootstrap's per-replicate EM histograms, and the parts of the feature that need no GPU.

tests/bootstrap_em_model.py states what speq_bootstrap_finalize_em must return and how a replicate is refined. Here its
row 0 is compared with em_reference.scan's merged histogram, and the host entry points that take plain arrays run
against it: speq_em_rows_step against em_reference.exact_step (the project's max_relative_deviation <= 1e-9,
tests/test_gpu_em.py's RTOL), speq_em_rows_refine against api.em_refine driven by em_rows_step (same iteration counts,
rtol 1e-12) and, at a fixed number of steps, against the model's refinement (rtol 1e-7, test_gpu_em.py's end-to-end
tolerance; a fixed length removes the stopping test's sensitivity to last-bit differences),
speq_bootstrap_summary_percent against bootstrap_model.summary's statistics, the argument checks and the CLI option."""
import ctypes as C
import os
import re
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest

import bootstrap_em_inputs as bi
import bootstrap_em_model as bem
import bootstrap_model as bm
import em_reference as er
import read_report_inputs as ri
from oracle.oracle import Oracle
from speq_amd import bootstrap_summary_percent, em_refine, em_rows_refine, em_rows_step, lib, unique_to_percent
from speq_amd._lib import LIB_PATH, SPEQ_E_ARG, BootstrapCI, ScanParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEQ = os.path.join(ROOT, "bin", "speq")
RTOL_STEP = 1e-9
SEED, B = 7, 3
ACCURACY = 0.99


def last_error() -> str:
    return lib().speq_last_error().decode()


# ---- the inputs and the model ----
def test_the_70_group_input_is_as_stated():
    h = bi.multi70().hist
    assert (h.n_windows, h.n_intervals, len(h.merged)) == (20_438, 3_937, 603)
    assert max(len(c) for c in h.merged) == 70 and max(h.merged.values()) == 7_270
    hb = bi.base_multi(21, False).hist
    assert (hb.n_windows, hb.n_intervals, len(hb.merged)) == (166_092, 15_591, 4)
    assert er.scan(er.build_index(*ri.many_ref(), 70, ri.MANY_K), 70, ri.MANY_K, *ri.many_reads(), ri.CUTOFF).n_windows == 0


def test_tiles_of_64_distinct_slots_and_of_one_slot_occur():
    """What the slot rounds of the kernel see: (multi-group windows, distinct k-mers, distinct contents) per tile. With
    one row per interval (SPEQ_EM_MERGE_ROWS=0) a tile of 64 distinct k-mers is 64 distinct slots."""
    seq, _, off = bi.reads70()
    tp70 = bem.tile_profiles(bi.index70(), bi.K, seq, off, bi.multi70().hist)
    seq, _, off = ri.base_reads(21)
    tpb = bem.tile_profiles(bi.base_index(21), 21, seq, off, bi.base_multi(21, False).hist)
    assert any(t[:2] == (64, 64) for t in tp70) and any(t[:2] == (64, 64) for t in tpb)
    assert (64, 64, 1) in tp70 and (64, 64, 1) in tpb
    assert max(t[2] for t in tp70) == 63  # merged rows: 63 rounds in one tile


@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
def test_model_row_0_is_the_scans_merged_histogram(paired):
    for mu in (bi.multi70(paired), bi.base_multi(21, paired), bi.base_multi(70, paired)):
        contents = sorted(mu.hist.merged)
        M, missed = bem.mult(mu, contents, SEED, 5)
        assert missed == 0 and M.shape == (6, len(contents))
        assert dict(zip(contents, M[0].tolist())) == mu.hist.merged
        assert (M[1:] != M[0]).any()
        unmerged = bem.mult_by_kmer(mu, SEED, 2)
        assert sorted((c, m[0]) for c, m in unmerged.elements()) == sorted(mu.hist.unmerged.elements())


def test_model_missed_counts_the_windows_outside_the_table():
    seq, qual, off = bi.reads70()
    n = 150
    sub = bem.multi_units(bi.index70(), bi.G70, bi.K, seq[:int(off[n])], qual[:int(off[n])], off[:n + 1], bi.CUTOFF)
    contents = sorted(sub.hist.merged)
    M, missed = bem.mult_in_table(bi.multi70(), sub, contents, SEED, 2)
    assert 0 < missed == bi.multi70().hist.n_windows - int(M[0].sum())
    assert (M[0] >= np.array([sub.hist.merged[c] for c in contents], dtype=np.uint64)).all()


# ---- shared pieces of the library tests ----
@lru_cache(maxsize=None)
def case70():
    """Rows, B + 1 multiplicity rows, the bootstrap's counts and the reference's uniqueness of the 70-group input."""
    mu = bi.multi70()
    contents = sorted(mu.hist.merged)
    M, _ = bem.mult(mu, contents, SEED, B)
    ref = bi.ref70()
    un = bm.units(bi.index70(), bi.G70, bi.K, *bi.reads70(), bi.CUTOFF, False, False)
    counts, _ = bm.replicates(un, SEED, B)
    u_ref, tot_ref = Oracle(ref.records, ref.groups, bi.G70, bi.K).ref_unique()
    group_counts = [1 + g % 3 for g in range(bi.G70)]
    return contents, M, counts, None, u_ref, tot_ref, group_counts, 1.0 / ACCURACY ** bi.K


@lru_cache(maxsize=None)
def case_base_local():
    k = 21
    mu = bi.base_multi(k, True)
    contents = sorted(mu.hist.merged)
    M, _ = bem.mult(mu, contents, SEED, B)
    ref = ri.base_ref()
    un = bm.units(bi.base_index(k), 3, k, *ri.base_reads(k), ri.CUTOFF, True, True)
    counts, w = bm.replicates(un, SEED, B)
    u_ref, tot_ref = Oracle(ref.records, ref.groups, 3, k).ref_unique()
    return contents, M, counts, w, u_ref, tot_ref, [1, 1, 1], 1.0


def percents(G: int):
    rng = np.random.default_rng(11)
    zeros = rng.uniform(0.5, 3.0, G)
    zeros[::3] = 0.0
    return {"uniform": np.full(G, 100.0 / G), "random": rng.uniform(0.0, 5.0, G), "zeros": zeros}


# ---- speq_em_rows_step ----
@pytest.mark.parametrize("case", [case70, case_base_local], ids=["g70", "base"])
def test_rows_step_against_the_exact_step(case):
    contents, M, counts, _, _, _, group_counts, _ = case()
    G = len(group_counts)
    ptr, grp, cnt = bem.csr(contents)
    for b in range(B + 1):
        unique = counts[b, 2:]
        merged = dict(zip(contents, (int(m) for m in M[b])))
        for which, p in percents(G).items():
            got = em_rows_step(G, ptr, grp, cnt, M[b], p, group_counts, unique)
            dev = er.max_relative_deviation(got, er.exact_step(p, group_counts, unique, merged))
            assert dev <= RTOL_STEP, (b, which, dev)
    assert (em_rows_step(G, ptr, grp, cnt, M[1], p, group_counts, unique) !=
            em_rows_step(G, ptr, grp, cnt, M[2], p, group_counts, unique)).any()


def literal_step(contents, m_row, percent, group_counts, unique):
    """The reference's pass in f64, every group of every window evaluated, zero terms included (IEEE semantics)."""
    G = len(group_counts)
    p, n = np.asarray(percent, dtype=np.float64), np.asarray(group_counts, dtype=np.float64)
    nxt = np.zeros(G)
    windows = [(((g, 1),), int(unique[g])) for g in range(G) if int(unique[g])] + list(zip(contents, (int(m) for m in m_row)))
    with np.errstate(all="ignore"):
        for content, m in windows:
            h = np.zeros(G)
            for g, c in content:
                h[g] = c
            a = h * p / n
            norm = np.float64(0.0)
            for g in range(G):
                norm = norm + a[g]
            if norm > 0.0:
                nxt += np.float64(m) * (a / norm)
    return nxt


def test_rows_step_dense_path_with_a_group_count_of_0():
    contents, M, counts, _, _, _, _, _ = case_base_local()
    ptr, grp, cnt = bem.csr(contents)
    for gc, p in (([1, 0, 2], [30.0, 0.0, 70.0]), ([1, 0, 2], [30.0, 20.0, 50.0]), ([2, 1, 1], [np.inf, 1.0, 2.0])):
        for b in (0, 2):
            got = em_rows_step(3, ptr, grp, cnt, M[b], p, gc, counts[b, 2:])
            exp = literal_step(contents, M[b], p, gc, counts[b, 2:])
            np.testing.assert_allclose(got, exp, rtol=RTOL_STEP, atol=0, equal_nan=True)


# ---- speq_em_rows_refine ----
def refine_by_python(case, precision, max_iterations):
    contents, M, counts, w, u_ref, tot_ref, group_counts, scale = case
    G = len(group_counts)
    ptr, grp, cnt = bem.csr(contents)
    out = []
    for b in range(len(M)):
        def step(p, b=b):
            return em_rows_step(G, ptr, grp, cnt, M[b], p, group_counts, counts[b, 2:])
        out.append(bem.refine_row(contents, M[b], counts[b], None if w is None else w[b], u_ref, tot_ref, group_counts,
                                  scale, precision, max_iterations, step=step))
    return out


def refine_by_library(case, precision, max_iterations):
    contents, M, counts, w, u_ref, tot_ref, group_counts, scale = case
    ptr, grp, cnt = bem.csr(contents)
    return em_rows_refine(len(group_counts), ptr, grp, cnt, M, counts, w, u_ref, tot_ref, group_counts, scale,
                          precision, max_iterations)


@pytest.mark.parametrize("case", [case70, case_base_local], ids=["g70", "base"])
def test_rows_refine_is_the_loop_over_rows_step(case):
    got_p, got_it = refine_by_library(case(), 1e-6, 1000)
    exp = refine_by_python(case(), 1e-6, 1000)
    assert got_it.tolist() == [it for _, it in exp] and min(got_it) >= 2
    for b, (p, _) in enumerate(exp):
        np.testing.assert_allclose(got_p[b], p, rtol=1e-12, atol=0)
    assert (got_p[1] != got_p[0]).any()
    # stopped by max_iterations
    got_p, got_it = refine_by_library(case(), 1e-6, 2)
    exp = refine_by_python(case(), 1e-6, 2)
    assert got_it.tolist() == [2] * (B + 1)
    for b, (p, _) in enumerate(exp):
        np.testing.assert_allclose(got_p[b], p, rtol=1e-12, atol=0)
    # no step at all: the initial percentages
    got_p, got_it = refine_by_library(case(), 1e-6, 0)
    assert got_it.tolist() == [0] * (B + 1)
    _, M, counts, w, u_ref, tot_ref, _, scale = case()
    ut = w[1] if w is not None else counts[1, 2:].astype(np.float64) * scale
    assert got_p[1].tolist() == unique_to_percent(ut, int(counts[1, 0]), u_ref.astype(np.float64), tot_ref.astype(np.float64))


@pytest.mark.parametrize("case", [case70, case_base_local], ids=["g70", "base"])
def test_rows_refine_at_12_steps_against_the_models_refinement(case):
    contents, M, counts, w, u_ref, tot_ref, group_counts, scale = case()
    got_p, got_it = refine_by_library(case(), 0.0, 12)
    assert got_it.tolist() == [12] * (B + 1)
    for b in range(B + 1):
        p, it = bem.refine_row(contents, M[b], counts[b], None if w is None else w[b], u_ref, tot_ref, group_counts,
                               scale, 0.0, 12)
        assert it == 12
        np.testing.assert_allclose(got_p[b], p, rtol=1e-7, atol=0)


def test_rows_refine_an_all_zero_row_and_no_rows():
    contents, M, counts, w, u_ref, tot_ref, group_counts, scale = case70()
    ptr, grp, cnt = bem.csr(contents)
    c, m = counts.copy(), M.copy()
    c[2], m[2] = 0, 0
    got_p, got_it = em_rows_refine(bi.G70, ptr, grp, cnt, m, c, None, u_ref, tot_ref, group_counts, scale)
    ref_p, ref_it = refine_by_library(case70(), 1e-6, 1000)
    assert got_it[2] == 0 and not got_p[2].any()
    for b in (0, 1, 3):
        assert got_it[b] == ref_it[b] and got_p[b].tolist() == ref_p[b].tolist()
    # a histogram without rows: only the single-group windows
    none = np.zeros((B + 1, 0), dtype=np.uint64)
    got_p, got_it = em_rows_refine(bi.G70, np.zeros(1, dtype=np.uint64), [], [], none, counts, None, u_ref, tot_ref,
                                   group_counts, scale)
    assert (got_it >= 1).all() and np.isfinite(got_p).all()


CHILD = """
import os, sys
os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})
os.environ["OMP_NUM_THREADS"] = "1"
sys.path[:0] = [sys.argv[1], os.path.join(sys.argv[1], "tests")]
import numpy as np
from speq_amd import em_rows_refine
z = np.load(sys.argv[2])
p, it = em_rows_refine(int(z["G"]), z["ptr"], z["grp"], z["cnt"], z["M"], z["counts"], None, z["u_ref"], z["tot_ref"],
                       z["gc"], float(z["scale"]), 1e-6, 1000)
np.savez(sys.argv[3], p=p, it=it)
"""


def test_rows_refine_does_not_depend_on_the_thread_count(tmp_path):
    """A child process bound to one CPU before the library loads has a worker pool of one thread (the pool is sized by
    the CPUs the process may run on): the same bits as here."""
    contents, M, counts, _, u_ref, tot_ref, group_counts, scale = case70()
    Mb, cb = np.concatenate([M] * 5), np.concatenate([counts] * 5)  # 20 rows: more rows than most pools have threads
    ptr, grp, cnt = bem.csr(contents)
    here_p, here_it = em_rows_refine(bi.G70, ptr, grp, cnt, Mb, cb, None, u_ref, tot_ref, group_counts, scale)
    assert here_p[:B + 1].tobytes() == refine_by_library(case70(), 1e-6, 1000)[0].tobytes()
    assert here_p[B + 1:2 * B + 2].tobytes() == here_p[:B + 1].tobytes()
    np.savez(tmp_path / "in.npz", G=bi.G70, ptr=ptr, grp=grp, cnt=cnt, M=Mb, counts=cb, u_ref=u_ref, tot_ref=tot_ref,
             gc=np.array(group_counts), scale=scale)
    subprocess.run([sys.executable, "-c", CHILD, ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], check=True,
                   timeout=120)
    z = np.load(tmp_path / "out.npz")
    assert z["p"].tobytes() == here_p.tobytes() and z["it"].tolist() == here_it.tolist()


# ---- speq_bootstrap_summary_percent ----
def test_summary_percent_against_the_models_statistics():
    rng = np.random.default_rng(3)
    Bs, G = 64, 5
    counts = rng.integers(1, 1000, (Bs + 1, G + 2)).astype(np.uint64)
    counts[[5, 17], 0] = 0  # replicates without a passing window are left out
    u_ref, tot_ref = rng.integers(1, 50, G), rng.integers(50, 100, G)
    tot_ref[4] = 0
    for level in (0.95, 0.5):
        exp = bm.summary(counts, None, u_ref, tot_ref, 1.25, level)
        with np.errstate(all="ignore"):
            percent = np.array([[bm._percent(counts, None, b, g, u_ref, tot_ref, 1.25) for g in range(G)]
                                for b in range(Bs + 1)])
        used = counts[:, 0] != 0
        assert bootstrap_summary_percent(percent, used, level=level) == exp
        est = rng.uniform(0, 10, G)
        got = bootstrap_summary_percent(percent, used, estimate=est, level=level)
        assert [ci["estimate"] for ci in got] == est.tolist()
        assert [{**ci, "estimate": 0} for ci in got] == [{**ci, "estimate": 0} for ci in exp]
    none = bootstrap_summary_percent(percent, np.zeros(Bs + 1, dtype=bool))
    assert all(ci["used"] == 0 and ci["mean"] == ci["se"] == ci["lo"] == ci["hi"] == 0.0 for ci in none)
    one = bootstrap_summary_percent(percent[:2], [0, 1])
    assert all(ci["used"] == 1 and ci["se"] == 0.0 and ci["lo"] == ci["hi"] == ci["mean"] for ci in one)


# ---- the library, without a device ----
NEW_SYMBOLS = ("speq_em_intervals", "speq_em_rows_step", "speq_em_rows_refine", "speq_bootstrap_summary_percent",
               "speq_bootstrap_attach_em", "speq_bootstrap_em_info", "speq_bootstrap_finalize_em",
               "speq_bootstrap_em_fastq")


def test_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (speq_[a-z0-9_]+)$", out, flags=re.M))
    assert not [s for s in NEW_SYMBOLS if s not in exported]
    hdr = open(os.path.join(ROOT, "include", "speq_scan.h")).read()
    assert not [s for s in NEW_SYMBOLS if "int " + s + "(" not in hdr]


def test_argument_checks():
    L = lib()
    u64p, u32p, dp = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    n = C.c_uint64()
    assert L.speq_em_intervals(None, C.byref(n), None, None) == SPEQ_E_ARG and "not finalized" in last_error()
    ptr = np.array([0, 2, 3], dtype=np.uint64)
    grp = np.array([0, 1, 2], dtype=np.uint32)
    cnt = np.ones(3, dtype=np.uint32)
    mult = np.ones(2, dtype=np.uint64)
    p, nxt = np.ones(3), np.zeros(3)
    gc = np.ones(3, dtype=np.int32)
    uq = np.ones(3, dtype=np.uint64)
    a = dict(ptr=ptr.ctypes.data_as(u64p), grp=grp.ctypes.data_as(u32p), cnt=cnt.ctypes.data_as(u32p),
             mult=mult.ctypes.data_as(u64p), p=p.ctypes.data_as(dp), gc=gc.ctypes.data_as(C.POINTER(C.c_int32)),
             uq=uq.ctypes.data_as(u64p), nxt=nxt.ctypes.data_as(dp))

    def step(G=3, n_rows=2, **kw):
        v = {**a, **kw}
        return L.speq_em_rows_step(G, n_rows, v["ptr"], v["grp"], v["cnt"], v["mult"], v["p"], v["gc"], v["uq"], v["nxt"])
    assert step() == 0
    for name in ("mult", "p", "gc", "uq", "nxt"):
        assert step(**{name: None}) == SPEQ_E_ARG and "null argument" in last_error(), name
    assert step(ptr=None) == SPEQ_E_ARG and "null row_ptr" in last_error()
    assert step(grp=None) == SPEQ_E_ARG and "null entries" in last_error()
    assert step(G=2) == SPEQ_E_ARG and "not below G" in last_error()
    bad = np.array([0, 3, 2], dtype=np.uint64)
    assert step(ptr=bad.ctypes.data_as(u64p)) == SPEQ_E_ARG and "must ascend" in last_error()
    bad[:] = [1, 2, 3]
    assert step(ptr=bad.ctypes.data_as(u64p)) == SPEQ_E_ARG and "row_ptr[0]" in last_error()

    counts = np.ones((2, 5), dtype=np.uint64)
    m2 = np.ones((2, 2), dtype=np.uint64)
    out, its = np.zeros((2, 3)), np.zeros(2, dtype=np.uint32)
    r = dict(mult=m2.ctypes.data_as(u64p), counts=counts.ctypes.data_as(u64p), u_ref=a["uq"], tot_ref=a["uq"], gc=a["gc"],
             out=out.ctypes.data_as(dp), its=its.ctypes.data_as(u32p), ptr=a["ptr"])

    def refine(G=3, **kw):
        v = {**r, **kw}
        return L.speq_em_rows_refine(G, 2, v["ptr"], a["grp"], a["cnt"], 1, v["mult"], v["counts"], None, 1.0,
                                     v["u_ref"], v["tot_ref"], v["gc"], 1e-6, 10, v["out"], v["its"])
    assert refine() == 0
    for name in ("mult", "counts", "u_ref", "tot_ref", "gc", "out", "its"):
        assert refine(**{name: None}) == SPEQ_E_ARG and "null argument" in last_error(), name
    assert refine(ptr=None) == SPEQ_E_ARG and "null row_ptr" in last_error()
    assert refine(G=2) == SPEQ_E_ARG and "not below G" in last_error()
    with pytest.raises(ValueError):
        em_rows_refine(3, ptr, grp, cnt, m2[:1], counts, None, uq, uq, gc)
    with pytest.raises(ValueError):
        em_rows_step(3, ptr[:2], grp, cnt, mult[:1], p, gc, uq)

    ci = (BootstrapCI * 3)()
    pm = np.ones((3, 3))
    used = np.ones(3, dtype=np.uint8)
    pp, up = pm.ctypes.data_as(dp), used.ctypes.data_as(C.POINTER(C.c_uint8))
    assert L.speq_bootstrap_summary_percent(pp, None, up, 2, 3, 0.9, ci) == 0
    assert L.speq_bootstrap_summary_percent(None, None, up, 2, 3, 0.9, ci) == SPEQ_E_ARG and "null" in last_error()
    assert L.speq_bootstrap_summary_percent(pp, None, None, 2, 3, 0.9, ci) == SPEQ_E_ARG
    assert L.speq_bootstrap_summary_percent(pp, None, up, 2, 3, 0.9, None) == SPEQ_E_ARG
    for reps in (0, 1025):
        assert L.speq_bootstrap_summary_percent(pp, None, up, reps, 3, 0.9, ci) == SPEQ_E_ARG
        assert "replicates must be in [1, 1024]" in last_error()
    for level in (0.0, 1.0, float("nan")):
        assert L.speq_bootstrap_summary_percent(pp, None, up, 2, 3, level, ci) == SPEQ_E_ARG and "level" in last_error()

    assert L.speq_bootstrap_attach_em(None, None) == SPEQ_E_ARG and "null argument" in last_error()
    assert L.speq_bootstrap_em_info(None, None, None) == SPEQ_E_ARG and "null handle" in last_error()
    assert L.speq_bootstrap_finalize_em(None, None, None) == SPEQ_E_ARG and "null handle" in last_error()
    g = ScanParams(21, 30, 0, 0)
    cp = counts.ctypes.data_as(u64p)
    assert L.speq_bootstrap_em_fastq(None, None, b"x.fq", None, C.byref(g), 10, 1, 2, cp, None, cp, None, None) == SPEQ_E_ARG
    assert "null histogram" in last_error()


def test_cli_bootstrap_em_option(tmp_path):
    r = subprocess.run([SPEQ, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--bootstrap-em FILE" in r.stdout
    (tmp_path / "r.fq").write_text("@r\nACGT\n+\nIIII\n")
    r = subprocess.run([SPEQ, "scan", "-1", "r.fq", "--bootstrap-em"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1 and "Missing value for option --bootstrap-em" in r.stderr
    # the shared options are validated with it, and an existing FILE needs --force like every output
    r = subprocess.run([SPEQ, "scan", "-1", "r.fq", "--bootstrap-em", "ci.tsv", "--bootstrap-replicates", "0"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Validation failed for option --bootstrap-replicates" in r.stderr
    r = subprocess.run([SPEQ, "index", "--bootstrap-em", "x"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Unknown option --bootstrap-em" in r.stderr
