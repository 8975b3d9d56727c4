"""GPU: every scan path on references of short, empty and tiny contigs (tests/frag_refs.py), against the CPU oracle.

What depends on where texts start and end, and no other test reaches below 300 bases per text: the END / SENT classes
of k_ax_classify and the END padding of k_ax_pack (several texts in one granule, positions past n), the text words
ax_text_words loads past a position (past n for a tiny collection), the text lookups by binary search (k_ax_insert,
k_bwt), runs of k_scan_ax that stop at an END window a dozen times per read, the substitution bitmap's "every window
over x lies inside x's text", the flattened reference windows of the .dat pass and of k_ktab_keys (texts and a whole
group without a window), and the planes of an index smaller than one 96-position block.

tests/test_frag_refs_cpu.py validates the inputs and the oracle on them without a GPU. Integer counters bit-exact, W to
test_gpu_parity.W_RTOL (inside check_all), EM rows by the criteria of tests/test_gpu_em_rows.py."""
import os
import subprocess
from functools import lru_cache

import numpy as np
import pytest

import byte_reads as br
import em_cases as ec
import em_reference as er
import frag_refs as fr
import test_gpu_em_rows as em_rows
from oracle.oracle import Oracle
from speq_amd import DeviceIndex, EmHistogram, FmIndex, unique_to_percent
from test_cli import SPEQ, _parse_vec
from test_gpu_ax import distinct_kmers
from test_gpu_build import assert_same
from test_gpu_shapes import check_all
from test_gpu_sproof import brute_force

pytestmark = pytest.mark.gpu

KS = [21, 33, 70]
BUILD = dict(prefix_q=8, pair_steps=True, triple_steps=True)
TINY_BUILD = dict(prefix_q=3, pair_steps=True, triple_steps=True)
_cache: dict = {}


def frag_env(k):
    """(Fragmented, FmIndex, DeviceIndex, Oracle) of k, kept for the module."""
    if k not in _cache:
        f = fr.fragmented(k)
        idx = FmIndex.build(f.records, f.groups, f.G, **BUILD)
        _cache[k] = (f, idx, DeviceIndex(idx), Oracle(f.records, f.groups, f.G, k))
    return _cache[k]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    for _, _, dev, _ in _cache.values():
        dev.close()
    _cache.clear()


def default_scan_equals(dev, orc, rd, k, paired=False):
    """One scan with the default tuning through each entry point; the anchor kernel must have taken it."""
    exp = orc.scan(rd.seq, rd.qual, rd.offsets, paired=paired)
    got = dev.scan(rd.seq.tobytes(), rd.qual.tobytes(), rd.offsets, k=k, paired=paired)
    assert dev.tuning("last_kernel") == 3  # k_scan_ax
    assert (got.total, got.ambiguous, got.unique.tolist()) == (exp[0], exp[1], exp[2].tolist())
    got = br.device_scan(dev, rd, k, 30, paired, False)
    assert dev.tuning("last_kernel") == 3
    assert (got[0], got[1], got[2].tolist()) == (exp[0], exp[1], exp[2].tolist())
    return exp


def check_dat(dev, orc, k):
    ou, ot = orc.ref_unique()
    u, t = dev.count_unique_kmers_per_group(k)
    assert np.array_equal(u, ou) and np.array_equal(t, ot), (k, u, ou, t, ot)
    for W in (2, 3, 8):
        parts = [dev.count_unique_kmers_per_group_shard(k, s, W) for s in range(W)]
        assert np.array_equal(sum(p[0] for p in parts), ou) and np.array_equal(sum(p[1] for p in parts), ot), (k, W)
    return u, t


# ---- 1. scans
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_scans_equal_the_oracle(k, paired):
    """Four kernels, global and local, device buffers and host reads (test_gpu_shapes.check_all)."""
    f, _, dev, orc = frag_env(k)
    rd = fr.reads(k, paired)
    exp = check_all(dev, orc, rd, k, paired)
    assert exp[0] > 0 and exp[2][:fr.GENOMES].all() and exp[2][fr.GENOMES] == 0 and exp[1] > 0
    default_scan_equals(dev, orc, rd, k, paired)


def test_scan_k128_reads_of_250():
    """The widest compare (four 2-bit words per k-mer) and reads of more than one 192-base segment."""
    k = 128
    f, _, dev, orc = frag_env(k)
    rd = fr.reads(k, read_len=250)
    exp = default_scan_equals(dev, orc, rd, k)
    assert exp[0] > 0 and exp[2][:fr.GENOMES].all() and exp[2][fr.GENOMES] == 0


# ---- 2. the .dat pass
@pytest.mark.parametrize("k", KS)
def test_dat_pass_with_a_group_without_windows(k):
    f, _, dev, orc = frag_env(k)
    u, t = check_dat(dev, orc, k)
    assert t[fr.GENOMES] == 0 and u[fr.GENOMES] == 0 and t[:fr.GENOMES].all()
    rd = fr.reads(k)
    T, _, U, _ = orc.scan(rd.seq, rd.qual, rd.offsets)
    p = unique_to_percent(U, T, u, t)
    assert p[fr.GENOMES] == 0.0 and np.isfinite(p).all() and all(x > 0 for x in p[:fr.GENOMES])


# ---- 3. the per-k structures
@pytest.mark.parametrize("k", KS + [128])
def test_distinct_kmers(k):
    f, _, dev, _ = frag_env(k)
    assert dev.prepare(k)["distinct_kmers"] == distinct_kmers(f.records, k)


@pytest.fixture(scope="module", params=[21, 33])
def bitmap_case(request):
    k = request.param
    f, idx, dev, _ = frag_env(k)
    dev.prepare(k)
    return (dev.sproof_bitmap(k),) + brute_force(idx.array("text", np.uint8), k)


def test_bitmap_sound(bitmap_case):
    S, all_valid, provable = bitmap_case
    assert not (S & ~all_valid).any(), "S = 1 within k - 1 of a text end or an N"
    assert not (S & ~provable).any(), "S = 1 where a substituted k-mer is indexed"


def test_bitmap_complete(bitmap_case):
    S, all_valid, provable = bitmap_case
    # (not degenerate: positions at least k - 1 from both ends of their text are a quarter of this text, 50-59 % by
    # the brute force, and most of them are provable)
    assert all_valid.sum() > 0.25 * len(S) and provable.sum() > 0.5 * all_valid.sum()
    assert not all_valid.all() and (all_valid & ~provable).any()
    assert not (provable & ~S).any(), "S = 0 at a provable position"


# ---- 4. the index built on the GPU
@pytest.mark.parametrize("k", KS)
def test_gpu_built_index_is_the_host_index_and_scans_alike(k):
    f, _, _, orc = frag_env(k)
    b = assert_same(f.records, f.groups, f.G, **BUILD)
    dev = DeviceIndex(b)
    default_scan_equals(dev, orc, fr.reads(k), k)
    dev.close()


# ---- 5. EM histograms
@lru_cache(maxsize=None)
def em_expected(k, paired):
    """The exact histogram of tests/em_reference.py for fr.reads(k, paired) on fr.fragmented(k)."""
    f, rd = fr.fragmented(k), fr.reads(k, paired)
    return er.scan(er.build_index(f.records, f.groups, f.G, k), f.G, k, rd.seq, rd.qual, rd.offsets, cutoff=ec.CUTOFF,
                   paired=paired)


EM_CASES = [(k, kernel, paired) for k, kernels in ((21, (ec.AX, ec.KT, ec.LF)), (70, (ec.AX,))) for kernel in kernels
            for paired in (False, True)]


@pytest.mark.parametrize("k,kernel,paired", EM_CASES, ids=[f"k{k}-{kn}-{'pe-local' if p else 'se-global'}"
                                                           for k, kn, p in EM_CASES])
def test_em_rows_equal_the_exact_reference(k, kernel, paired, monkeypatch):
    """The criteria of tests/test_gpu_em_rows.py::test_rows_equal_the_exact_reference, with its own checks: counters
    against the oracle, rows unmerged and merged and info() equal to em_reference exactly, and one step per
    em_cases.percents against the oracle's literal pass (RTOL) and within check_steps' bound of the exact step.
    Single-end scans are global, paired ones local."""
    local = paired
    f, idx, _, orc = frag_env(k)
    rd, h = fr.reads(k, paired), em_expected(k, paired)
    counts = tuple(g % 3 + 1 for g in range(f.G))  # the "(count)" of each groupings line
    exp = orc.scan(rd.seq, rd.qual, rd.offsets, phred_cutoff=ec.CUTOFF, paired=paired, local=local)

    def check_counters(got):
        assert (got[0], got[1], got[2].tolist()) == (exp[0], exp[1], exp[2].tolist())
        if local:
            np.testing.assert_allclose(got[3], exp[3], rtol=1e-10, atol=0)

    dev = DeviceIndex(idx)
    dev.tune(**ec.TUNE[kernel])
    monkeypatch.setenv("SPEQ_EM_MERGE_ROWS", "0")  # one row per interval
    em = EmHistogram(dev)
    check_counters(em_rows.scan_into(em, rd, k, paired, local))
    assert dev.tuning("last_kernel") in ec.KERNEL_CODES[kernel]
    em.finalize()
    assert em.info() == (h.n_intervals, h.n_entries, h.n_windows)
    em_rows.check_rows_unmerged(em, h)
    em.close()
    monkeypatch.delenv("SPEQ_EM_MERGE_ROWS")  # merged (the default)
    em = EmHistogram(dev)
    got = em_rows.scan_into(em, rd, k, paired, local)
    check_counters(got)
    em.finalize()
    assert em.info() == (h.n_intervals, h.n_entries, h.n_windows)
    em_rows.check_rows_merged(em, h)
    assert h.n_windows > 100 and h.n_intervals > 50 and h.unique[fr.GENOMES] == 0
    bound = (h.n_intervals + 2 * f.G + 80) * em_rows.U
    for which, percent in ec.percents(f.G).items():
        step = em.step(percent, counts, got[2])
        lit = orc.em_pass(rd.seq, rd.qual, rd.offsets, percent, counts, phred_cutoff=ec.CUTOFF, paired=paired,
                          local=local)
        np.testing.assert_allclose(step, lit, rtol=em_rows.RTOL, atol=0, err_msg=which)
        dev_ = er.max_relative_deviation(step, er.exact_step(percent, counts, h.unique, h.merged))
        print(f"k={k} {kernel} {which}: deviation from the exact step {dev_:.3e}, bound {bound:.3e}")
        assert dev_ <= bound, (which, dev_, bound)
    em.close()
    dev.close()


# ---- 6. tiny collections
@pytest.mark.parametrize("case", fr.TINY, ids=fr.TINY_IDS)
def test_tiny_collections(case):
    records, groups, G, k, rd = case
    b = assert_same(records, groups, G, **TINY_BUILD)
    orc = Oracle(records, groups, G, k)
    for idx in (FmIndex.build(records, groups, G, **TINY_BUILD), b):
        dev = DeviceIndex(idx)
        assert dev.prepare(k)["distinct_kmers"] == distinct_kmers(records, k)
        check_all(dev, orc, rd, k, False)
        default_scan_equals(dev, orc, rd, k)
        check_dat(dev, orc, k)
        dev.close()


# ---- 7. the CLI
def test_cli_scan_k70(tmp_path):
    """`speq index` and `speq scan -k 70` on the non-empty records (a FASTA record without bases is not written), global
    (--fixed-accuracy 1: the unique totals are U) and local: the printed .dat vectors, counters and percentages are
    those of the oracle's counters (printed with six digits, as tests/test_cli.py compares them), and the group
    without a window prints 0."""
    k = 70
    f = fr.fragmented(k)
    keep = [i for i, r in enumerate(f.records) if r]
    records, groups = [f.records[i] for i in keep], [f.groups[i] for i in keep]
    assert sorted(groups) == groups and set(groups) == set(range(f.G))
    fasta = []
    for i, r in enumerate(records):
        fasta += [f">contig{i}"] + [r[p:p + 60].decode() for p in range(0, len(r), 60)]
    (tmp_path / "refs.fa").write_text("\n".join(fasta) + "\n")
    first = [groups.index(g) for g in range(f.G)] + [len(groups)]
    (tmp_path / "groups.txt").write_text(
        "".join(f"G{g}({g % 3 + 1}): {first[g]}-{first[g + 1] - 1}\n" for g in range(f.G)))
    rd = fr.reads(k)
    (tmp_path / "reads.fq").write_text(rd.fastq_text())
    orc = Oracle(records, groups, f.G, k)
    ou, ot = orc.ref_unique()
    assert ot[fr.GENOMES] == 0

    def run(args):
        return subprocess.run([SPEQ] + args, cwd=tmp_path, capture_output=True, text=True, timeout=300)

    r = run(["index", "-r", "refs.fa", "-g", "groups.txt", "-x", "ref", "-o", "i.txt"])
    assert r.returncode == 0, r.stderr
    for mode in ("global", "local"):
        T, amb, U, W = orc.scan(rd.seq, rd.qual, rd.offsets, local=mode == "local")
        r = run(["scan", "-1", "reads.fq", "-x", "ref", "-k", str(k), "-o", f"{mode}.txt"] +
                (["--fixed-accuracy", "1"] if mode == "global" else []))
        assert r.returncode == 0, r.stderr
        lines = r.stderr.strip().split("\n")
        if mode == "global":  # the first scan computes the .dat pass
            assert _parse_vec(lines[0]) == ou.tolist() and _parse_vec(lines[1]) == ot.tolist()
            lines = lines[2:]
            assert _parse_vec(lines[1]) == U.tolist()
        totals = U if mode == "global" else W
        percent = unique_to_percent(totals, T, ou, ot)
        got = _parse_vec(lines[0])
        np.testing.assert_allclose(got, percent, rtol=1e-5, atol=0)
        assert got[fr.GENOMES] == 0.0 and all(x > 0 for x in got[:fr.GENOMES])
        assert [ln for ln in lines if "\t" in ln][0] == f"{T}\t{amb}"
        out = [float(ln.split("\t")[1]) for ln in (tmp_path / f"{mode}.txt").read_text().strip().split("\n")]
        assert len(out) == f.G and out[fr.GENOMES] == 0.0 and np.isfinite(out).all() and all(x > 0 for x in out[:4])
    assert os.path.exists(tmp_path / f"ref_{k}mer.dat")
