"""GPU: the duplicate-read pass (speq_dedup_*, `speq scan --dedup`) against the pure-Python model
(tests/dedup_model.py) and the C oracle.

Representatives, statistics, masked bytes, counts and EM rows are integers: every comparison of them is exact. The local
weights of a deduplicated scan are compared with the oracle's over the removed reads within the bound tests/test_gpu_ax.py
states for two sums of the same windows: each window within 3 k 2^-53 relative, and a group's sum of n_g windows within
another (2 n_g + 2) 2^-53 for the order of the additions. tests/test_dedup_cpu.py checks, without a GPU, that no input
here holds a fingerprint collision and that the masked scan is the scan of the removed reads."""
import os
import shutil
import subprocess
from functools import lru_cache

import numpy as np
import pytest

import dedup_inputs as di
import dedup_model as dm
import em_reference as er
import read_report_inputs as ri
from golden_io import Case
from oracle.oracle import Oracle
from speq_amd import (Dedup, DeviceIndex, EmHistogram, FmIndex, SpeqError, em_refine, file_to_map, unique_to_percent)
from speq_amd._lib import SPEQ_E_ARG

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEQ = os.path.join(ROOT, "bin", "speq")
FULL = dict(pair_steps=True, triple_steps=True, label_table=True)
FLAVOURS = pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])


@lru_cache(maxsize=None)
def base_index() -> FmIndex:
    ref = ri.base_ref()
    return FmIndex.build(ref.records, ref.groups, 3, prefix_q=8, **FULL)


@pytest.fixture(scope="module")
def dev():
    d = DeviceIndex(base_index())
    yield d
    d.close()


@lru_cache(maxsize=None)
def model(k: int, paired: bool):
    seq, _, off = di.reads(k, paired)
    rep = dm.rep_fingerprint(seq, off, paired)
    return rep, dm.stats(rep)


def assert_stats(got, exp: dict):
    assert (got.units, got.distinct, got.max_multiplicity) == (exp["units"], exp["distinct"], exp["max_multiplicity"])
    np.testing.assert_array_equal(got.mult_hist, exp["mult_hist"])
    assert got.duplicates == exp["units"] - exp["distinct"]


def to_device(rd):
    import torch
    seq, qual, off = rd
    return (torch.from_numpy(np.frombuffer(seq, np.uint8).copy()).cuda(),
            torch.from_numpy(np.frombuffer(qual, np.uint8).copy()).cuda(),
            torch.from_numpy(np.asarray(off).astype(np.int64)).cuda())


def expect_arg_error(f, *a, **kw):
    with pytest.raises(SpeqError) as e:
        f(*a, **kw)
    assert e.value.code == SPEQ_E_ARG, e.value


# ---- representatives and statistics ----
@FLAVOURS
def test_representatives_and_statistics_however_the_units_are_added(dev, paired):
    import torch
    k = 21
    rd = di.reads(k, paired)
    rep, st = model(k, paired)
    n, per = len(rep), 2 if paired else 1
    assert st["distinct"] < n and st["max_multiplicity"] == 4096

    def check(dd):
        assert_stats(dd.finalize(), st)
        np.testing.assert_array_equal(dd.representatives(0, n), rep)
        np.testing.assert_array_equal(dd.representatives(n // 3, n // 2), rep[n // 3:n // 3 + n // 2])
        assert len(dd.representatives(n, 0)) == 0
        dd.close()

    # one call, host buffers
    dd = Dedup(dev, paired)
    dd.add(rd[0], rd[2])
    check(dd)
    # three calls out of order, each with its first unit
    cuts = [0, n // 3 + 1, 2 * n // 3, n]
    dd = Dedup(dev, paired)
    for i in (2, 0, 1):
        s, _, o = di.split(rd, per * cuts[i], per * cuts[i + 1])
        dd.add(s, o, first_unit=cuts[i])
    check(dd)
    # device buffers: one call, and two halves on two streams
    d_seq, _, d_off = to_device(rd)
    dd = Dedup(dev, paired)
    dd.add_device(d_seq.data_ptr(), d_off.data_ptr(), per * n)
    check(dd)
    dd = Dedup(dev, paired)
    half = n // 2 + 1
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    dd.add_device(d_seq.data_ptr(), d_off.data_ptr() + 8 * per * half, per * (n - half), first_unit=half,
                  stream=s1.cuda_stream)
    dd.add_device(d_seq.data_ptr(), d_off.data_ptr(), per * half, stream=s0.cuda_stream)
    check(dd)


def test_units_on_both_sides_of_a_storage_chunk(dev):
    """The handle's storage grows in chunks of 65,536 units: adds that end at, start at and straddle the boundary."""
    rd = di.chunk_reads()
    rep = dm.rep_fingerprint(rd[0], rd[2], False)
    n = len(rep)
    dd = Dedup(dev)
    for a, b in ((65_536, n), (60_000, 65_536), (0, 60_000)):
        s, _, o = di.split(rd, a, b)
        dd.add(s, o, first_unit=a)
    assert_stats(dd.finalize(), dm.stats(rep))
    np.testing.assert_array_equal(dd.representatives(0, n), rep)
    dd.close()
    dd = Dedup(dev)
    for a, b in ((0, 65_000), (65_000, n)):
        s, _, o = di.split(rd, a, b)
        dd.add(s, o, first_unit=a)
    assert_stats(dd.finalize(), dm.stats(rep))
    np.testing.assert_array_equal(dd.representatives(65_000, 1_000), rep[65_000:66_000])
    dd.close()


# ---- the contract of finalize and of what needs it ----
def test_finalize_contract(dev):
    k = 21
    rd = di.reads(k, False)
    rep, st = model(k, False)
    n = len(rep)
    d_seq, d_qual, d_off = to_device(rd)
    head, tail = di.split(rd, 0, 100), di.split(rd, 101, n)
    dd = Dedup(dev)
    # nothing added: an add of no reads launches nothing, and a finalize gives zeros
    dd.add(b"", np.zeros(1, dtype=np.uint64))
    dd.add_device(0, 0, 0)
    z = dd.finalize()
    assert (z.units, z.distinct, z.max_multiplicity, z.mult_hist.tolist()) == (0, 0, 0, [0] * 8)
    # before the units are there, nothing can be masked or scanned
    expect_arg_error(dd.representatives, 0, 1)
    dd.add(head[0], head[2])
    expect_arg_error(dd.mask_device, d_qual.data_ptr(), d_off.data_ptr(), 100)
    expect_arg_error(dd.scan, *head, k=k)
    # unit 100 is missing
    dd.add(tail[0], tail[2], first_unit=101)
    expect_arg_error(dd.finalize)
    expect_arg_error(dd.scan, *head, k=k)
    one = di.split(rd, 100, 101)
    dd.add(one[0], one[2], first_unit=100)
    assert_stats(dd.finalize(), st)
    np.testing.assert_array_equal(dd.representatives(0, n), rep)
    # a range past the units, another pairing, and a later add all refuse the three that need a finalize
    expect_arg_error(dd.representatives, n - 1, 2)
    expect_arg_error(dd.mask_device, d_qual.data_ptr(), d_off.data_ptr(), 100, first_unit=n - 50)
    expect_arg_error(dd.scan, *head, k=k, first_unit=n - 50)
    bad = Dedup(dev, paired=True)
    expect_arg_error(bad.add, one[0], one[2])  # an odd record count
    expect_arg_error(bad.add_device, d_seq.data_ptr(), d_off.data_ptr(), 3)
    bad.close()
    lib_scan = dd.scan(*head, k=k)
    assert lib_scan.total > 0
    dd.paired = True  # (the Python object's flag only: params->paired now differs from the handle's)
    expect_arg_error(dd.scan, *di.split(rd, 0, 100), k=k)
    dd.paired = False
    extra = di.split(rd, 0, 7)
    dd.add(extra[0], extra[2], first_unit=n)
    expect_arg_error(dd.representatives, 0, n)
    expect_arg_error(dd.mask_device, d_qual.data_ptr(), d_off.data_ptr(), 100)
    expect_arg_error(dd.scan, *head, k=k)
    both = dd.finalize()  # everything added so far: the first seven units once more
    assert (both.units, both.distinct) == (n + 7, st["distinct"])
    np.testing.assert_array_equal(dd.representatives(n, 7), rep[:7])
    # a unit added twice can never be 0 .. N - 1 each once
    dd.add(one[0], one[2], first_unit=100)
    expect_arg_error(dd.finalize)
    dd.close()
    # unit indices stay below 2^32 - 1
    dd = Dedup(dev)
    expect_arg_error(dd.add_device, d_seq.data_ptr(), d_off.data_ptr(), 2, first_unit=2 ** 32 - 2)
    expect_arg_error(dd.add, one[0], one[2], first_unit=2 ** 32 - 1)
    dd.close()


# ---- the mask ----
@FLAVOURS
def test_mask_device_writes_the_dropped_records_and_nothing_else(dev, paired):
    import torch
    k = 21
    rd = di.reads(k, paired)
    seq, qual, off = rd
    rep, _ = model(k, paired)
    n, per = len(rep), 2 if paired else 1
    dd = Dedup(dev, paired)
    dd.add(seq, off)
    dd.finalize()
    exp = np.frombuffer(dm.mask(qual, off, rep, paired), np.uint8)
    assert (exp != np.frombuffer(qual, np.uint8)).any()
    # an over-allocated, poisoned buffer: the bytes past offsets[n] stay what they were
    pad = 4_099
    host = np.concatenate([np.frombuffer(qual, np.uint8), np.full(pad, 0xAB, np.uint8)])
    d_q = torch.from_numpy(host.copy()).cuda()
    d_off = torch.from_numpy(np.asarray(off).astype(np.int64)).cuda()
    dd.mask_device(d_q.data_ptr(), d_off.data_ptr(), per * n)
    torch.cuda.synchronize()
    got = d_q.cpu().numpy()
    np.testing.assert_array_equal(got[:len(exp)], exp)
    assert (got[len(exp):] == 0xAB).all()
    # a range of units in the middle, with offsets that do not start at 0: only its records are written
    u0, u1 = n // 4 + 1, n // 2
    d_q = torch.from_numpy(host.copy()).cuda()
    dd.mask_device(d_q.data_ptr(), d_off.data_ptr() + 8 * per * u0, per * (u1 - u0), first_unit=u0)
    torch.cuda.synchronize()
    got = d_q.cpu().numpy()
    a, b = int(off[per * u0]), int(off[per * u1])
    part = host.copy()
    part[a:b] = exp[a:b]
    assert (exp[a:b] != host[a:b]).any()
    np.testing.assert_array_equal(got, part)
    dd.close()


# ---- the deduplicated scan against the oracle on the removed reads ----
# each scan family once: the k-mer table (k = 21 with the anchor kernel tuned off), the anchor-and-extend kernel
# (k = 70, the default) and the LF-step kernel (k = 151, which the other two do not take)
FAMILY = {21: (dict(ax_scan=0), (1, 2)), 70: ({}, (3,)), 151: ({}, (0,))}


@FLAVOURS
@pytest.mark.parametrize("k", [21, 70, 151])
def test_scan_equals_the_oracle_on_the_removed_reads(k, paired):
    ref = ri.base_ref()
    tune, codes = FAMILY[k]
    d = DeviceIndex(base_index())
    d.tune(**tune)
    seq, qual, off = di.reads(k, paired)
    rep, _ = model(k, paired)
    removed = dm.remove(seq, qual, off, rep, paired)
    oracle = Oracle(ref.records, ref.groups, 3, k)
    dd = Dedup(d, paired)
    dd.add(seq, off)
    dd.finalize()
    u = 2.0 ** -53
    for local in (False, True):
        T, amb, U, W = oracle.scan(*removed, ri.CUTOFF, paired, local)
        got = dd.scan(seq, qual, off, k=k, phred_cutoff=ri.CUTOFF, local=local)
        assert d.tuning("last_kernel") in codes
        assert (got.total, got.ambiguous, got.unique.tolist()) == (T, amb, U.tolist()), (k, paired, local)
        assert T > 0 and U.sum() > 0
        if local:
            tol = (3 * k + 2 * U.astype(np.float64) + 2) * u * W
            assert (np.abs(got.weights - W) <= tol).all(), (got.weights, W)
        else:
            assert got.weights is None
        plain = d.scan(seq, qual, off, k=k, phred_cutoff=ri.CUTOFF, paired=paired, local=local)
        assert plain.total > got.total  # the duplicates carried windows
    # two calls with their first units add up to the one call
    cut = len(rep) // 2
    per = 2 if paired else 1
    a = dd.scan(*di.split((seq, qual, off), 0, per * cut), k=k, phred_cutoff=ri.CUTOFF)
    b = dd.scan(*di.split((seq, qual, off), per * cut, per * len(rep)), k=k, phred_cutoff=ri.CUTOFF, first_unit=cut)
    T, amb, U, _ = oracle.scan(*removed, ri.CUTOFF, paired, False)
    assert (a.total + b.total, a.ambiguous + b.ambiguous, (a.unique + b.unique).tolist()) == (T, amb, U.tolist())
    dd.close()
    d.close()


@FLAVOURS
def test_scan_with_an_em_histogram(dev, paired):
    k = 21
    ref = ri.base_ref()
    seq, qual, off = di.reads(k, paired)
    rep, _ = model(k, paired)
    removed = dm.remove(seq, qual, off, rep, paired)
    index = er.build_index(ref.records, ref.groups, 3, k)
    h = er.scan(index, 3, k, *removed, ri.CUTOFF, paired)
    whole = er.scan(index, 3, k, seq, qual, off, ri.CUTOFF, paired)
    assert 0 < h.n_windows < whole.n_windows
    dd = Dedup(dev, paired)
    dd.add(seq, off)
    dd.finalize()
    em = EmHistogram(dev)
    got = dd.scan(seq, qual, off, k=k, phred_cutoff=ri.CUTOFF, em=em)
    assert (got.total, got.unique.tolist()) == (h.total, h.unique)
    em.finalize()
    assert em.info() == (h.n_intervals, h.n_entries, h.n_windows)
    rows = em.rows()
    assert len({content for _, content in rows}) == len(rows)
    assert {content: m for m, content in rows} == h.merged
    em.close()
    dd.close()


# ---- files ----
@lru_cache(maxsize=None)
def case_index(name: str) -> FmIndex:
    c = Case(name)
    return FmIndex.build(c.records, c.groups, c.G, prefix_q=4, **FULL)


@pytest.mark.parametrize("name", ["tiny_single", "tiny_paired"])
def test_dedup_fastq_for_any_thread_count(name, tmp_path):
    """40,000 records: more than one of the sequential reader's 32,768-record blocks, so that a block's first record
    index matters. Plain and gzip, statistics and counters identical across thread counts and equal to the handle's own
    result on the same records in memory."""
    c = Case(name)
    k = c.ks[0]
    seqs, quals, paired = di.fastq_records(name)
    assert paired == c.paired
    local = not paired
    rd = ri.pack(seqs, quals)
    rep = dm.rep_fingerprint(rd[0], rd[2], paired)
    st = dm.stats(rep)
    assert st["distinct"] < st["units"] and st["max_multiplicity"] >= 3
    d = DeviceIndex(case_index(name))
    dd = Dedup(d, paired)
    dd.add(rd[0], rd[2])
    assert_stats(dd.finalize(), st)
    mem = dd.scan(*rd, k=k, phred_cutoff=c.cutoff, local=local)
    dd.close()
    T, amb, U, W = Oracle(c.records, c.groups, c.G, k).scan(*dm.remove(*rd, rep, paired), c.cutoff, paired, local)
    assert (mem.total, mem.ambiguous, mem.unique.tolist()) == (T, amb, U.tolist()) and T > 0
    if paired:
        paths = [(str(tmp_path / "r1.fq"), str(tmp_path / "r2.fq"), False)]
        di.write_fastq(paths[0][0], seqs, quals, 0, 2)
        di.write_fastq(paths[0][1], seqs, quals, 1, 2)
    else:
        paths = [(str(tmp_path / "r.fq"), None, False), (str(tmp_path / "r.fq.gz"), None, True)]
        for p, _, gz in paths:
            di.write_fastq(p, seqs, quals, gz=gz)
    for p1, p2, _ in paths:
        for threads in (1, 4):
            got_st, got = d.dedup_fastq(p1, p2, k=k, phred_cutoff=c.cutoff, local=local, threads=threads)
            assert_stats(got_st, st)
            assert (got.total, got.ambiguous, got.unique.tolist()) == (mem.total, mem.ambiguous, mem.unique.tolist())
            if local:  # sums of the same windows' weights in another order
                np.testing.assert_allclose(got.weights, mem.weights, rtol=1e-12, atol=0)
    # with a histogram: the rows of the in-memory scan
    em_f, em_m = EmHistogram(d), EmHistogram(d)
    d.dedup_fastq(paths[0][0], paths[0][1], k=k, phred_cutoff=c.cutoff, local=local, threads=4, em=em_f)
    dd = Dedup(d, paired)
    dd.add(rd[0], rd[2])
    dd.finalize()
    dd.scan(*rd, k=k, phred_cutoff=c.cutoff, local=local, em=em_m)
    em_f.finalize()
    em_m.finalize()
    assert em_f.info() == em_m.info() and sorted(em_f.rows()) == sorted(em_m.rows())
    for x in (em_f, em_m, dd, d):
        x.close()


@pytest.mark.parametrize("name,accuracy", [("tiny_single", None), ("tiny_paired", "0.99")])
def test_cli_dedup_file(name, accuracy, tmp_path):
    """`speq all --dedup FILE` on the golden reads with copies inserted: stderr, stdout and -o are byte-identical to the
    run without the option, FILE's header holds the model's statistics, and its deduplicated columns are, formatted
    %.6f, what the Python API gives for the FASTQ of the unique records: the initial percentages of a scan with an EM
    histogram, refined by em_refine with the run's cutoffs."""
    c = Case(name)
    k = c.ks[0]
    local = accuracy is None
    uniq, dup, paired = di.cli_records(name)
    precision, max_it = 1e-4, 50
    outs = {}
    for tag in ("plain", "dedup"):
        d = tmp_path / tag
        d.mkdir()
        for f in ("refs.fa", "groups.txt"):
            shutil.copy(os.path.join(c.dir, f), d / f)
        for units, stem in ((dup, "dup"), (uniq, "uniq")):
            s, q = [x for u in units for x, _ in u], [x for u in units for _, x in u]
            if paired:
                di.write_fastq(str(d / f"{stem}_1.fq"), s, q, 0, 2)
                di.write_fastq(str(d / f"{stem}_2.fq"), s, q, 1, 2)
            else:
                di.write_fastq(str(d / f"{stem}_1.fq"), s, q)
        args = ["all", "-r", "refs.fa", "-g", "groups.txt", "-1", "dup_1.fq"]
        if paired:
            args += ["-2", "dup_2.fq"]
        args += ["-x", "ref", "-k", str(k), "--phred-cutoff", str(c.cutoff), "--prefix-q", "4", "-o", "p.txt",
                 "--precision-cutoff", str(precision), "--max-em-iterations", str(max_it)]
        if accuracy:
            args += ["--fixed-accuracy", accuracy]
        if tag == "dedup":
            args += ["--dedup", "f.tsv"]
        r = subprocess.run([SPEQ] + args, cwd=d, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        outs[tag] = (r.stderr, r.stdout, (d / "p.txt").read_bytes())
    assert outs["plain"] == outs["dedup"]
    assert not (tmp_path / "plain" / "f.tsv").exists()
    lines = (tmp_path / "dedup" / "f.tsv").read_text().splitlines()
    flat = di.flatten(dup)
    st = dm.stats(dm.rep_fingerprint(flat[0], flat[2], paired))
    assert st["distinct"] == len(uniq) and st["units"] == len(dup)
    assert lines[:7] == [f"# units {st['units']}", f"# distinct {st['distinct']}",
                         f"# duplicates {st['units'] - st['distinct']}",
                         "# duplicate_fraction %.6f" % ((st["units"] - st["distinct"]) / st["units"]),
                         f"# max_multiplicity {st['max_multiplicity']}",
                         "# multiplicity_hist " + " ".join(str(int(x)) for x in st["mult_hist"]),
                         "name\tpercent\tpercent_dedup\trefined\trefined_dedup"]
    # the Python API on the unique records
    dev = DeviceIndex(case_index(name))
    grp = file_to_map(os.path.join(c.dir, "groups.txt"))
    u_ref, tot_ref = dev.count_unique_kmers_per_group(k)

    def percentages(stem: str):
        em = EmHistogram(dev)
        d = tmp_path / "dedup"
        res, _ = dev.scan_fastq(str(d / f"{stem}_1.fq"), str(d / f"{stem}_2.fq") if paired else None, k=k,
                                phred_cutoff=c.cutoff, local=local, em=em)
        em.finalize()
        totals = res.weights if local else res.unique.astype(np.float64) / float(accuracy) ** k
        first = unique_to_percent(totals, res.total, u_ref, tot_ref)
        steps = em_refine(lambda p: em.step(p, grp.counts, res.unique), totals, res.total, first, precision, max_it)
        em.close()
        return first, (steps[-1][0] if steps else first)

    first_u, last_u = percentages("uniq")
    first_d, last_d = percentages("dup")
    assert len(lines) == 7 + c.G
    moved = False
    for line, nm, g in zip(lines[7:], grp.names, range(c.G)):
        f = line.split("\t")
        assert len(f) == 5 and f[0] == nm
        assert f[2] == "%.6f" % first_u[g] and f[4] == "%.6f" % last_u[g], (nm, f, first_u[g], last_u[g])
        assert abs(float(f[1]) - first_d[g]) <= 1e-6 and abs(float(f[3]) - last_d[g]) <= 1e-6
        moved |= f[1] != f[2]
    assert moved  # the copies had moved the percentages
    dev.close()
